/* ot_matrix_plan.h -- the pure-host part of --ot_matrix (include/linreg_gc_ot_matrix.h): the magic word and the rule that cuts
 * the rows of a provider pair's block into batches.  Both providers of a pair call it with the same arguments, so they agree on
 * every batch without a message.  No GPU, no sockets: tests/tools/asan_ot_matrix.c runs it under the sanitizers. */
#ifndef LINREG_OT_MATRIX_PLAN_H
#define LINREG_OT_MATRIX_PLAN_H
#include <stddef.h>
#include <stdint.h>

#define OTM_MAGIC 0x4d58544d544f474cull          /* "LGOTMTXM" as little-endian bytes: sent each way after the base OTs */
#define OTM_MAX_OTS ((uint64_t)1 << 24)          /* OTs per batch: the per-pair mode's batch (256 MiB of u) */
#define OTM_MAX_Y_BYTES ((uint64_t)256 << 20)    /* bytes of y per batch */

/* rows of a batch (the last one may be shorter) between a receiver with r columns and a sender with s at width w (32 or 64): as
 * many whole rows as keep rows r w <= OTM_MAX_OTS and rows r w s w / 8 <= OTM_MAX_Y_BYTES, and at least one */
size_t otm_batch_rows(size_t r, size_t s, int w);

/* --ot_half (include/linreg_gc_ot_half.h): its own magic word, and the same rule on the half y of a row,
 * r (w / 2 + 1) s w / 8 bytes: where y binds, a batch holds about twice the rows */
#define OTM_HALF_MAGIC 0x464c4854544f474cull     /* "LGOTTHLF" as little-endian bytes */
size_t otm_half_batch_rows(size_t r, size_t s, int w);
#endif
