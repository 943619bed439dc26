/* ti_matrix_plan.h -- the pure-host part of --ti_matrix (include/linreg_gc_p1_matrix.h): which provider pairs run an instance
 * of the matrix-triple protocol and on which columns, where a share block lands, and the initializer's messages.  No device,
 * no sockets: the initializer and every provider derive the same plan from the column ownership alone. */
#ifndef LINREG_TI_MATRIX_PLAN_H
#define LINREG_TI_MATRIX_PLAN_H
#include <stddef.h>
#include <stdint.h>

/* the first 8 bytes the initializer sends a provider in matrix mode.  A default-mode provider reads them as the length prefix of
 * a protobuf message and refuses it (far beyond the bound of pmsg_set_limit); a matrix-mode provider refuses anything else */
#define TM_MAGIC 0x4d5854414d49544cull          /* "LTIMATXM" as little-endian bytes */

/* one instance: provider A = party index hi (the higher columns; column d, y, can only be among cols_a), B = party index lo */
typedef struct {
    int lo, hi;
    uint64_t u;                 /* the instance number: the seeds are blocks 3u .. 3u + 2 of the master seed's keystream */
    uint32_t *cols_a, *cols_b;  /* a and b column indices, ascending */
    size_t a, b;
} tm_inst;

/* owner[i], i <= d: the 0-based party index that holds column i (column d is y).  Every pair (lo, hi) of providers, lo ascending
 * then hi ascending, takes the next u; pairs where a side holds no column are numbered but not listed.  Returns the number of
 * instances in *out (malloc'd; tm_plan_free), or (size_t)-1 when out of memory */
size_t tm_plan(const int *owner, size_t d, int num_parties, tm_inst **out);
void tm_plan_free(tm_inst *v, size_t count);
/* blk[i][j] (a x b words) = the share of <column cols_a[i], column cols_b[j]>: into share_A[idx(., .)], or share_b[.] for y */
void tm_scatter(const tm_inst *t, const uint64_t *blk, size_t d, uint64_t *share_A, uint64_t *share_b);
/* the initializer's messages: to A seed_a | seed_s (32 bytes); to B seed_b | T (16 + a b W / 8 bytes, malloc'd by tm_msg_b) */
enum { TM_MSG_A_BYTES = 32 };
size_t tm_msg_b_bytes(const tm_inst *t, int width);
void tm_msg_a(const uint8_t seed_a[16], const uint8_t seed_s[16], uint8_t out[TM_MSG_A_BYTES]);
uint8_t *tm_msg_b(const tm_inst *t, int width, const uint8_t seed_b[16], const void *T, size_t *len);
#endif
