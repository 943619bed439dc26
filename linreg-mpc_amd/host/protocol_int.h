/* protocol_int.h -- what the files of the host protocol share among themselves (protocol.c, tables.c, phase1_ti.c,
 * phase1_party.c, phase1_matrix.c, phase1_ot.c, phase1_ot_matrix.c); not part of what bin/linreg and the benchmark binaries see
 * (protocol.h).  Phase 1's mode and its pair plans are phase1_plan.h's. */
#ifndef LINREG_PROTOCOL_INT_H
#define LINREG_PROTOCOL_INT_H
#include "ot_pipe.h"
#include "protocol.h"

/* protocol.c */
extern size_t g_pmsg_limit;
uint8_t *frame_pmsg(const uint64_t *vec, size_t n, uint64_t value, size_t *len);      /* a length-prefixed proto2 message, malloc'd */
/* readdata.c */
int read_own_columns(FILE *f, size_t n, size_t d, size_t c0, size_t c1, int own_y, int precision, double normalizer, int w2,
                            int64_t *Xq, int64_t *yq);
int read_own_columns_threads(FILE *f, size_t n, size_t d, size_t c0, size_t c1, int own_y, int precision, double normalizer, int w2,
                             int64_t *Xq, int64_t *yq, int threads);
int read_own_columns_rows(FILE *f, size_t n, size_t d, size_t c0, size_t c1, int own_y, int precision, const double *row_norm, int w2,
                          int64_t *Xq, int64_t *yq);
/* phase1_ti.c */
void tune_malloc(void);
size_t p1_plan_of(const config *c, size_t M, p1_pair **out);    /* p1_plan_ti on the configuration's column owners */
/* --ti_ring: a provider's cross part (whole files only: c->n rows) */
int run_party_ti_ring(node *self, config *c, lgc_p1 *p1, int device, uint64_t *share_A, uint64_t *share_b);
/* phase1_matrix.c: --ti_matrix, the initializer's run for n rows and a provider's cross part */
int run_trusted_initializer_matrix(node *self, config *c, size_t n, int w1, int device, const uint8_t master[16]);
int run_party_ti_matrix(node *self, config *c, lgc_p1 *p1, size_t n, int w1, uint64_t *share_A, uint64_t *share_b);
/* phase1_ot.c: the cross part of a provider for n rows in the OT transport of `mode` */
int run_party_ot(node *self, config *c, int device, size_t n, const int64_t *Xq, const int64_t *yq, int w1, const p1_mode *mode,
                 uint64_t *share_A, uint64_t *share_b);
/* one provider pair of it: the role, the session, the mode's batches -- `per` of `total` units each (pairs of columns; rows of the
 * matrix mode's block), the last batch what is left -- and the batch pipeline, whose callbacks get the ot_pair (ot_pipe.h) */
typedef struct {
    node *self; int peer;                       /* peer: 1-based party number */
    int i_am_sender, device;
    const int64_t *Xq, *yq; size_t n, d; int w1;
    lgc_ot_sender *S; lgc_ot_receiver *R;       /* the one of this party's role */
    const size_t *cols;                         /* this party's column (d: y) of each pair; matrix mode: its ncols columns of the r x s block */
    size_t ncols, r, s, total, per;
    const struct ot_block_form *form;           /* matrix mode: its payload form (--ot_half or not), phase1_ot_matrix.c's */
    uint64_t *shares, *part;                    /* malloc'd: a word per pair; matrix mode: the block summed over the batches, and one batch's */
    uint64_t *vals;                             /* page-locked: a batch of the own operand, gathered */
    ot_pipe pipe;                               /* u and y page-locked: two each as the sender, else one */
} ot_pair;
static inline size_t ot_pair_batch(const ot_pair *o, size_t k) { return o->total - k * o->per < o->per ? o->total - k * o->per : o->per; }
int ot_pair_open(ot_pair *o);                   /* the base OTs in this party's role and its session */
/* total, per and what the callbacks read are set: buffers for the largest batch, then this party's role through the pipeline */
int ot_pair_run(ot_pair *o, const ot_pipe *calls, size_t vals_bytes, size_t u_bytes, size_t y_bytes);
void ot_pair_close(ot_pair *o);                 /* the session, every buffer, shares and part: from any state */
int ot_put_blob(void *pair, const void *buf, size_t len);                           /* ot_pipe's put: send_blob to the peer */
/* the status of a liblinreg_gc call, its message printed where it failed */
static inline int lgc_said(int rc) { if (rc) fprintf(stderr, "%s\n", lgc_last_error()); return rc; }
/* phase1_ot_matrix.c: --use_ot --ot_matrix, one vector OT per operand bit (include/linreg_gc_ot_matrix.h); the batch rule and the
 * magic word are ot_matrix_plan.h's.  One provider pair: sender columns [i0, i1) against receiver columns [j0, j1), with y where
 * that side is the last provider; half: --ot_half, that mode's half-payload form (include/linreg_gc_ot_half.h) */
int run_party_ot_matrix_pair(ot_pair *o, int half, size_t i0, size_t i1, int y_on_sender, size_t j0, size_t j1, int y_on_receiver,
                             uint64_t *share_A, uint64_t *share_b);
/* the per-pair mode's hint when the length prefix of a blob (recv_blob_prefix) turns out to be the matrix mode's magic word */
void otm_hint_if_magic(uint64_t prefix);
#endif
