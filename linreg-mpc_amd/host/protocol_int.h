/* protocol_int.h -- what the files of the host protocol share among themselves (protocol.c, tables.c, phase1_ti.c,
 * phase1_party.c); not part of what bin/linreg and the benchmark binaries see (protocol.h). */
#ifndef LINREG_PROTOCOL_INT_H
#define LINREG_PROTOCOL_INT_H
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
extern int g_ti_ring;                                    /* --ti_ring (protocol_set_ti_ring) */
/* --scan=M (protocol_set_scan): the last M of the d feature columns are the candidates of an association scan.  No model holds
 * two of them, so every side -- the initializer, both peers of a pair, the OT threads -- leaves the pairs (i, j) with both
 * columns in the candidate block and i != j out of its loops, in the same loop order: the message streams stay aligned */
extern size_t g_scan;
static inline int scan_skips(size_t d, size_t i, size_t j) { return g_scan && i < d && j < d && i != j && i >= d - g_scan && j >= d - g_scan; }
void tune_malloc(void);
/* phase1_matrix.c: --ti_matrix (protocol_set_ti_matrix), the initializer's run for n rows and a provider's cross part */
extern int g_ti_matrix;
int run_trusted_initializer_matrix(node *self, config *c, size_t n, int w1, int device, const uint8_t master[16]);
int run_party_ti_matrix(node *self, config *c, lgc_p1 *p1, size_t n, int w1, uint64_t *share_A, uint64_t *share_b);
/* phase1_ot_matrix.c: --use_ot --ot_matrix (protocol_set_ot_matrix), one vector OT per operand bit (include/linreg_gc_ot_matrix.h);
 * the batch rule and the magic word are ot_matrix_plan.h's */
extern int g_ot_matrix;
/* peer: 1-based; cols_s / cols_r: the sender's and the receiver's columns (d: y); blk_dst[ir * s + j]: where that word is added */
int run_party_ot_matrix_pair(node *self, int peer, int i_am_sender, int device, const int64_t *Xq, const int64_t *yq, size_t n, size_t d,
                             int w1, const size_t *cols_s, size_t s, const size_t *cols_r, size_t r, uint64_t **blk_dst);
/* the per-pair mode's hint when the length prefix of a blob (recv_blob_prefix) turns out to be the matrix mode's magic word */
void otm_hint_if_magic(uint64_t prefix);
int run_party_ti_ring(node *self, config *c, lgc_p1 *p1, int device, uint64_t *share_A, uint64_t *share_b);
#endif
