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
int run_party_ti_ring(node *self, config *c, lgc_p1 *p1, int device, uint64_t *share_A, uint64_t *share_b);
#endif
