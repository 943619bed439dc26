/*
 * linreg_gc_targets.h -- several target columns against the same features in one secure solve (liblinreg_gc.so).
 *
 * Not part of the drop-in surface of linreg_gc.h: the reference solves one b per circuit and has no counterpart for these
 * calls.  A program with k targets factors A (Cholesky, LDL^T) or multiplies by it (CGD) once and carries k right-hand
 * sides through the launches a single solve already has; target t performs exactly the operations of a single-target solve
 * with b = b_t, so beta_t is bit-identical to that solve.  k = 1 is today's program, record for record.
 *
 * Sizes on objects created here (T = d(d+1)/2):
 *   shares     nshares x (T + k d), share-major: [A packed lower triangle (T)] [b_0 (d)] ... [b_{k-1} (d)]
 *              (lgc_solver_set_shares; the data-provider path sums and normalises every b_t as it does b)
 *   beta       k x d, target-major (lgc_solver_get_beta, lgc_party_finish)
 *   inputs     T + k d: A, then b_0 .. b_{k-1} (lgc_solver_get_inputs, lgc_party_finish; reveal_inputs)
 *   input bits (T + k d) x width per share (lgc_party_input_bits)
 * Rejected with LGC_EINVAL: k = 0 or k > LGC_MAX_TARGETS, and trace with k > 1.  Every other linreg_gc.h call works on
 * these objects unchanged; lgc_party_program_fingerprint differs between target counts.
 */
#ifndef LINREG_GC_TARGETS_H
#define LINREG_GC_TARGETS_H
#include "linreg_gc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LGC_MAX_TARGETS 256

/* ---- phase 2 */
/* the lowered program (host only, no GPU needed; the lgc_program calls of linreg_gc_debug.h introspect and destroy it) */
struct lgc_program;
int lgc_program_build_targets(struct lgc_program **out, const lgc_system *sys, size_t k);
int lgc_solver_create_targets(lgc_solver **out, int device, const lgc_system *sys, const uint8_t seed[16], size_t k);
int lgc_party_create_targets(lgc_party **out, int device, const lgc_system *sys, int role, const uint8_t seed[16],
                             size_t max_launch_table_bytes, size_t k);
size_t lgc_solver_num_targets(const lgc_solver *s);   /* 1 for objects of linreg_gc.h */
size_t lgc_party_num_targets(const lgc_party *p);

/* ---- phase 1 with k target columns */
/* The device array is n x (d + k): X, then the targets.  On such a handle lgc_p1_mask, lgc_p1_dot and lgc_p1_ti_a[_batch]
 * take column index d + t as target t, and lgc_p1_local's with_y means target 0. */
int lgc_p1_create_targets(lgc_p1 **out, int device, size_t n, size_t d, size_t k, int width, int precision);
/* Xq: n x d row-major, Yq: n x k row-major or NULL (targets zero) -- fixed point, sign-extended when width == 32 */
int lgc_p1_set_targets(lgc_p1 *h, const int64_t *Xq, const int64_t *Yq);
/* What a data provider computes alone for its own columns [c0, c1): out_A as lgc_p1_local (packed lower triangle, the
 * double-precision diagonal), out_B[t][i] = <column c0 + i, target t> mod 2^width, k x (c1 - c0) (NULL: not wanted). */
int lgc_p1_local_targets(lgc_p1 *h, size_t c0, size_t c1, uint64_t *out_A, uint64_t *out_B);

#ifdef __cplusplus
}
#endif
#endif
