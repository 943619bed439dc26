/*
 * linreg_gc_inference.h -- standard errors, the residual variance and R^2 from the Cholesky solve (liblinreg_gc.so).
 *
 * Every other program reveals beta and nothing else.  No party can form a residual (the rows are split between the
 * providers) or a standard error ((X^T X)^-1 exists only inside the circuit, as the Cholesky factor the solve overwrites M
 * with), so what summary(lm), statsmodels and sklearn print beside the coefficients can only come from the circuit.  The
 * calls here lower the plain LGC_ALG_CHOLESKY solve, operation for operation, and behind it the diagonal of M^-1 (a forward
 * substitution of the d unit vectors: with M = L L^T, (M^-1)_jj = |L^-1 e_j|^2, no back substitution) and the mean squared
 * residual, from one extra input word.  All arithmetic mod 2^width; mul, div, sqrt are the word machine's, q(v) =
 * (int64)(v 2^precision) is how lgc_system.lambda is quantised, mulc(x, c) = mul(x, the word c) for a public c >= 0.
 *
 * Sizes.  Every share is [A (T)] [b (d)] [yy (1)], T = d (d + 1) / 2: lgc_solver_set_shares takes nshares x (T + d + 1)
 * words and lgc_party_input_bits is (T + d + 1) x width.  yy is an additive share of sum_q y_q y_q mod 2^64, masked to the
 * width -- the integer Gram entry (y, y), the arithmetic of the entries of b -- non-zero only from the provider that holds y.
 * lgc_p1_local_yy(h, c0, c1, out_A, out_b, out_yy) is lgc_p1_local(h, c0, c1, 1, out_A, out_b), the same launches, out_A and
 * out_b word for word, and additionally returns that entry, which the Gram launch has always formed with the rest of the lower
 * triangle and the older call drops (lgc_p1_local_folds_yy, linreg_gc_folds_yy.h, is the same thing per row fold: its K words
 * sum to this one mod 2^width).  LGC_EINVAL: what lgc_p1_local rejects; an object without y; a null out_b or out_yy.
 *
 * Definition.
 *   M, b       the input assembly of the plain solve, lambda included: share sums; with normalize = 1 the off-diagonals and b
 *              divided by the public normaliser d, and q(lambda) added to the diagonal
 *   Y          the share sum of yy, with normalize = 1 divided by d as the words of b are, in the launches that divide b
 *   b0         b as assembled (the forward substitution overwrites b)
 *   L, beta    the Cholesky program; beta is bit for bit what the plain solve reveals on the same (A, b)
 *   z_j        column j of L^-1, j = 0 .. d - 1:  z_j[i] = 0 (i < j),  z_j[j] = div(2^p, L_jj),
 *              z_j[i] = div(0 - sum_{k=j}^{i-1} mul(L_ik, z_j[k]), L_ii) (i > j)
 *   v_j        sum_{i>=j} mul(z_j[i], z_j[i])                              = (M^-1)_jj
 *   e          Y - sum_i mul(b0_i, beta_i) - mulc(sum_i mul(beta_i, beta_i), q(lambda))   (the last term absent when
 *              q(lambda) = 0; q(lambda) enters here on both input paths): the mean squared residual, exact for the solution
 *              of (X^T X / n + lambda I) beta = X^T y / n
 *   s2         mulc(e, q(resid_scale)): resid_scale is a public real, n / (n - d) for the unbiased estimate
 *   u_j        sqrt(mul(s2, v_j)): the standard error of beta_j is u_j / sqrt(n).  n is public and the division happens on the
 *              host in double -- a division by n inside the circuit would cost width 32 most of its precision
 *   r2         2^p - div(e, Y)
 * At lambda = 0 these are the OLS quantities.  For lambda > 0, u_j^2 / n is sigma^2 ((X^T X + n lambda I)^-1)_jj: the usual
 * ridge, or posterior, form -- not the sandwich.  e is used as computed: a fit exact to the ulp can make it a negative word,
 * and the result is then what sqrt and div give on that word.  On studentised data every quantity is in studentised units.
 * With normalize = 1 the whole system is the caller's divided by the public normaliser d (lambda counts in those units, as
 * it always has), so e and s2 are the mean squared residual and the residual variance divided by d: the host multiplies the
 * revealed s2 by d (bin/linreg and the binding's summary() do).  u_j and r2 are ratios in which d cancels.
 *
 * Revealed.  lgc_solver_get_beta and the beta of lgc_party_finish hold, in this order,
 *   beta                           d words
 *   u_0 .. u_{d-1}                 d words, with LGC_INFER_SE
 *   s2, r2                         2 words, with LGC_INFER_FIT
 * Everything else stays garbled words: L, the z columns, v, e, Y, b0.  resid_scale and the reveal bits are public.  With
 * LGC_INFER_FIT alone the inverse columns are not lowered at all: the program is the plain solve plus two short dot products.
 *
 * Range condition: the plain solve's, and every z_j[i], v_j, Y, sum_i mul(beta_i, beta_i), s2 and mul(s2, v_j) fit in
 * width - 1 - precision integer bits.  At precision 56 of 64 that is seven bits: v_j < 128.  For studentised columns v_j is
 * the variance-inflation factor of column j.
 *
 * Lowering.  No new record kind and no launch added to the dependent chain of the factorisation: step i of
 * the inverse columns j < i rides in column i's batch of dot products, its divisions and z_i[i] in column i's division launch
 * (d + 1 records instead of d - i); with Karatsuba products the z words lie inside the factorisation's shadow.
 * lgc_party_program_fingerprint covers the reveal bits and q(resid_scale).  The table ring modes, lgc_solver_get_inputs
 * (reveal_inputs: T + d + 1 words, Y last) and the statistics work on the objects created here.
 * Rejected with LGC_EINVAL: any algorithm but LGC_ALG_CHOLESKY; a system with trace set; reveal = 0 or bits other than the two
 * below; a resid_scale that is not finite and positive, or whose q does not fit below the sign bit; a program whose word ids
 * do not fit 31 bits.
 */
#ifndef LINREG_GC_INFERENCE_H
#define LINREG_GC_INFERENCE_H
#include "linreg_gc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LGC_INFER_SE  1   /* u_0 .. u_{d-1} behind beta */
#define LGC_INFER_FIT 2   /* then s2, r2 */

int lgc_program_build_inference(struct lgc_program **out, const lgc_system *sys, double resid_scale, int reveal);
int lgc_solver_create_inference(lgc_solver **out, int device, const lgc_system *sys, const uint8_t seed[16], double resid_scale, int reveal);
int lgc_party_create_inference(lgc_party **out, int device, const lgc_system *sys, int role, const uint8_t seed[16],
                               size_t max_launch_table_bytes, double resid_scale, int reveal);
int lgc_p1_local_yy(lgc_p1 *h, size_t c0, size_t c1, uint64_t *out_A, uint64_t *out_b, uint64_t *out_yy);

#ifdef __cplusplus
}
#endif
#endif
