/*
 * linreg_gc_scan.h -- an association scan: M candidate columns, each fitted with the same shared covariates, in one secure
 * solve (liblinreg_gc.so).
 *
 * c covariate columns C (intercept, age, sex, principal components) are shared; each of M candidate columns g_m (genotypes,
 * probes, features) is tested one at a time in the model y ~ [C, g_m], and only the candidate's own coefficient -- and its
 * standard error -- is revealed.  M runs of the plain solve would repeat phase 1 on the covariates and factor the same c x c
 * block M times; one solve on all c + M columns would form the M^2 / 2 cross products between candidates that no model needs
 * and fit the wrong, joint model.  The calls here factor the covariate block once; candidate m is one more row of the Cholesky
 * factor, and rows never meet one another.  All arithmetic mod 2^width; mul, div, sqrt, mulc and q(.) are the word machine's,
 * exactly as linreg_gc_inference.h states them, with d := D.
 *
 * Sizes.  D = c + 1 is the size of each fitted system and what lgc_system.d holds for a scan (D >= 2); the algorithm is
 * LGC_ALG_CHOLESKY.  Every share is, with T_c = c (c + 1) / 2,
 *   [A (T_c)] [b (c)] [yy (1)] [h_0 (c)] .. [h_{M-1} (c)] [gg (M)] [gy (M)]
 * T_c + c + 1 + M (c + 2) words: lgc_solver_set_shares takes nshares rows of that many and lgc_party_input_bits is that many
 * times the width.  A, b, yy are the covariates' Gram triangle, (C_k, y) and (y, y) as linreg_gc_inference.h has them;
 * h_m[k] = (g_m, C_k), gg_m = (g_m, g_m), gy_m = (g_m, y).
 *
 * Definition.
 *   assembly   the plain solve's, with normaliser D: share sums; with normalize = 1 the off-diagonals of A, b, yy, every h_m[k]
 *              and every gy_m are divided by D (truncating, OP_IDIVC) and q(lambda) is added to every A_kk and every gg_m --
 *              phase 1 delivers diagonals already divided, as it always has; with normalize = 0 the words are used as given
 *   L          the Cholesky factor of the c x c block; y_k the forward substitution of b; E0 = Y - sum_k mul(y_k, y_k)
 *              (Y: the assembled yy) -- the shared prefix, lowered once
 *   u_m[k]     div(h_m[k] - sum_{j<k} mul(L_kj, u_m[j]), L_kk),  k = 0 .. c - 1
 *   l_m        sqrt(gg_m - sum_k mul(u_m[k], u_m[k]))
 *   t_m        div(gy_m - sum_k mul(u_m[k], y_k), l_m)
 *   beta_m     div(t_m, l_m)
 * and with LGC_SCAN_SE
 *   z_m        div(2^p, l_m);   v_m = mul(z_m, z_m)
 *   e_m        E0 - mul(t_m, t_m)
 *   s2_m       mulc(e_m, q(resid_scale)): resid_scale is a public real, n / (n - D) for the unbiased estimate
 *   w_m        sqrt(mul(s2_m, v_m)): the standard error of beta_m is w_m / sqrt(n), divided on the host in double
 * These are, operation for operation, row c of the plain Cholesky program on the augmented D x D system [C, g_m] followed by
 * the first step of its back substitution: beta_m is bit for bit the last coefficient the plain LGC_ALG_CHOLESKY solve reveals
 * on that augmented system.  e_m is the mean squared residual exactly when q(lambda) = 0; for lambda > 0 it overstates it by
 * lambda |beta|^2, because forming |beta|^2 would need the full back substitution per candidate: the term is not added.
 * With normalize = 1 everything is in units of the system divided by D, in which w_m is a ratio where D cancels.
 *
 * Revealed.  lgc_solver_get_beta and the beta of lgc_party_finish hold beta_0 .. beta_{M-1} and, with LGC_SCAN_SE, then
 * w_0 .. w_{M-1}.  Nothing else is revealed, and no covariate coefficient: L, y, U, l, t, z, v, e, s2 stay garbled words.
 *
 * Range condition: the inference header's -- every u_m[k], v_m, s2_m and mul(s2_m, v_m) fits in width - 1 - precision integer
 * bits.  With normalize = 1, v_m is D times the variance-inflation factor of the candidate given the covariates.
 *
 * Lowering.  No new record kind.  U is M x c, row-major; step k of all M candidates rides in covariate column
 * k's batch of dot products and in its division launch, so no launch is added to a dependent chain that grows with M; a tail
 * of one batch of 2 M dot products of length c, M square roots, the divisions, products and reveals follows.  Launches of M
 * records are cut by the launch caps as every launch is.  lgc_party_program_fingerprint covers M, the reveal bits and
 * q(resid_scale); the table-ring modes and the statistics work on the objects created here.
 * Rejected with LGC_EINVAL: any algorithm but LGC_ALG_CHOLESKY; sys->d < 2; M = 0 or M > LGC_MAX_SCAN; a system with trace or
 * reveal_inputs set; reveal bits other than 0 or LGC_SCAN_SE; with LGC_SCAN_SE a resid_scale the inference calls reject (not
 * finite and positive, or q does not fit below the sign bit); a program whose word ids do not fit 31 bits.
 *
 * Phase 1.  lgc_p1_set_divisor(h, divisor) sets the divisor of the floating-point diagonal for every later call on h (the
 * default is the column count d, so existing callers see no change; LGC_EINVAL on 0): a scan's providers set c + 1.
 * lgc_p1_local_scan(h, c0, c1, s0, s1, with_y, out_H, out_gg, out_gy): the own covariate columns are [c0, c1) (may be empty),
 * the own candidate columns [s0, s1) (non-empty, disjoint from the covariates).  out_H[m (c1 - c0) + i] = (column s0 + m,
 * column c0 + i) mod 2^width, out_gg[m] the floating-point diagonal of column s0 + m with the object's divisor, out_gy[m] =
 * (column s0 + m, y) with with_y set -- every word bit-identical to the corresponding word of lgc_p1_local over a range holding
 * both columns.  out_H may be null when c1 == c0, out_gy when with_y is 0.  The call honours lgc_p1_set_rows and device I/O as
 * the other local calls do.  LGC_EINVAL: a null handle or out_gg, ranges out of order, past d or overlapping, with_y on an
 * object without y.
 */
#ifndef LINREG_GC_SCAN_H
#define LINREG_GC_SCAN_H
#include "linreg_gc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LGC_SCAN_SE 1              /* w_0 .. w_{M-1} behind the coefficients */
#define LGC_MAX_SCAN (1u << 20)    /* candidate columns of one scan */

int lgc_program_build_scan(struct lgc_program **out, const lgc_system *sys, size_t M, double resid_scale, int reveal);
int lgc_solver_create_scan(lgc_solver **out, int device, const lgc_system *sys, const uint8_t seed[16], size_t M, double resid_scale, int reveal);
int lgc_party_create_scan(lgc_party **out, int device, const lgc_system *sys, int role, const uint8_t seed[16],
                          size_t max_launch_table_bytes, size_t M, double resid_scale, int reveal);
int lgc_p1_set_divisor(lgc_p1 *h, size_t divisor);
int lgc_p1_local_scan(lgc_p1 *h, size_t c0, size_t c1, size_t s0, size_t s1, int with_y,
                      uint64_t *out_H, uint64_t *out_gg, uint64_t *out_gy);

#ifdef __cplusplus
}
#endif
#endif
