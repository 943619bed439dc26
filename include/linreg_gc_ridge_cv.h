/*
 * linreg_gc_ridge_cv.h -- the ridge lambda sweep cross-validated over K folds inside the circuit; only the refit is revealed
 * (liblinreg_gc.so).
 *
 * The per-lambda sweep of linreg_gc_sweep.h reveals all count x d coefficients and leaves the choice of lambda to somebody
 * outside the circuit, who holds no validation data.  The calls here do what RidgeCV and cv.glmnet(alpha = 0) do, for the
 * headline solvers (cgd, cholesky, ldlt): K train / validation pairs, the K scores of every lambda summed before the
 * arg-min, and one model, refitted on ALL rows at the winning lambda.  Public K, 2 <= K <= LGC_MAX_FOLDS; a public grid of
 * L values lambda_0 .. lambda_{L-1}, 1 <= L <= LGC_MAX_RIDGE_CV_VALUES, each quantised as lgc_system.lambda is;
 * lgc_system.lambda itself is ignored, as the sweep ignores it.  All arithmetic mod 2^width.
 *   F_k        fold k, assembled from the shares exactly as linreg_gc_lasso_cv.h assembles it: share sums; with
 *              normalize = 1 the off-diagonal entries and b are then divided by the public normaliser d, the diagonal is
 *              left as summed; no lambda.  Fold inputs never contain lambda.
 *   tot        sum_k F_k, entry by entry
 *   training system k   entry = tdiv(tot - F_k, K - 1) (truncating; K = 2: no division);  full system (index K): tdiv(tot, K)
 *   fits       for every system s = 0 .. K and value l: M_{s,l} = system s with q(lambda_l) added to its diagonal, on BOTH
 *              input paths, and beta_{s,l} = bit for bit what the single-solve program of lgc_system.algorithm (cgd with
 *              num_iterations, cholesky, ldlt) reveals on the normalize = 0 two-share path with share 1 = (M_{s,l}, b_s)
 *              packed and share 2 = 0
 *   score_k,l  the selection's score (linreg_gc_lasso_select.h) of beta_{k,l} on the lambda-free fold F_k:
 *              t_i = sum_j mul(F_k.M_ij, beta_j), r_i = 2 b_k,i - t_i, score = 0 - sum_i mul(beta_i, r_i)
 *   cv_l       sum_k score_k,l
 *   l*         the smallest l whose cv_l is minimal under a SIGNED compare;  beta* = beta_{K,l*}, the full-data refit
 * Folds weigh equally whatever their row counts: a caller should make them equal in size to within one row.
 * Range condition: the cross-validation's (linreg_gc_lasso_cv.h) -- the selection's for every fold, and tot, every
 * 2 b_k and every cv_l fit in width - 1 - precision integer bits -- besides what each single solve needs for its own system.
 *
 * Sizes.  The share layout is the lasso cross-validation's: every share is [A_0 (T)] [b_0 (d)] ... [A_{K-1} (T)] [b_{K-1} (d)],
 * T = d (d + 1) / 2; lgc_solver_set_shares takes nshares x K (T + d) words and lgc_party_input_bits is K (T + d) x width.
 * Phase 1 runs once per fold (linreg_gc_folds.h: lgc_p1_local_folds, lgc_p1_set_rows); bin/linreg --lambdas=.. --folds=K
 * drives it through the five-process protocol.
 *
 * Revealed.  lgc_solver_get_beta and the beta of lgc_party_finish hold, in this order,
 *   beta*                          d words
 *   l*                             1 word, with LGC_SELECT_REVEAL_INDEX
 *   cv_0 .. cv_{L-1}               L words, with LGC_SELECT_REVEAL_SCORES: the sums only, never a per-fold score
 * Everything else stays garbled words: the K L fold models, the L - 1 losing refits, every per-fold score.
 * LGC_SELECT_REVEAL_SCORES is a debugging aid, as for the lasso.
 *
 * One value (count = 1) needs neither scores nor a selection: beta* = beta_{K,0}, l* = 0, the K fold fits are not lowered
 * at all and a revealed cv_0 is the constant 0.
 *
 * The lambda-free part (fold sums, divisions by d, tot, differences, constant divisions) is garbled once; the (K + 1) L
 * fits run as merged circuits, as the blocks of a sweep do, and the scoring and selection read across them.
 * lgc_solver_num_folds / lgc_party_num_folds (linreg_gc_lasso_cv.h), lgc_solver_selected_index / lgc_party_selected_index
 * (linreg_gc_lasso_select.h), lgc_solver_num_circuits / lgc_party_num_circuits (linreg_gc_sweep.h; they return L),
 * lgc_solver_get_iterations and the table ring modes work on the objects created here; lgc_party_program_fingerprint covers
 * K, the L values, the reveal flags and the algorithm.
 * Rejected with LGC_EINVAL: algorithm LGC_ALG_LASSO (use linreg_gc_lasso_cv.h); a system with trace or reveal_inputs set;
 * folds outside 2..LGC_MAX_FOLDS; count outside 1..LGC_MAX_RIDGE_CV_VALUES; a lambda that is not finite or is negative;
 * reveal bits other than the two above; a program whose word ids, circuit count or per-circuit gate steps do not fit.
 */
#ifndef LINREG_GC_RIDGE_CV_H
#define LINREG_GC_RIDGE_CV_H
#include "linreg_gc_lasso_cv.h"
#include "linreg_gc_sweep.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LGC_MAX_RIDGE_CV_VALUES 256

int lgc_program_build_ridge_cv(struct lgc_program **out, const lgc_system *sys, size_t count, const double *lambdas, size_t folds, int reveal);
int lgc_solver_create_ridge_cv(lgc_solver **out, int device, const lgc_system *sys, const uint8_t seed[16], size_t count,
                               const double *lambdas, size_t folds, int reveal);
int lgc_party_create_ridge_cv(lgc_party **out, int device, const lgc_system *sys, int role, const uint8_t seed[16],
                              size_t max_launch_table_bytes, size_t count, const double *lambdas, size_t folds, int reveal);

#ifdef __cplusplus
}
#endif
#endif
