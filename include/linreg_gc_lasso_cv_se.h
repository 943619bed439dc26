/*
 * linreg_gc_lasso_cv_se.h -- the one-standard-error rule for the in-circuit K-fold cross-validation of a lasso path, and
 * the curve (cvm, cvsd) behind it (liblinreg_gc.so).
 *
 * linreg_gc_lasso_cv.h reveals the refit at the arg-min of K summed scores.  cv.glmnet users mostly take lambda.1se
 * instead: the most regularised model whose cross-validated error is within one standard error of the minimum.  The scores
 * drop the constant y_k^T y_k, which differs between folds, so the spread of the per-fold errors needs one more input word
 * per fold.  The calls here take it and apply the rule inside the circuit; nobody could apply it afterwards, because the
 * losing models and the per-fold scores are never revealed.
 *
 * Everything of linreg_gc_lasso_cv.h stands: the folds F_k, the K + 1 training systems, lambda2, the (K + 1) L fits,
 * score_k,l, cv_l and l* = the first signed minimum of cv.  All arithmetic mod 2^width; mul, tdiv by a public constant and
 * sqrt are the circuit's (OP_MUL, OP_IDIVC, OP_SQRT); compares are signed at both widths.
 *
 * Sizes.  Every share is [A_0 (T)] [b_0 (d)] ... [A_{K-1} (T)] [b_{K-1} (d)] [yy_0 .. yy_{K-1}]: K (T + d) + K words.  The
 * fold stride T + d is unchanged, the K new words sit at the end.  yy_k is an additive share of sum_{rows q of fold k}
 * y_q y_q mod 2^64, masked to the width, y quantised with the fold's normaliser exactly as for b_k: the integer Gram entry,
 * NOT the floating-point diagonal rule.  Only the provider that holds y contributes a non-zero word;
 * lgc_p1_local_folds_yy (linreg_gc_folds_yy.h) returns it from the pass that forms A_k and b_k.  lgc_solver_set_shares,
 * lgc_party_input_bits, the input calls of a party and reveal_inputs all use K (T + d) + K (a revealed Y_k is 0 where the
 * program does not form it).
 *
 *   Y_k        the share sum of yy_k; with normalize = 1 divided by d (truncating), as b_k is
 *   e_k,l      score_k,l + Y_k: fold k's squared error at value l in the units of the scores
 *   S_l        sum_k e_k,l;   mean_l = tdiv(S_l, K)                                        (cv.glmnet's cvm)
 *   q_l        sum_k mul(e_k,l - mean_l, e_k,l - mean_l);   se_l = sqrt(tdiv(q_l, K (K - 1)))   (cvsd, equal fold weights)
 *   thr        mean_{l*} + se_{l*}
 *   pi         the public order of the L values by decreasing penalty: the quantised lambda1_l (LGC_L1_ABSOLUTE) or r_l
 *              (LGC_L1_RATIO) compared as unsigned words, ties to the smaller l
 *   l+         the first index in pi-order with mean_l <= thr (signed); l* always qualifies
 *   beta+      beta_{K,l+}, the full-data refit
 * LGC_CV_RULE_ONE_SE reveals beta+; LGC_CV_RULE_MIN reveals beta* = beta_{K,l*} by a program that equals
 * lgc_program_build_lasso_cv's except for the extra input words (and the curve, where asked for).
 * Range condition: that of linreg_gc_lasso_cv.h; in addition every Y_k, e_k,l, S_l (K errors summed), q_l and thr fits in
 * width - 1 - precision integer bits.
 *
 * Revealed.  lgc_solver_get_beta and the beta of lgc_party_finish hold, in this order,
 *   beta+ (beta* with LGC_CV_RULE_MIN)      d words
 *   l+, then l*                             2 words, with LGC_SELECT_REVEAL_INDEX (LGC_CV_RULE_MIN: l* alone, 1 word)
 *   cv_0 .. cv_{L-1}                        L words, with LGC_SELECT_REVEAL_SCORES (a debugging aid, as ever)
 *   mean_0 .. mean_{L-1}, se_0 .. se_{L-1}  2 L words, with LGC_SELECT_REVEAL_CURVE
 * LGC_SELECT_REVEAL_CURVE is a user's choice, not a debugging aid: it is what cv.glmnet returns as cvm and cvsd.  It leaks
 * L means and L spreads of quadratic forms in the hidden models (and, through mean_l - cv_l / K, the mean of y^T y over the
 * folds).  A per-fold error is never revealed.  Everything else stays garbled: the K L fold models, the L - 1 other refits,
 * every Y_k, thr, which values qualified.
 * lgc_solver_selected_index / lgc_party_selected_index (linreg_gc_lasso_select.h) give l+ (the index of the revealed
 * model), lgc_solver_min_index / lgc_party_min_index l*; both -1 without LGC_SELECT_REVEAL_INDEX, before a run / finish,
 * and on NULL.  On an object of another selection call lgc_*_min_index equals lgc_*_selected_index.
 *
 * One value (l1_count = 1): as in linreg_gc_lasso_cv.h nothing is scored; beta+ = beta_{K,0}, l+ = l* = 0, and revealed
 * curve words are the constant 0.  lgc_party_program_fingerprint covers the rule, the reveal flags and pi.
 * Rejected with LGC_EINVAL: a rule other than the two below; reveal bits other than the three; everything
 * lgc_program_build_lasso_cv rejects (the word-count check counts the K extra words).
 */
#ifndef LINREG_GC_LASSO_CV_SE_H
#define LINREG_GC_LASSO_CV_SE_H
#include "linreg_gc_lasso_cv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LGC_SELECT_REVEAL_CURVE 4 /* beside LGC_SELECT_REVEAL_INDEX (1) and LGC_SELECT_REVEAL_SCORES (2) */

enum lgc_cv_rule { LGC_CV_RULE_MIN = 0, LGC_CV_RULE_ONE_SE = 1 };

int lgc_program_build_lasso_cv_se(struct lgc_program **out, const lgc_system *sys, const lgc_lasso_opts *opts, size_t folds, int reveal,
                                  int rule);
int lgc_solver_create_lasso_cv_se(lgc_solver **out, int device, const lgc_system *sys, const uint8_t seed[16],
                                  const lgc_lasso_opts *opts, size_t folds, int reveal, int rule);
int lgc_party_create_lasso_cv_se(lgc_party **out, int device, const lgc_system *sys, int role, const uint8_t seed[16],
                                 size_t max_launch_table_bytes, const lgc_lasso_opts *opts, size_t folds, int reveal, int rule);

int64_t lgc_solver_min_index(const lgc_solver *s);
int64_t lgc_party_min_index(const lgc_party *p);

#ifdef __cplusplus
}
#endif
#endif
