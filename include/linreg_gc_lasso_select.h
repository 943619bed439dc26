/*
 * linreg_gc_lasso_select.h -- a lasso path whose model is chosen inside the circuit on a hold-out (liblinreg_gc.so).
 *
 * A lasso path (linreg_gc_lasso_path.h, with the options of linreg_gc_lasso_opts.h) fits L models beta_0 .. beta_{L-1} and
 * reveals all of them.  The calls here take a second, VALIDATION system (A_v, b_v) beside the training system, score every
 * model on it inside the circuit, and reveal only the best one (what cv.glmnet's lambda.min or sklearn's LassoCV return):
 *   M_v, b_v   assembled from the shares exactly as M and b are, without lambda2: share sums; with normalize = 1 the
 *              off-diagonal entries and b_v are then divided by the public normaliser d, the diagonal is left as summed
 *   score_l    t_i = sum_j mul(M_v,ij, beta_l,j);  r_i = 2 b_v,i - t_i;  score_l = 0 - sum_i mul(beta_l,i, r_i)   (mod 2^width)
 *              = beta_l^T M_v beta_l - 2 b_v^T beta_l up to the truncation of every mul: the hold-out squared error of
 *              beta_l minus a constant that does not depend on l
 *   l*         the smallest l whose score is minimal under a SIGNED compare at both widths: ties go to the value listed first
 *   beta*      beta_{l*}
 * Range condition, beside those of the path: 2 b_v, every t_i and every score fit in width - 1 - precision integer bits.
 *
 * Sizes.  Every share is [A (T)] [b (d)] [A_v (T)] [b_v (d)], T = d (d + 1) / 2: lgc_solver_set_shares takes
 * nshares x 2 (T + d) words, lgc_party_input_bits is 2 (T + d) x width, the input calls of a party take 2 (T + d) values per
 * share, and reveal_inputs (lgc_solver_get_inputs, lgc_party_finish) gives 2 (T + d) words in that layout.  Phase 1 needs no
 * change: a caller runs the lgc_p1_* calls once on the training rows and once on the validation rows (each divided by its
 * own row count, as the aggregation does) and places the two results side by side in its share.
 *
 * Revealed.  lgc_solver_get_beta and the beta of lgc_party_finish hold, in this order,
 *   beta*                          d words
 *   l*                             1 word, with LGC_SELECT_REVEAL_INDEX
 *   score_0 .. score_{L-1}         L words, with LGC_SELECT_REVEAL_SCORES
 * so d, d + 1, d + L or d + 1 + L words.  The L - 1 losing models, lambda_max, the step exponent, every theta and -- without
 * LGC_SELECT_REVEAL_SCORES -- the scores stay garbled words.  LGC_SELECT_REVEAL_INDEX tells which of the public lambda1
 * values won.  LGC_SELECT_REVEAL_SCORES is a debugging aid like `trace`: L scores are L quadratic forms of the validation
 * system in the hidden models -- they leak about the models that were NOT selected and about (M_v, b_v); do not set it in
 * production.
 *
 * One value (l1_count = 1) needs no selection: beta* = beta_0, l* = 0.  Every other linreg_gc.h call works on the objects
 * created here as on a lasso path's (lgc_solver_path_length is still L; the iteration marks are the path's);
 * lgc_party_program_fingerprint covers the validation system and the reveal flags.  Both roles on one GPU or apart; the
 * table ring modes need nothing new.
 * Rejected with LGC_EINVAL: a null opts; everything lgc_program_build_lasso_opts rejects (hence everything a lasso path
 * rejects); reveal bits other than the two below; a system with trace set (it would reveal every iterate of every model).
 */
#ifndef LINREG_GC_LASSO_SELECT_H
#define LINREG_GC_LASSO_SELECT_H
#include "linreg_gc_lasso_opts.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LGC_SELECT_REVEAL_INDEX 1  /* reveal l*, the index of the selected value */
#define LGC_SELECT_REVEAL_SCORES 2 /* reveal the L scores as well (debugging: see above for what they leak) */

int lgc_program_build_lasso_select(struct lgc_program **out, const lgc_system *sys, const lgc_lasso_opts *opts, int reveal);
int lgc_solver_create_lasso_select(lgc_solver **out, int device, const lgc_system *sys, const uint8_t seed[16],
                                   const lgc_lasso_opts *opts, int reveal);
int lgc_party_create_lasso_select(lgc_party **out, int device, const lgc_system *sys, int role, const uint8_t seed[16],
                                  size_t max_launch_table_bytes, const lgc_lasso_opts *opts, int reveal);

/* l* of a solver that has run, or -1 when the index was not revealed (no LGC_SELECT_REVEAL_INDEX, not a selection, not run) */
int64_t lgc_solver_selected_index(const lgc_solver *s);
/* l* on the evaluator as lgc_party_finish decoded it; -1 before lgc_party_finish has succeeded, when the index was not
 * revealed, or when p is not the evaluator of a selection */
int64_t lgc_party_selected_index(const lgc_party *p);

#ifdef __cplusplus
}
#endif
#endif
