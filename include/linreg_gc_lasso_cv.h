/*
 * linreg_gc_lasso_cv.h -- a lasso path cross-validated over K folds inside the circuit; only the refit is revealed
 * (liblinreg_gc.so).
 *
 * The selection of linreg_gc_lasso_select.h scores a path on ONE hold-out: its rows are lost to the fit, the winner depends
 * on which rows were held out, and the revealed model was fitted on the training part only.  The calls here do what
 * cv.glmnet and sklearn's LassoCV do: K train / validation pairs, the K scores of every lambda1 summed before the arg-min,
 * and one model, refitted on ALL rows at the winning lambda1.  Public K, 2 <= K <= LGC_MAX_FOLDS.  All arithmetic mod 2^width.
 *   F_k        fold k, assembled from the shares exactly as the selection's validation system is: share sums; with
 *              normalize = 1 the off-diagonal entries and b are then divided by the public normaliser d, the diagonal is
 *              left as summed; no lambda2
 *   tot        sum_k F_k, entry by entry
 *   validation system of fold k    (M_v,k, b_v,k) = F_k
 *   training system of fold k      entry = tdiv(tot - F_k, K - 1) (truncating; K = 2: no division), then lambda2 on the diagonal
 *   full system (index K)          entry = tdiv(tot, K), then lambda2 on the diagonal
 *   lambda2    lgc_system.lambda, quantised as ever, is added to the K + 1 training diagonals on BOTH input paths.  This
 *              is the one departure from "normalize = 0 adds nothing": the folds double as validation systems and must
 *              stay free of lambda2, so it cannot be part of the inputs.  Fold inputs never contain lambda2.
 *   fits       (K + 1) L recurrences, each bit for bit the lasso path's (penalty factors and bounds included) on its own
 *              system with its own step exponent; the momentum constants are shared.  LGC_L1_ABSOLUTE: the same lambda1
 *              values for every system.  LGC_L1_RATIO: lambda_max = max_i |b_i| of the FULL system, for all K + 1 systems
 *              (cv.glmnet likewise fixes its sequence on all rows): index l means the same penalty in every fold.
 *   score_k,l  the selection's score of beta_{k,l} on (M_v,k, b_v,k);  cv_l = sum_k score_k,l
 *   l*         the smallest l whose cv_l is minimal under a SIGNED compare;  beta* = beta_{K,l*}, the full-data refit
 * Folds weigh equally whatever their row counts: a caller should make them equal in size to within one row.
 * Range condition: the selection's, for every fold; in addition tot, every 2 b_v,k and every cv_l fit in
 * width - 1 - precision integer bits.
 *
 * Sizes.  Every share is [A_0 (T)] [b_0 (d)] ... [A_{K-1} (T)] [b_{K-1} (d)], T = d (d + 1) / 2: lgc_solver_set_shares takes
 * nshares x K (T + d) words, lgc_party_input_bits is K (T + d) x width, the input calls of a party take K (T + d) values per
 * share, and reveal_inputs (lgc_solver_get_inputs, lgc_party_finish) gives K (T + d) words in that layout: the folds F_k.
 * Phase 1 needs no change: a caller runs the lgc_p1_* calls once per fold, on that fold's rows alone and divided by its own
 * row count, and places the K results side by side in its share.  linreg_gc_folds.h has the fold rule, the row window that
 * makes the lgc_p1_* calls act on one fold of an uploaded object, and all K local blocks in one pass; bin/linreg --folds=K
 * drives them through the five-process protocol.
 *
 * Revealed.  lgc_solver_get_beta and the beta of lgc_party_finish hold, in this order,
 *   beta*                          d words
 *   l*                             1 word, with LGC_SELECT_REVEAL_INDEX
 *   cv_0 .. cv_{L-1}               L words, with LGC_SELECT_REVEAL_SCORES: the sums only, never a per-fold score
 * Everything else stays garbled words: the K L fold models, the L - 1 losing refits, every step exponent, lambda_max, every
 * theta.  LGC_SELECT_REVEAL_SCORES is a debugging aid, as for the selection.
 *
 * One value (l1_count = 1) needs neither scores nor a selection: beta* = beta_{K,0}, l* = 0, the K fold fits are not lowered
 * at all and a revealed cv_0 is the constant 0.  lgc_solver_selected_index and lgc_party_selected_index
 * (linreg_gc_lasso_select.h) work on the objects created here; lgc_party_program_fingerprint covers K and the reveal flags.
 * Both roles on one GPU or apart; the table ring modes need nothing new.
 * Rejected with LGC_EINVAL: folds outside 2..LGC_MAX_FOLDS; a system with trace set; reveal bits other than the two of
 * linreg_gc_lasso_select.h; a null opts and everything lgc_program_build_lasso_opts rejects; a program whose word ids or
 * whose OP_PROX pair offset (K + 1) L d would not fit their fields.
 */
#ifndef LINREG_GC_LASSO_CV_H
#define LINREG_GC_LASSO_CV_H
#include "linreg_gc_lasso_select.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LGC_MAX_FOLDS 16

int lgc_program_build_lasso_cv(struct lgc_program **out, const lgc_system *sys, const lgc_lasso_opts *opts, size_t folds, int reveal);
int lgc_solver_create_lasso_cv(lgc_solver **out, int device, const lgc_system *sys, const uint8_t seed[16],
                               const lgc_lasso_opts *opts, size_t folds, int reveal);
int lgc_party_create_lasso_cv(lgc_party **out, int device, const lgc_system *sys, int role, const uint8_t seed[16],
                              size_t max_launch_table_bytes, const lgc_lasso_opts *opts, size_t folds, int reveal);

/* K of an object created here; 0 on every other object (and on NULL) */
size_t lgc_solver_num_folds(const lgc_solver *s);
size_t lgc_party_num_folds(const lgc_party *p);

#ifdef __cplusplus
}
#endif
#endif
