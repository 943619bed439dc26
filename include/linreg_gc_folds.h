/*
 * linreg_gc_folds.h -- phase 1 on row folds: what a data provider needs to feed the K-fold cross-validation of
 * linreg_gc_lasso_cv.h from inside the five-process protocol (liblinreg_gc.so).
 *
 * The fold systems X_k^T X_k and X_k^T y_k exist only as sums of phase-1 shares: the columns are spread over the data
 * providers, so no party can cut a finished share into folds.  Every provider instead runs phase 1 once per fold on that
 * fold's rows, and the K results go side by side into its share ([A_0][b_0] ... [A_{K-1}][b_{K-1}]).
 *
 * Folds.  Public, contiguous row blocks: fold k of K over n rows is rows [floor(k n / K), floor((k + 1) n / K)); the folds
 * partition [0, n) and their sizes differ by at most one.  lgc_fold_rows is the ONE statement of that rule (bin/linreg and
 * python/linreg_gc.py both call it).  LGC_EINVAL: K outside 2..LGC_MAX_FOLDS, K > n, k >= K, a null pointer.  No GPU needed.
 *
 * Row window.  lgc_p1_set_rows(h, r0, r1): from now on every call on h -- lgc_p1_local, lgc_p1_local_targets, lgc_p1_mask,
 * lgc_p1_dot, lgc_p1_ti_a, lgc_p1_ti_a_batch, with host or device I/O -- acts on rows [r0, r1) of the data the object was
 * given, exactly as an object created from those rows alone would: vector arguments and results have r1 - r0 entries and
 * the split-K chunking follows r1 - r0.  (The divisor of the floating-point diagonal is the column count d, src/phase1.c:566,
 * which a window leaves alone; the row count enters through the quantisation of the data, which is the caller's.)
 * lgc_p1_set_rows(h, 0, n) restores the whole object; a fresh object has that window.  lgc_p1_set_data / _set_targets always
 * write all n rows.  Not to be called while another thread is inside a call on h.  LGC_EINVAL: r0 >= r1, r1 > n.
 *
 * All folds in one pass.  lgc_p1_local_folds(h, c0, c1, with_y, K, out_A, out_b) computes what K lgc_p1_local calls behind
 * lgc_p1_set_rows(fold k) would, from one read of X: out_A holds K blocks of own (own + 1) / 2 words in lgc_p1_local's layout
 * (own = c1 - c0), out_b K blocks of own words (with_y; else it may be NULL).  The folds are those of the object's current
 * window.  Every word is bit-identical to the windowed call's: the off-diagonal sums are exact integer arithmetic, and the
 * floating-point diagonal of fold k is summed over that fold's rows, k ascending.
 */
#ifndef LINREG_GC_FOLDS_H
#define LINREG_GC_FOLDS_H
#include "linreg_gc_lasso_cv.h"

#ifdef __cplusplus
extern "C" {
#endif

int lgc_fold_rows(size_t n, size_t folds, size_t k, size_t *r0, size_t *r1);
int lgc_p1_set_rows(lgc_p1 *h, size_t r0, size_t r1);
int lgc_p1_local_folds(lgc_p1 *h, size_t c0, size_t c1, int with_y, size_t folds, uint64_t *out_A, uint64_t *out_b);

#ifdef __cplusplus
}
#endif
#endif
