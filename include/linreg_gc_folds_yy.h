/*
 * linreg_gc_folds_yy.h -- phase 1 on row folds with the folds' y^T y: what the provider that holds y adds to its share for
 * the one-standard-error rule of linreg_gc_lasso_cv_se.h (liblinreg_gc.so).
 *
 * lgc_p1_local_folds_yy(h, c0, c1, K, out_A, out_b, out_yy) is lgc_p1_local_folds(h, c0, c1, 1, K, out_A, out_b)
 * (linreg_gc_folds.h) -- the same single launch of the same kernel, no second pass over X, out_A and out_b word for word --
 * and additionally returns out_yy[k] = sum over the rows q of fold k of y_q y_q mod 2^64, masked to the width: the entry
 * (own, own) of fold k's Gram block over the own columns and y, which the kernel has always formed and the older call
 * drops.  It is the integer Gram entry, the arithmetic of the entries of b_k, not the floating-point diagonal rule.
 * LGC_EINVAL: what lgc_p1_local_folds rejects; an object without y; a null out_b or out_yy.
 */
#ifndef LINREG_GC_FOLDS_YY_H
#define LINREG_GC_FOLDS_YY_H
#include "linreg_gc_folds.h"

#ifdef __cplusplus
extern "C" {
#endif

int lgc_p1_local_folds_yy(lgc_p1 *h, size_t c0, size_t c1, size_t folds, uint64_t *out_A, uint64_t *out_b, uint64_t *out_yy);

#ifdef __cplusplus
}
#endif
#endif
