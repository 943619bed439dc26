"""An independent model of the ridge sweep's in-circuit K-fold cross-validation (include/linreg_gc_ridge_cv.h)
in Python integers.

It restates the definition on top of the lasso cross-validation's fold assembly (tests/lasso_cv_model.py) and the selection's
score (tests/lasso_select_model.py); the per-fit solve is the semantic oracle's (oracle/liblinreg_oracle.so: orc_cgd,
orc_cholesky, orc_ldlt on the packed system), the one the solver tests compare the single-solve programs against.  All mod 2^w:
  F_k      fold k: share sums; on the data-provider path the off-diagonals and b divided by d (truncating); no lambda
  tot      sum_k F_k;  training system k = tdiv(tot - F_k, K - 1) (K = 2: as it is), full system = tdiv(tot, K)
  fits     beta_{s,l} = solve(system s with q(lambda_l) added on the diagonal, b_s) for s = 0 .. K, l = 0 .. L - 1
  cv_l     sum_k score(beta_{k,l}; F_k);  l* the first signed minimum;  beta* = beta_{K,l*}
One value: beta* = beta_{K,0}, l* = 0, no scores (a revealed cv_0 is 0), the fold fits are not formed.
"""
import numpy as np

import lasso_cv_model as lcm
import lasso_model as lm
import lasso_select_model as lsm

REVEAL_INDEX, REVEAL_SCORES = lsm.REVEAL_INDEX, lsm.REVEAL_SCORES


def systems(fold_shares, d, w, normalize):
    """(folds [(M, b)], the K + 1 lambda-free training systems [(a_packed, b)], the full system last)"""
    folds = lcm.fold_systems(fold_shares, d, w, normalize)
    return folds, lcm.training_systems(folds, d, w, 0)


def with_lambda(a_packed, d, w, lam_fixed):
    """the packed triangle with lam_fixed added on the diagonal"""
    diag = {i * (i + 1) // 2 + i for i in range(d)}
    return [lm.wrap(int(x) + lam_fixed, w) if e in diag else int(x) for e, x in enumerate(a_packed)]


def solve(oracle, alg, a_packed, b, d, w, p, iters):
    """beta of the single solve on the packed system as given (nothing added, nothing divided)"""
    a = np.array(a_packed, dtype=np.int64)
    bb = np.array([int(v) for v in b], dtype=np.int64)
    if alg == "cgd":
        return [int(v) for v in oracle.cgd(a, bb, d, p, w, iters)]
    if alg == "cholesky":
        return [int(v) for v in oracle.cholesky(a, bb, d, p, w)]
    return [int(v) for v in oracle.ldlt(a, bb, d, p, w)]


def ridge_cv(oracle, fold_shares, d, w, p, alg, iters, lambdas, normalize):
    """(beta*, l*, cv, fits, per-fold scores): fits[s][l] the model of system s at lambda_l (s = K: the full system; one value:
    only that one is fitted), scores[k][l]"""
    folds, train = systems(fold_shares, d, w, normalize)
    K, L = len(folds), len(lambdas)
    q = [lm.to_fixed(v, p, w) for v in lambdas]
    which = range(K + 1) if L > 1 else [K]
    fits = {s: [solve(oracle, alg, with_lambda(train[s][0], d, w, ql), train[s][1], d, w, p, iters) for ql in q] for s in which}
    if L == 1:
        return fits[K][0], 0, [0], fits, None
    scores = [[lsm.score(folds[k][0], folds[k][1], fits[k][l], d, w, p) for l in range(L)] for k in range(K)]
    cv = [lm.wrap(sum(scores[k][l] for k in range(K)), w) for l in range(L)]
    best = lsm.argmin_first(cv)
    return fits[K][best], best, cv, fits, scores


revealed = lsm.revealed
