"""An independent model of the lasso path's in-circuit K-fold cross-validation (include/linreg_gc_lasso_cv.h)
in Python integers.

It restates the definition on top of the selection's model (tests/lasso_select_model.py) and the path models
(tests/lasso_bounds_model.py) and shares no code with the product.  All mod 2^w:
  F_k      fold k as the selection's validation system: share sums; on the data-provider path the off-diagonals and b
           divided by d (truncating), the diagonal as summed; no lambda2
  tot      sum_k F_k;  training system k = tdiv(tot - F_k, K - 1) (K = 2: as it is), full system = tdiv(tot, K), each with
           q(lambda2) added on the diagonal -- on both input paths
  fits     the path's recurrences on each of the K + 1 systems with its own step exponent; in ratio mode lambda_max is the
           FULL system's max_i |b_i| for all of them
  cv_l     sum_k score(beta_{k,l}; F_k);  l* the first signed minimum;  beta* = beta_{K,l*}
One value: beta* = beta_{K,0}, l* = 0, no scores (a revealed cv_0 is 0).
"""
import lasso_bounds_model as lbm
import lasso_model as lm
import lasso_path_model as lpm
import lasso_select_model as lsm

ABSOLUTE, RATIO = lbm.ABSOLUTE, lbm.RATIO
REVEAL_INDEX, REVEAL_SCORES = lsm.REVEAL_INDEX, lsm.REVEAL_SCORES


def fold_systems(fold_shares, d, w, normalize):
    """[(M_v,k, b_v,k)] from fold_shares[k]: the rows (one per share) of T + d words of fold k"""
    return [lsm.validation_system(sh, d, w, normalize) for sh in fold_shares]


def packed(M, d):
    return [M[i][j] for i in range(d) for j in range(i + 1)]


def training_systems(folds, d, w, lam_fixed):
    """[(a_packed, b)] of the K + 1 training systems, the full system last, from the folds [(M, b)]"""
    K = len(folds)
    T = d * (d + 1) // 2
    F = [packed(M, d) + list(b) for M, b in folds]
    tot = [lm.wrap(sum(f[e] for f in F), w) for e in range(T + d)]
    diag = {i * (i + 1) // 2 + i for i in range(d)}

    def finish(v):
        return [lm.wrap(x + lam_fixed, w) if e in diag else x for e, x in enumerate(v[:T])], v[T:]
    out = []
    for k in range(K):
        diff = [lm.wrap(tot[e] - F[k][e], w) for e in range(T + d)]
        out.append(finish(diff if K == 2 else [lsm.tdiv(x, K - 1) for x in diff]))
    out.append(finish([lsm.tdiv(x, K) for x in tot]))
    return out


def fit(a_packed, b, lmax, d, w, p, iters, values, mode, factors, lower, upper):
    """the path's models on one system; ratio mode: with the given lambda_max instead of the system's own"""
    M = lm.full_matrix(a_packed, d, w)
    b = [lm.wrap(int(v), w) for v in b]
    ell = lm.step_exponent(M, d, w)
    lo, hi, _ = lbm.bound_words(lower, upper, d, w, p)
    factors = [1.0] * d if factors is None else list(factors)
    betas = []
    for v in values:
        theta = []
        for f in factors:
            q = lm.to_fixed(v * f, p, w)
            assert q >= 0
            theta.append(lm.step(q if mode == ABSOLUTE else lm.mul(lmax, q, w, p), ell, w, p))
        betas.append(lbm.fista(M, b, d, w, p, iters, ell, theta, lo, hi))
    return betas


def lasso_cv(fold_shares, d, w, p, iters, values, mode, normalize, lam, factors=None, lower=None, upper=None):
    """(beta*, l*, cv, fits): fits[s][l] the model of system s (s = K: the full system; one value: only that one is fitted)"""
    folds = fold_systems(fold_shares, d, w, normalize)
    K = len(folds)
    systems = training_systems(folds, d, w, lm.to_fixed(lam, p, w))
    lmax = lpm.lambda_max([lm.wrap(int(v), w) for v in systems[K][1]], w) if mode == RATIO else None
    which = range(K + 1) if len(values) > 1 else [K]
    fits = {s: fit(systems[s][0], systems[s][1], lmax, d, w, p, iters, values, mode, factors, lower, upper) for s in which}
    if len(values) == 1:
        return fits[K][0], 0, [0], fits
    cv = [lm.wrap(sum(lsm.score(folds[k][0], folds[k][1], fits[k][l], d, w, p) for k in range(K)), w) for l in range(len(values))]
    best = lsm.argmin_first(cv)
    return fits[K][best], best, cv, fits


revealed = lsm.revealed
