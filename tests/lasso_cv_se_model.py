"""An independent model of the one-standard-error rule for the lasso path's in-circuit K-fold cross-validation
(include/linreg_gc_lasso_cv_se.h) in Python integers.

It restates the definition on top of the cross-validation's model (tests/lasso_cv_model.py) and shares no code with the
product.  Every share is [A_0][b_0] ... [A_{K-1}][b_{K-1}] [yy_0 .. yy_{K-1}].  All mod 2^w, compares signed:
  Y_k      the share sum of yy_k; on the data-provider path divided by d (truncating)
  e_{k,l}  score_{k,l} + Y_k;  S_l = sum_k e_{k,l};  mean_l = tdiv(S_l, K)
  q_l      sum_k mul(e_{k,l} - mean_l, e_{k,l} - mean_l);  se_l = sqrt(tdiv(q_l, K (K - 1)))
  thr      mean_{l*} + se_{l*}, l* the first signed minimum of cv_l = sum_k score_{k,l}
  pi       the values by decreasing penalty: their quantised words compared unsigned, ties to the smaller l
  l+       the first l in pi-order with mean_l <= thr;  beta+ = beta_{K,l+}
One value: beta+ = beta_{K,0}, l+ = l* = 0, nothing scored (revealed cv and curve words are 0).
"""
import math

import lasso_cv_model as lcm
import lasso_model as lm
import lasso_select_model as lsm

ABSOLUTE, RATIO = lcm.ABSOLUTE, lcm.RATIO
REVEAL_INDEX, REVEAL_SCORES, REVEAL_CURVE = lcm.REVEAL_INDEX, lcm.REVEAL_SCORES, 4
RULE_MIN, RULE_ONE_SE = 0, 1


def sqrt(a, w, p):
    """OP_SQRT on the signed word a: the root of a 2^p (the word read as unsigned), as the reference's fixed-point sqrt forms
    it at either width"""
    if w == 64:
        return lm.wrap(math.isqrt((a & ((1 << 64) - 1)) << p), 64)
    mask = (1 << (32 + p)) - 1
    x = ((a & 0xFFFFFFFFFFFFFFFF) << p) & mask
    r, e = 0, mask + 1
    while e:
        if (x & mask) >= ((r + e) & mask):
            x = (x - (r + e)) & 0xFFFFFFFFFFFFFFFF
            r = ((r >> 1) + e) & mask
        else:
            r >>= 1
        e >>= 2
    return lm.wrap(r, 32)


def order(values, w, p):
    """pi: the indices by decreasing quantised value (unsigned), ties to the smaller index"""
    q = [lm.to_fixed(v, p, w) & ((1 << w) - 1) for v in values]
    return sorted(range(len(values)), key=lambda l: (-q[l], l))


def fold_sums(yy_shares, d, w, normalize):
    """Y_k from yy_shares: one row of K words per share"""
    K = len(yy_shares[0])
    Y = [lm.wrap(sum(int(sh[k]) for sh in yy_shares), w) for k in range(K)]
    return [lsm.tdiv(y, d) for y in Y] if normalize else Y


def curve(errors, w, p):
    """(mean, se) of errors[k][l]"""
    K, L = len(errors), len(errors[0])
    mean = [lsm.tdiv(lm.wrap(sum(errors[k][l] for k in range(K)), w), K) for l in range(L)]
    se = []
    for l in range(L):
        dev = [lm.wrap(errors[k][l] - mean[l], w) for k in range(K)]
        q = lm.wrap(sum(lm.mul(v, v, w, p) for v in dev), w)
        se.append(sqrt(lsm.tdiv(q, K * (K - 1)), w, p))
    return mean, se


def lasso_cv_se(fold_shares, yy_shares, d, w, p, iters, values, mode, normalize, lam, rule=RULE_ONE_SE, factors=None, lower=None,
                upper=None):
    """dict(beta, index (l+), min (l*), cv, mean, se, errors (e[k][l]), order)"""
    L = len(values)
    _, lmin, cv, fits = lcm.lasso_cv(fold_shares, d, w, p, iters, values, mode, normalize, lam, factors, lower, upper)
    K = len(fold_shares)
    pi = order(values, w, p)
    if L == 1:
        return dict(beta=fits[K][0], index=0, min=0, cv=[0], mean=[0], se=[0], errors=None, order=pi)
    folds = lcm.fold_systems(fold_shares, d, w, normalize)
    Y = fold_sums(yy_shares, d, w, normalize)
    errors = [[lm.wrap(lsm.score(folds[k][0], folds[k][1], fits[k][l], d, w, p) + Y[k], w) for l in range(L)] for k in range(K)]
    mean, se = curve(errors, w, p)
    thr = lm.wrap(mean[lmin] + se[lmin], w)
    pick = next(l for l in pi if mean[l] <= thr) if rule == RULE_ONE_SE else lmin
    return dict(beta=fits[K][pick], index=pick, min=lmin, cv=cv, mean=mean, se=se, errors=errors, order=pi)


def revealed(m, flags, rule=RULE_ONE_SE):
    """the words revealed, in order: beta+, [l+, l*] (RULE_MIN: [l*]), [cv], [mean, se]"""
    out = list(m["beta"])
    if flags & REVEAL_INDEX:
        out += [m["index"], m["min"]] if rule == RULE_ONE_SE else [m["min"]]
    if flags & REVEAL_SCORES:
        out += list(m["cv"])
    if flags & REVEAL_CURVE:
        out += list(m["mean"]) + list(m["se"])
    return out
