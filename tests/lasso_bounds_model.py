"""An independent model of the lasso's penalty factors and bounds (include/linreg_gc_lasso_opts.h) in Python
integers.

It restates the definition on top of the single-solve model (tests/lasso_model.py) and shares no code with the product.  Per
value l and coordinate i:
  absolute  theta_{l,i} = step(q(lambda1_l * w_i))                   (the product in IEEE double, then quantised)
  ratio     theta_{l,i} = step(mul(lambda_max, q(r_l * w_i)))
  x_i' = clamp(soft(z_i; theta_{l,i}), lo_i, hi_i), signed compares; an infinite side of a bound is the extreme word.
`prox_record` is the flagged OP_PROX record (bit 31 of cnt) on a word file, next to word_model's unflagged one.
"""
import math

import numpy as np

import lasso_model as lm
import lasso_path_model as lpm
import word_model as wm

ABSOLUTE, RATIO = lpm.ABSOLUTE, lpm.RATIO
BOUNDED = 1 << 31


def clamp(v, lo, hi):
    assert lo <= hi
    return lo if v < lo else hi if v > hi else v


def bound_words(lower, upper, d, w, p):
    """([lo_i], [hi_i], [boxed_i]) as signed words: q(v) for a finite bound, -2^(w-1) / 2^(w-1) - 1 for a missing side"""
    lower = [-math.inf] * d if lower is None else list(lower)
    upper = [math.inf] * d if upper is None else list(upper)
    lo = [lm.to_fixed(v, p, w) if math.isfinite(v) else -(1 << (w - 1)) for v in lower]
    hi = [lm.to_fixed(v, p, w) if math.isfinite(v) else (1 << (w - 1)) - 1 for v in upper]
    boxed = [math.isfinite(a) or math.isfinite(b) for a, b in zip(lower, upper)]
    return lo, hi, boxed


def thetas(M, b, d, w, p, values, mode, factors):
    """(ell, [[theta_{l,i}]])"""
    ell = lm.step_exponent(M, d, w)
    factors = [1.0] * d if factors is None else list(factors)
    lmax = lpm.lambda_max(b, w) if mode == RATIO else None
    out = []
    for v in values:
        row = []
        for f in factors:
            q = lm.to_fixed(v * f, p, w)
            assert q >= 0, "range condition: lambda1 w_i (or r w_i) must fit below the sign bit"
            row.append(lm.step(q if mode == ABSOLUTE else lm.mul(lmax, q, w, p), ell, w, p))
        out.append(row)
    return ell, out


def fista(M, b, d, w, p, iters, ell, theta, lo, hi):
    """the single solve's recurrence with per-coordinate theta and bounds: beta = x_N"""
    c = lm.coefficients(iters, w, p)
    x, y = [0] * d, [0] * d
    for k in range(iters):
        xn, yn = [0] * d, [0] * d
        for i in range(d):
            g = lm.wrap(sum(lm.mul(M[i][j], y[j], w, p) for j in range(d)) - b[i], w)
            z = lm.wrap(y[i] - lm.step(g, ell, w, p), w)
            xn[i] = clamp(lm.soft(z, theta[i], w), lo[i], hi[i])
            yn[i] = lm.wrap(xn[i] + lm.mul(lm.wrap(xn[i] - x[i], w), c[k], w, p), w)
        x, y = xn, yn
    return x


def lasso_opts(a_packed, b, d, w, p, iters, values, mode=ABSOLUTE, factors=None, lower=None, upper=None):
    """(betas, ell, thetas): betas[l] = x_N of value l; a_packed / b: the words every solver sees after the prefix"""
    M = lm.full_matrix(a_packed, d, w)
    b = [lm.wrap(int(v), w) for v in b]
    ell, th = thetas(M, b, d, w, p, values, mode, factors)
    lo, hi, _ = bound_words(lower, upper, d, w, p)
    return [fista(M, b, d, w, p, iters, ell, t, lo, hi) for t in th], ell, th


def prox_record(m, r, W):
    """OP_PROX on the word file W (unsigned words) with the model m (word_model.Model).  Unflagged: word_model's record;
    flagged (bit 31 of cnt): the constant is b | (cnt & 0x7fffffff) << 32, and x' is clamped to [W[c + 3], W[c + 4]]
    before dx, y' and hdiff(y') are formed"""
    op, cnt, dst, a, b, c, sa, sb = [int(x) for x in r]
    if not cnt & BOUNDED:
        m.exec(r, W, [], {}, set(), set())
        return
    w, M32 = m.w, 0xFFFFFFFF
    s = lambda v: wm.s(v, w)
    yi = (dst + sa) & M32
    g = m.sub(W[a], W[(a + sa) & M32])
    z = m.sub(W[yi], m.step_shift(g, W[c]))
    xn = wm.u(clamp(lm.soft(s(z), s(W[c + 1]), w), s(W[c + 3]), s(W[c + 4])), w)
    dx = m.sub(xn, W[dst])
    coef = b | ((cnt & (BOUNDED - 1)) << 32)
    yn = m.add(xn, wm.u(s(dx) * coef >> m.p, w))
    W[dst], W[yi] = xn, yn
    if sb:
        W[(yi + sb) & M32] = m.hdiff(yn)


# ---- a corpus of flagged OP_PROX records on edge operands (op_corpus.Corpus), for the per-op tests
def _bound_pairs(w, rng):
    """(lo, hi) signed pairs with lo <= hi: both extremes, one extreme, lo = hi, around 0, random"""
    lo_w, hi_w = -(1 << (w - 1)), (1 << (w - 1)) - 1
    r = sorted(int(v) - (1 << (w - 2)) for v in rng.integers(0, 1 << (w - 1), 2, dtype=np.uint64))
    return [(lo_w, hi_w), (0, hi_w), (lo_w, 0), (lo_w, lo_w), (hi_w, hi_w), (0, 0), (-1, 1), (5, 5), (r[0], r[1]),
            (-(1 << (w - 3)), 1 << (w - 3))]


def bounds_corpus(w, p, rng, n_rand=24):
    """the corpus (op_corpus.Corpus) of flagged OP_PROX records: every bound pair against edge (M y)_i, b_i, x_i, y_i, steps both ways,
    theta in {0, 1, random, near the top} and momentum constants; with hdiff(y') at w = 64 on every other record"""
    import op_corpus as oc
    from helpers import edge_operands
    M32 = 0xFFFFFFFF

    def once(n_inputs):
        C = oc.Corpus(w, p, n_inputs)
        mdl = wm.Model(None, w, p)
        a, b = (list(map(int, v)) for v in edge_operands(rng_fixed(), w, n_rand))
        recs = []
        for i, ell in enumerate((0, max(p - 3, 0), p, p + 1, p + 7, 2 * w)):
            theta = [0, 1, 12345 % (1 << (w - 2)), (1 << (w - 1)) - 1][i % 4]
            for j, coef in enumerate((0, 1, (1 << p) - 1, 0x0123456789abcdef & ((1 << p) - 1))):
                for q, (lo, hi) in enumerate(pairs):
                    E = C.inp([mdl.step_word(ell), theta, wm.u(-theta, w), wm.u(lo, w), wm.u(hi, w)])
                    k = (7 * i + 13 * j + 5 * q) % len(a)
                    g = C.inp([a[k], b[k]])                                      # (M y)_i, b_i
                    x = C.inp([b[(k + 1) % len(b)], a[(k + 3) % len(a)]])          # x_i, y_i
                    sb = (C.out() - (x + 1)) if (w == 64 and (j + q) % 2) else 0
                    recs.append((wm.OP["PROX"], ((coef >> 32) & M32) | BOUNDED, x, g, coef & M32, E, 1, sb))
        C.launch("gen", recs)
        return C

    seed = int(rng.integers(0, 1 << 31))
    rng_fixed = lambda: np.random.default_rng(seed)
    pairs = _bound_pairs(w, np.random.default_rng(seed + 1))
    C0 = once(None)
    return once(len(C0.inputs))


def corpus_words(C):
    """every word of the corpus after its launches, by prox_record (the revealed words of the corpus program)"""
    m = wm.Model(None, C.w, C.p)
    W = C.words0()
    for _, recs in C.launches:
        for r in recs:
            prox_record(m, r, W)
    return W
