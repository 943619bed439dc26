"""An independent model of the lasso path's in-circuit model selection (include/linreg_gc_lasso_select.h) in
Python integers.

It restates the definition on top of the path models (tests/lasso_path_model.py, tests/lasso_bounds_model.py) and shares no
code with the product.  beta_l = x_N of value l; on the validation system (M_v, b_v), all mod 2^w:
  t_i = sum_j mul(M_v,ij, beta_l,j);  r_i = 2 b_v,i - t_i;  score_l = 0 - sum_i mul(beta_l,i, r_i)
  l* = the smallest l whose score is the SIGNED minimum;  beta* = beta_{l*}
M_v, b_v: the share sums; on the data-provider path the off-diagonal entries and b_v divided by d (truncating), the diagonal
as summed; no lambda2.  The three record variants the selection is lowered to are modelled at the end, with a corpus of them
on edge operands.
"""
import numpy as np

import lasso_bounds_model as lbm
import lasso_model as lm
import word_model as wm

ABSOLUTE, RATIO = lbm.ABSOLUTE, lbm.RATIO
REVEAL_INDEX, REVEAL_SCORES = 1, 2


def tdiv(a, c):
    """a / c truncated toward zero (OP_IDIVC)"""
    return -((-a) // c) if a < 0 else a // c


def validation_system(shares_v, d, w, normalize):
    """(M_v as a d x d list, b_v) from the validation halves of the shares: rows of T + d words, A_v packed then b_v"""
    T = d * (d + 1) // 2
    tot = [lm.wrap(sum(int(s[k]) for s in shares_v), w) for k in range(T + d)]
    if normalize:
        k = 0
        for i in range(d):
            for j in range(i + 1):
                if j < i:
                    tot[k] = tdiv(tot[k], d)
                k += 1
        for i in range(d):
            tot[T + i] = tdiv(tot[T + i], d)
    return lm.full_matrix(tot[:T], d, w), tot[T:]


def score(Mv, bv, beta, d, w, p):
    acc = 0
    for i in range(d):
        t = lm.wrap(sum(lm.mul(Mv[i][j], beta[j], w, p) for j in range(d)), w)
        r = lm.wrap(2 * bv[i] - t, w)
        acc += lm.mul(beta[i], r, w, p)
    return lm.wrap(-acc, w)


def argmin_first(scores):
    """the smallest index of a minimal (signed) score"""
    return min(range(len(scores)), key=lambda l: (scores[l], l))


def select(betas, Mv, bv, d, w, p):
    """(beta*, l*, scores)"""
    sc = [score(Mv, bv, b, d, w, p) for b in betas]
    best = argmin_first(sc)
    return betas[best], best, sc


def lasso_select(a_packed, b, shares_v, d, w, p, iters, values, mode, normalize, factors=None, lower=None, upper=None):
    """(beta*, l*, scores, betas): a_packed / b are the training words every solver sees after the prefix; shares_v the
    validation halves of the raw shares"""
    betas = lbm.lasso_opts(a_packed, b, d, w, p, iters, values, mode, factors, lower, upper)[0]
    Mv, bv = validation_system(shares_v, d, w, normalize)
    return select(betas, Mv, bv, d, w, p) + (betas,)


def revealed(beta_star, index, scores, flags):
    """the words a selection reveals, in order: beta*, [l*], [scores]"""
    return list(beta_star) + ([index] if flags & REVEAL_INDEX else []) + (list(scores) if flags & REVEAL_SCORES else [])


# ---- the three record variants on a word file W of unsigned words: (op, cnt, dst, a, b, c, sa, sb)
def variant_record(r, W, w):
    op, cnt, dst, a, b, c, sa, sb = [int(x) for x in r]
    full = wm.mask(w)
    if op == wm.OP["MAX"] and b == 2:                        # the signed minimum of cnt words
        W[dst] = wm.u(min(wm.s(W[a + k * sa], w) for k in range(cnt)), w)
    elif op == wm.OP["EQ"] and cnt >= 2:                     # first-match one-hot and its index
        hit = [k for k in range(cnt) if W[a + k * sa] == W[b]]
        vals = [full if hit and k == hit[0] else 0 for k in range(cnt)]
        for k in range(cnt):
            W[dst + k] = vals[k]
        W[c] = hit[0] if hit else 0
    elif op == wm.OP["SUM"] and b != 0:                      # gated select
        v = 0
        for k in range(cnt):
            v ^= W[b + k * sb] & W[a + k * sa]
        W[dst] = v & full
    else:
        raise ValueError("not a selection variant: %r" % (r,))


CNTS = (2, 7, 8, 9, 64, 256)


def _placements(cnt):
    """where the minimum sits: first, a middle position, last, several at once"""
    mid = cnt // 2
    out = [[0], [cnt - 1], [0, cnt - 1]]
    if cnt > 2:
        out += [[mid], [1, mid, cnt - 1]]
    return out


def select_corpus(w, p, rng, cnts=CNTS):
    """the corpus (op_corpus.Corpus) of the three variants.  Per cnt and placement of the minimum a vector of `cnt` scores drawn
    from -2^(w-1), -1, 0, 2^(w-1) - 1 and random words, with the minimum value forced at the placement: one signed-minimum
    record, one first-match record against that minimum (and one against a word no candidate equals), one launch later a
    gated select of `cnt` value words by the one-hot words, and a gated select whose gate words are all zero"""
    import op_corpus as oc
    seed = int(rng.integers(0, 1 << 31))
    lo_w, hi_w = -(1 << (w - 1)), (1 << (w - 1)) - 1

    def once(n_inputs):
        g = np.random.default_rng(seed)
        C = oc.Corpus(w, p, n_inputs)
        mins, eqs, sels = [], [], []
        zeros = C.inp([0] * max(cnts))
        for cnt in cnts:
            for q, place in enumerate(_placements(cnt)):
                pool = [lo_w, -1, 0, hi_w] + [int(v) - (1 << 62) for v in g.integers(0, 1 << 63, 4, dtype=np.uint64)]
                pool = [lm.wrap(v, w) for v in pool]
                mn = [lo_w, -1, 0, hi_w, pool[4]][q % 5]      # the minimum is each edge value in turn
                cand = [v for v in pool if v > mn] or [mn]
                sc = [cand[int(g.integers(0, len(cand)))] for _ in range(cnt)]
                for k in place:
                    sc[k] = mn
                sa = 2 if q == 1 else 1                        # one placement per cnt reads its scores with a stride
                strided = []
                for v in sc:
                    strided += [wm.u(v, w)] + [0x5a] * (sa - 1)     # (the words between two scores are never read)
                iv = C.inp(strided)
                vals = C.inp([int(v) & wm.mask(w) for v in g.integers(0, 1 << 63, cnt, dtype=np.uint64) * 2 + 1])
                ref, other = C.inp([wm.u(mn, w)]), C.inp([wm.u(mn, w) ^ 1])
                m = C.out()
                mins.append((wm.OP["MAX"], cnt, m, iv, 2, 0, sa, 1))
                hot, idx, none, idx0 = C.out(cnt), C.out(), C.out(cnt), C.out()
                eqs.append((wm.OP["EQ"], cnt, hot, iv, ref, idx, sa, 1))
                eqs.append((wm.OP["EQ"], cnt, none, iv, other, idx0, sa, 1))   # (mn ^ 1 is no candidate's value)
                o = C.out(2)
                sels.append((wm.OP["SUM"], cnt, o, vals, hot, 0, 1, 1))
                sels.append((wm.OP["SUM"], cnt, o + 1, vals, zeros, 0, 1, 1))
        C.launch("gen", mins)
        C.launch("gen", eqs)
        C.launch("gen", sels)
        return C

    return once(len(once(None).inputs))


def corpus_words(C):
    """every word of the corpus after its launches, by variant_record"""
    W = C.words0()
    for _, recs in C.launches:
        for r in recs:
            variant_record(r, W, C.w)
    return W
