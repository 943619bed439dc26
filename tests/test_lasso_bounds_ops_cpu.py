"""The bounded OP_PROX record (bit 31 of cnt) on edge operands, on the CPU checker's plaintext machine and its garble +
evaluate backends, against the record model of tests/lasso_bounds_model.py.  No GPU needed."""
import numpy as np
import pytest

import lasso_bounds_model as lbm
import linreg_gc
import op_corpus as oc
import word_model as wm


def _mismatches(C, got, want):
    m = wm.mask(C.w)
    return ["word %d: got 0x%x, expected 0x%x" % (i, int(got[i]) & m, want[i]) for i in range(len(want))
            if int(got[i]) & m != want[i]][:8]


@pytest.mark.parametrize("w", [64, 32])
def test_flagged_prox_plain(gccpu, w):
    for p in (1, w - 8, w - 1):
        C = lbm.bounds_corpus(w, p, np.random.default_rng([w, p]))
        prog = C.program(linreg_gc, lambda kind: ("auto", "auto"))
        got = oc.plain_words(gccpu, prog, C)
        bad = _mismatches(C, got, lbm.corpus_words(C))
        assert not bad, (w, p, bad)


@pytest.mark.parametrize("w", [64, 32])
def test_flagged_prox_garbled(gccpu, w):
    p = w - 8
    C = lbm.bounds_corpus(w, p, np.random.default_rng([w, p, 1]))
    prog = C.program(linreg_gc, lambda kind: ("auto", "auto"))
    got, gates, _ = gccpu.garble_eval(prog, np.array(C.inputs, dtype=np.uint64))
    assert gates == prog.info.total_gates
    bad = _mismatches(C, got, lbm.corpus_words(C))
    assert not bad, bad


def test_clamp_reaches_every_branch():
    """the corpus exercises v < lo, v > hi and v inside, and records whose result is an extreme word"""
    w, p = 64, 56
    C = lbm.bounds_corpus(w, p, np.random.default_rng(5))
    W = lbm.corpus_words(C)
    below = above = inside = 0
    for r in C.launches[0][1]:
        x, c = r[2], r[5]
        lo, hi, v = wm.s(W[c + 3], w), wm.s(W[c + 4], w), wm.s(W[x], w)
        assert lo <= v <= hi
        below += v == lo and lo != hi
        above += v == hi and lo != hi
        inside += lo < v < hi
    assert below > 10 and above > 10 and inside > 10, (below, above, inside)
