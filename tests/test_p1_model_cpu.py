"""tests/p1_model.py against the oracle and against Python integers, and the conditions on the inputs of test_p1_diag_gpu.py
(tests/p1_diag_data.py) without which its comparisons could pass for the wrong reason: the w = 64 in-range words change when the
rows are summed in another order, no in-range word is the saturated word, every word of the saturating inputs is."""
import numpy as np
import pytest

import p1_diag_data as dd
import p1_model


def _oracle_diag(oracle, X, p, w):
    """the diagonal of oracle.aggregate over all of X: its divisor is the column count"""
    n, d = X.shape
    A, _ = oracle.aggregate(X, np.zeros(n, dtype=np.int64), n, d, p, w)
    return [int(A[oracle.lib.orc_idx(i, i)]) for i in range(d)]


def _oracle_word(oracle, col, p, w, divisor):
    """any divisor: the oracle's conversions around the k-ascending sum of diag_share"""
    xy = 0.0
    for x in col:
        v = oracle.lib.orc_fixed_to_double(int(x), p)
        xy += (v * v) * float(1 << p)
    return oracle.lib.orc_double_to_fixed(xy / float(divisor), p, w) & ((1 << w) - 1)


@pytest.mark.parametrize("n,d,p,w", [(300, 7, 56, 64), (1000, 70, 56, 64), (257, 9, 30, 32), (5000, 130, 54, 64)])
def test_diag_word_matches_oracle_on_quantised_data(oracle, n, d, p, w):
    """the shapes and the data of test_gpu_phase1.py::test_local_block_matches_oracle"""
    rng = np.random.default_rng(n + d)
    X = rng.standard_normal((n, d)); X /= np.abs(X).max(axis=0)
    Xq = oracle.quantize(X, p, n, w).reshape(n, d)
    assert p1_model.diag_words(Xq, 0, d, p, w, d) == _oracle_diag(oracle, Xq, p, w)


def test_in_range_words_match_oracle_and_are_not_saturated(oracle):
    cases = dd.in_range_cases()
    assert len(cases) == 2 * (len(dd.ROWS) + len(dd.OWNS) + len(dd.FOLDS) + 3)
    for n, d, w, c0, c1, divisor, r0, r1 in cases:
        p = dd.PREC[w]
        X = dd.in_range(n, d, w)[r0:r1]
        ref = list(dd.words("in_range", n, d, w, c0, c1, divisor, r0, r1))
        assert len(ref) == c1 - c0
        assert p1_model.saturated(w) not in ref, (n, d, w, divisor)
        if divisor == d:
            assert ref == _oracle_diag(oracle, X, p, w)[c0:c1], (n, d, w, r0, r1)
        else:
            assert ref == [_oracle_word(oracle, X[:, c], p, w, divisor) for c in range(c0, c1)], (n, d, w, divisor)


def test_in_range_words_at_64_bits_depend_on_the_order_of_the_rows():
    """a kernel that adds the terms of a column in another order than k ascending must not pass: with the rows reversed, at least
    one of the 17 words differs at every row count from 59 on (in fact most of them do)"""
    w, p = 64, 56
    for n in [n for n in dd.ROWS if n >= 59] + [dd.OWNS_N, dd.DIVISORS_N]:
        X = dd.in_range(n, dd.D, w)
        fwd = dd.words("in_range", n, dd.D, w, dd.C0, dd.C0 + dd.OWN, dd.D)
        rev = p1_model.diag_words(X[::-1], dd.C0, dd.C0 + dd.OWN, p, w, dd.D)
        changed = sum(a != b for a, b in zip(fwd, rev))
        print("n = %d: %d of %d words change with the rows reversed" % (n, changed, dd.OWN))
        assert changed >= 1, n
    for r0, r1 in dd.FOLDS:
        X = dd.in_range(dd.FOLDS_N, dd.D, w)[r0:r1]
        fwd = dd.words("in_range", dd.FOLDS_N, dd.D, w, dd.C0, dd.C0 + dd.OWN, dd.D, r0, r1)
        assert list(fwd) != p1_model.diag_words(X[::-1], dd.C0, dd.C0 + dd.OWN, p, w, dd.D), (r0, r1)


@pytest.mark.parametrize("w,p", dd.WIDTHS)
def test_every_word_of_the_saturating_inputs_is_saturated(oracle, w, p):
    X = dd.full_range(dd.SAT_N, dd.D, w)
    ref = list(dd.words("full_range", dd.SAT_N, dd.D, w, 0, dd.D, dd.D))
    assert ref == [p1_model.saturated(w)] * dd.D
    assert ref == _oracle_diag(oracle, X, p, w)
    assert p1_model.saturated(32) == 0x80000000 and p1_model.saturated(64) == 0x8000000000000000


@pytest.mark.parametrize("w,x,word", dd.BOUNDARY)
def test_boundary_words(oracle, w, x, word):
    """n = 1, divisor 1: the word is x^2 (rounded to 53 bits at w = 64: within 2^9) below 2^(w-1), saturated from there on"""
    p = dd.PREC[w]
    assert (x * x < 1 << (w - 1)) == (word != p1_model.saturated(w))
    if word != p1_model.saturated(w):
        assert abs(word - x * x) <= (0 if w == 32 else 1 << 9)
    assert p1_model.diag_word([x], p, w, 1) == word
    assert _oracle_diag(oracle, np.array([[x]], dtype=np.int64), p, w) == [word]      # d = 1: the oracle's divisor is 1
    assert _oracle_word(oracle, [x], p, w, 1) == word
    X, ws = dd.boundary(w)
    assert x in X[0].tolist() and ws[X[0].tolist().index(x)] == word


@pytest.mark.parametrize("w", [64, 32])
def test_share_models_match_python_integers(w):
    """mask, dot and ti_a in exact integers; X holds negative words, whose sign extension beyond bit w - 1 must not reach a result"""
    rng = np.random.default_rng([7, w])
    n, ld, M = 5, 3, 1 << w
    X = rng.integers(-(1 << (w - 1)), 1 << (w - 1), (n, ld), dtype=np.int64)
    X[0, 2] = -1; X[1, 2] = -(1 << (w - 1))
    cols = [2, 0, 1, 2]
    V, Y = (rng.integers(0, M, (len(cols), n), dtype=np.uint64, endpoint=False) for _ in range(2))
    sub = rng.integers(0, M, len(cols), dtype=np.uint64, endpoint=False)
    Xi, Vi, Yi, si = X.tolist(), V.tolist(), Y.tolist(), sub.tolist()
    for sign in (+1, -1):
        exp = [[(Xi[k][c] + sign * Vi[q][k]) % M for k in range(n)] for q, c in enumerate(cols)]
        assert p1_model.mask(X, cols, V, sign, w).tolist() == exp
    exp = [(sum(Vi[q][k] * Yi[q][k] for k in range(n)) - si[q]) % M for q in range(len(cols))]
    assert p1_model.dot(V, Y, sub, w).tolist() == exp
    exp = [sum(Vi[q][k] * Xi[k][c] for k in range(n)) % M for q, c in enumerate(cols)]
    assert p1_model.dot(V, p1_model.columns(X, cols), None, w).tolist() == exp
    a, s = p1_model.ti_a(X, cols, Y, V, sub, w)
    assert a.tolist() == [[(Xi[k][c] - Yi[q][k]) % M for k in range(n)] for q, c in enumerate(cols)]
    assert s.tolist() == [(sum(Vi[q][k] * Yi[q][k] for k in range(n)) - si[q]) % M for q in range(len(cols))]
