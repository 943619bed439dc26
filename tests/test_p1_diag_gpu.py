"""p1_diag_kernel (csrc/phase1.hip), the IEEE-double diagonal of X^T X added in k-ascending order, on the MI355X against
p1_model.diag_word: the diagonal words of lgc_p1_local, of lgc_p1_local_scan (gg) and of lgc_p1_local_folds.  The kernel takes 600
rows at a time through two LDS buffers, fifteen waves forming the terms of one chunk (a wave's quarter r0 reads rows r0 + 60 u)
while the first wave adds those of the chunk before; a workgroup owns 16 columns.  Inputs and reference words are those of
tests/p1_diag_data.py; test_p1_model_cpu.py shows that the w = 64 words depend on the order of the additions (every addition
rounds), that no in-range word is saturated and that every word of the saturating inputs is.  The off-diagonal words of these
calls are test_p1_blocks_gpu.py's."""
import numpy as np
import pytest

import p1_diag_data as dd

pytestmark = pytest.mark.gpu

C0, OWN, D = dd.C0, dd.OWN, dd.D


def _diag(A, own):
    """the diagonal of a packed lower triangle"""
    i = np.arange(own)
    return A[i * (i + 1) // 2 + i].tolist()


def _check(h, c0, c1, ref):
    """local and local_scan over the window of h: columns [c0, c1) as the own block, and as the candidates of a scan with column
    c0 - 1 as the one covariate"""
    ref = list(ref)
    assert _diag(h.local(c0, c1), c1 - c0) == ref
    H, gg = h.local_scan(c0 - 1, c0, c0, c1)
    assert gg.tolist() == ref


@pytest.mark.parametrize("w,p", dd.WIDTHS)
@pytest.mark.parametrize("n", dd.ROWS)
def test_rows(lgc, n, w, p):
    h = lgc.Phase1(dd.in_range(n, D, w), None, w, p)
    _check(h, C0, C0 + OWN, dd.words("in_range", n, D, w, C0, C0 + OWN, D))
    h.close()


@pytest.mark.parametrize("w,p", dd.WIDTHS)
@pytest.mark.parametrize("own", dd.OWNS)
def test_columns(lgc, own, w, p):
    n, d = dd.OWNS_N, own + 2
    h = lgc.Phase1(dd.in_range(n, d, w), None, w, p)
    _check(h, C0, C0 + own, dd.words("in_range", n, d, w, C0, C0 + own, d))
    h.close()


@pytest.mark.parametrize("w,p", dd.WIDTHS)
def test_row_folds_and_row_windows(lgc, w, p):
    """K = 2 folds of 1201 rows: 600 and 601 rows, each launch with the base of its own fold; the same ranges as row windows"""
    n, K = dd.FOLDS_N, len(dd.FOLDS)
    h = lgc.Phase1(dd.in_range(n, D, w), None, w, p)
    A = h.local_folds(C0, C0 + OWN, K)
    assert A.shape == (K, OWN * (OWN + 1) // 2)
    for k, (r0, r1) in enumerate(dd.FOLDS):
        assert lgc.fold_rows(n, K, k) == (r0, r1)
        ref = dd.words("in_range", n, D, w, C0, C0 + OWN, D, r0, r1)
        assert _diag(A[k], OWN) == list(ref)
        h.set_rows(r0, r1)
        _check(h, C0, C0 + OWN, ref)
        h.set_rows(0, n)
    h.close()


@pytest.mark.parametrize("w,p", dd.WIDTHS)
def test_divisor(lgc, w, p):
    """lgc_p1_set_divisor holds for every later call; the default is d"""
    n = dd.DIVISORS_N
    h = lgc.Phase1(dd.in_range(n, D, w), None, w, p)
    refs = {v: dd.words("in_range", n, D, w, C0, C0 + OWN, v) for v in (1, 7, D)}
    assert len(set(refs.values())) == 3
    _check(h, C0, C0 + OWN, refs[D])
    for v in (1, 7, D):
        h.set_divisor(v)
        _check(h, C0, C0 + OWN, refs[v])
    h.close()


@pytest.mark.parametrize("w,p", dd.WIDTHS)
def test_boundary_words(lgc, w, p):
    """n = 1, divisor 1: the last x whose square is a w-bit signed word, and the first beyond it on either side"""
    X, ref = dd.boundary(w)
    X = np.column_stack([np.zeros((1, 1), dtype=np.int64), X])          # (a covariate for the scan)
    h = lgc.Phase1(X, None, w, p)
    h.set_divisor(1)
    _check(h, 1, X.shape[1], ref)
    h.close()


@pytest.mark.parametrize("w,p", dd.WIDTHS)
def test_saturation_on_full_range_data(lgc, w, p):
    n = dd.SAT_N
    h = lgc.Phase1(dd.full_range(n, D, w), None, w, p)
    ref = dd.words("full_range", n, D, w, C0, C0 + OWN, D)
    assert set(ref) == {1 << (w - 1)}
    _check(h, C0, C0 + OWN, ref)
    h.close()
