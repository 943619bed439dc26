"""Phase 1 on row folds (include/linreg_gc_folds.h) on the MI355X: lgc_p1_local_folds against Python integers and against
lgc_p1_local on an object created from each fold's rows alone; the row window of lgc_p1_set_rows against objects created from
the window's rows.  Inputs are full-range words (sign-extended from 32 bits at w = 32), so every sum wraps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# n, K, d, c0, c1: folds of 16 / 17 rows straddle the 16-row slab; one row per fold; the smallest case; two tile rows with the
# triangle skip and a ragged tile; a fold of 1050 rows in four splits whose last chunk is no multiple of 16
SHAPES = [(83, 5, 5, 0, 5), (7, 7, 3, 0, 3), (2, 2, 1, 0, 1), (40, 3, 70, 2, 67), (4200, 4, 8, 0, 8)]


def _data(rng, n, d, w):
    if w == 64:
        X = rng.integers(-2 ** 63, 2 ** 63, (n, d), dtype=np.int64, endpoint=False)
        y = rng.integers(-2 ** 63, 2 ** 63, n, dtype=np.int64, endpoint=False)
    else:
        X = rng.integers(-2 ** 31, 2 ** 31, (n, d), dtype=np.int64, endpoint=False)
        y = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64, endpoint=False)
    return X, y


def _int_model(X, y, r0, r1, c0, c1, w):
    """off-diagonal words of the packed own block and X^T y over rows [r0, r1), in Python integers mod 2^w"""
    m = (1 << w) - 1
    cols = [[int(v) for v in X[r0:r1, c]] for c in range(c0, c1)]
    yy = [int(v) for v in y[r0:r1]]
    A = {}
    for i in range(c1 - c0):
        for j in range(i):
            A[i * (i + 1) // 2 + j] = sum(a * b for a, b in zip(cols[i], cols[j])) & m
    b = [sum(a * t for a, t in zip(cols[i], yy)) & m for i in range(c1 - c0)]
    return A, b


@pytest.mark.parametrize("with_y", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 28)])
@pytest.mark.parametrize("n,K,d,c0,c1", SHAPES)
def test_local_folds_is_k_local_calls(lgc, n, K, d, c0, c1, w, p, with_y):
    rng = np.random.default_rng([n, K, d, w, with_y])
    X, y = _data(rng, n, d, w)
    own = c1 - c0
    whole = lgc.Phase1(X, y, w, p)
    got = whole.local_folds(c0, c1, K, with_y=bool(with_y))
    gA, gb = got if with_y else (got, None)
    assert gA.shape == (K, own * (own + 1) // 2)
    for k in range(K):
        r0, r1 = lgc.fold_rows(n, K, k)
        alone = lgc.Phase1(X[r0:r1], y[r0:r1], w, p)                             # the parent's code on that fold's rows alone
        ref = alone.local(c0, c1, with_y=bool(with_y))
        rA, rb = ref if with_y else (ref, None)
        alone.close()
        assert gA[k].tolist() == rA.tolist(), (k, "A")                           # every word, the floating-point diagonal included
        if with_y:
            assert gb[k].tolist() == rb.tolist(), (k, "b")
        mA, mb = _int_model(X, y, r0, r1, c0, c1, w)                             # independent of any kernel
        assert all(int(gA[k][e]) == v for e, v in mA.items()), (k, "A vs integers")
        if with_y:
            assert [int(v) for v in gb[k]] == mb, (k, "b vs integers")
        # and the windowed call on the SAME object
        whole.set_rows(r0, r1)
        win = whole.local(c0, c1, with_y=bool(with_y))
        wA = win[0] if with_y else win
        assert wA.tolist() == rA.tolist(), (k, "window")
    whole.close()


@pytest.mark.parametrize("w,p", [(64, 56), (32, 28)])
def test_row_window_is_an_object_of_those_rows(lgc, w, p):
    n, d, r0, r1 = 83, 6, 17, 50
    rng = np.random.default_rng([w, 83])
    X, y = _data(rng, n, d, w)
    m = np.uint64((1 << w) - 1)
    win = lgc.Phase1(X, y, w, p)
    sub = lgc.Phase1(X[r0:r1], y[r0:r1], w, p)
    fresh = lgc.Phase1(X, y, w, p)
    nk = r1 - r0

    def same(a, b):
        a = a if isinstance(a, tuple) else (a,)
        b = b if isinstance(b, tuple) else (b,)
        assert len(a) == len(b) and all(np.array_equal(np.asarray(u), np.asarray(v)) for u, v in zip(a, b))

    def calls(o, nn):
        r = np.random.default_rng(nn)
        cols = np.array([0, 3, d, 5], dtype=np.uint32)                         # column d is y
        V = r.integers(0, 2 ** 64, (4, nn), dtype=np.uint64) & m
        W = r.integers(0, 2 ** 64, (4, nn), dtype=np.uint64) & m
        s = r.integers(0, 2 ** 64, 4, dtype=np.uint64) & m
        return [o.local(1, 5, with_y=True), o.mask(cols, V, +1), o.mask(cols[:1], V[:1], -1), o.dot(V, cols=cols, sub=s),
                o.dot(V, B=W), o.dot(V[:1], cols=cols[:1]), o.ti_a_batch(cols, V, W, s), o.ti_a(2, V[0], W[0], int(s[0]))]

    whole_before = calls(win, n)
    win.set_rows(r0, r1)
    assert win.n == nk and win.n_all == n
    for a, b in zip(calls(win, nk), calls(sub, nk)):
        same(a, b)
    win.set_rows(0, n)
    for a, b, c in zip(calls(win, n), calls(fresh, n), whole_before):
        same(a, b)
        same(a, c)
    for bad in ((5, 5), (0, n + 1), (7, 3)):
        with pytest.raises(lgc.LgcError) as e:
            win.set_rows(*bad)
        assert e.value.code == -1
    win.set_rows(0, n)
    with pytest.raises(lgc.LgcError):
        win.local_folds(0, 3, n + 1 if n < 16 else 17)
    with pytest.raises(lgc.LgcError):
        win.local_folds(0, 3, 1)
    for o in (win, sub, fresh):
        o.close()
