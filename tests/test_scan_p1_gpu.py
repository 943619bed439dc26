"""lgc_p1_local_scan and lgc_p1_set_divisor (include/linreg_gc_scan.h) on the MI355X: p1_scan_kernel against numpy uint64
wrap-around arithmetic, and every word bit for bit against lgc_p1_local / lgc_p1_local_yy over the whole column range with the
same divisor.  Inputs are full-range words (sign-extended from 32 bits at w = 32), so every sum wraps.  The shapes are named
after what they cross: the passes of 32 columns of Z (nz = 1, 2, 32, 33), the 256 candidate columns of a workgroup (1, 255, 256,
257), the 16-row slab (n = 1, 15, 16, 17) and the first row count that splits K (n = 600)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (name, n, own covariates nc, with_y, candidates ns): nz = nc + with_y
SHAPES = [
    ("nz1_no_covariate", 17, 0, True, 3),
    ("nz2", 15, 1, True, 5),
    ("nz2_without_y", 16, 2, False, 4),
    ("nz32_one_pass", 17, 31, True, 2),
    ("nz33_two_passes", 17, 32, True, 3),
    ("one_row_one_candidate", 1, 1, True, 1),
    ("candidates_255", 16, 2, True, 255),
    ("candidates_256", 15, 2, True, 256),
    ("candidates_257_two_groups", 17, 2, True, 257),
    ("n600_splits_k", 600, 3, True, 257),
    ("n600_two_passes", 600, 33, True, 5),
]


def _data(rng, n, d, w):
    lo, hi = (-2 ** 63, 2 ** 63) if w == 64 else (-2 ** 31, 2 ** 31)
    return rng.integers(lo, hi, (n, d), dtype=np.int64, endpoint=False), rng.integers(lo, hi, n, dtype=np.int64, endpoint=False)


def _wrap_gram(X, y, w):
    """[X, y]^T [X, y] mod 2^w in numpy uint64 wrap-around arithmetic"""
    Z = np.column_stack([X, y]).astype(np.uint64)
    with np.errstate(over="ignore"):
        G = (Z[:, :, None] * Z[:, None, :]).sum(axis=0, dtype=np.uint64)
    return G & np.uint64((1 << w) - 1)


def _check(h, X, y, w, nc, ns, with_y, pad=1):
    """the own covariates are columns [pad, pad + nc), the candidates the ns columns behind them"""
    d = X.shape[1]
    c0, c1, s0, s1 = pad, pad + nc, pad + nc, pad + nc + ns
    G = _wrap_gram(X, y, w)
    out = h.local_scan(c0, c1, s0, s1, with_y=with_y)
    H, gg = out[0], out[1]
    assert H.shape == (ns, nc) and H.tolist() == G[s0:s1, c0:c1].tolist()
    if with_y:
        assert out[2].tolist() == G[s0:s1, d].tolist()
    # bit for bit against the existing local call over the whole range [c0, s1), the floating-point diagonal included
    ref = h.local_yy(c0, s1) if with_y else (h.local(c0, s1),)
    A = ref[0]
    tri = lambda i, j: i * (i + 1) // 2 + j
    assert gg.tolist() == [int(A[tri(nc + m, nc + m)]) for m in range(ns)]
    assert H.tolist() == [[int(A[tri(nc + m, i)]) for i in range(nc)] for m in range(ns)]
    if with_y:
        assert out[2].tolist() == ref[1][nc:].tolist()
    return out


@pytest.mark.parametrize("w,p", [(64, 56), (32, 28)])
@pytest.mark.parametrize("name,n,nc,with_y,ns", SHAPES, ids=[s[0] for s in SHAPES])
def test_local_scan_against_numpy_and_local(lgc, name, n, nc, with_y, ns, w, p):
    rng = np.random.default_rng([n, nc, ns, w])
    d = 1 + nc + ns + 1                                   # a column before and one behind, owned by nobody here
    X, y = _data(rng, n, d, w)
    h = lgc.Phase1(X, y, w, p)
    _check(h, X, y, w, nc, ns, with_y)
    h.close()


def test_row_window_device_io_and_divisor(lgc):
    """lgc_p1_set_rows: the call acts on the window as an object created from those rows would; lgc_p1_set_device_io changes
    nothing for a local call (its outputs are host memory, as lgc_p1_local's); lgc_p1_set_divisor(d) on a fresh object leaves
    every result unchanged, and another divisor changes the floating-point diagonals of lgc_p1_local and lgc_p1_local_scan
    alike and no other word"""
    w, p, n, nc, ns = 64, 56, 700, 3, 260
    rng = np.random.default_rng(9)
    d = 1 + nc + ns + 1
    X, y = _data(rng, n, d, w)
    h = lgc.Phase1(X, y, w, p)
    before = _check(h, X, y, w, nc, ns, True)
    full = h.local_yy(1, 1 + nc + ns)
    h.set_divisor(d)                                      # the default: nothing moves
    after = _check(h, X, y, w, nc, ns, True)
    assert all(a.tolist() == b.tolist() for a, b in zip(before, after))
    again = h.local_yy(1, 1 + nc + ns)
    assert all(np.asarray(a).tolist() == np.asarray(b).tolist() for a, b in zip(full, again))
    L = lgc.lib()
    L.lgc_p1_set_device_io.argtypes = [C.c_void_p, C.c_int]; L.lgc_p1_set_device_io.restype = C.c_int
    assert L.lgc_p1_set_device_io(h._h, 1) == 0
    dev = _check(h, X, y, w, nc, ns, True)
    assert all(a.tolist() == b.tolist() for a, b in zip(before, dev))
    assert L.lgc_p1_set_device_io(h._h, 0) == 0
    r0, r1 = 37, 655                                      # 618 rows: splits K, ends inside a slab
    h.set_rows(r0, r1)
    win = _check(h, X[r0:r1], y[r0:r1], w, nc, ns, True)
    fresh = lgc.Phase1(X[r0:r1], y[r0:r1], w, p)
    ref = _check(fresh, X[r0:r1], y[r0:r1], w, nc, ns, True)
    assert all(a.tolist() == b.tolist() for a, b in zip(win, ref))
    fresh.close()
    h.close()
    # (full-range words overflow the double diagonal into the "integer indefinite" word whatever the divisor; the diagonal is
    # sum x^2 / divisor: words below 2^23 keep 700 rows of it below 2^56)
    Xs, ys = X >> 41, y >> 41
    h = lgc.Phase1(Xs, ys, w, p)
    before = _check(h, Xs, ys, w, nc, ns, True)
    h.set_divisor(nc + 1)                                 # a scan's providers: c + 1
    other = _check(h, Xs, ys, w, nc, ns, True)            # (still bit for bit lgc_p1_local's with the same divisor)
    assert other[0].tolist() == before[0].tolist() and other[2].tolist() == before[2].tolist()
    assert all(0 < int(a) < int(b) < 2 ** 62 for a, b in zip(before[1], other[1]))      # d = 265 against c + 1 = 4
    h.close()


def test_rejections(lgc):
    rng = np.random.default_rng(5)
    X, y = _data(rng, 9, 6, 64)
    h = lgc.Phase1(X, y, 64, 56)
    for args, want in (((0, 2, 2, 2), "bad candidate range"), ((0, 2, 3, 7), "bad candidate range"), ((3, 2, 4, 5), "bad covariate range"),
                       ((0, 3, 2, 5), "overlap the covariates"), ((2, 5, 0, 3), "overlap the covariates")):
        with pytest.raises(lgc.LgcError) as e:
            h.local_scan(*args, with_y=True)
        assert e.value.code == -1 and want in str(e.value), str(e.value)
    with pytest.raises(lgc.LgcError) as e:
        h.set_divisor(0)
    assert "divisor" in str(e.value)
    assert h.local_scan(3, 5, 0, 3, with_y=True)[0].shape == (3, 2)          # candidates may lie before the covariates
    h.close()
    no_y = lgc.Phase1(X, None, 64, 56)
    with pytest.raises(lgc.LgcError) as e:
        no_y.local_scan(0, 2, 2, 4, with_y=True)
    assert "y requested but not set" in str(e.value)
    assert no_y.local_scan(0, 2, 2, 4)[1].shape == (2,)
    no_y.close()
