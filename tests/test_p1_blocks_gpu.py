"""The integer words of lgc_p1_local / _yy, lgc_p1_local_folds_yy and lgc_p1_local_targets on the MI355X against numpy uint64
wrap-around arithmetic of [X, Y]^T [X, Y]: the off-diagonal words of A, b, yy, and B of the targets call.  Inputs are full-range
words (sign-extended from 32 bits at w = 32), so every sum wraps.  These calls share one tile body, one split-K rule and, for the
Gram blocks, one kernel that reads its row ranges from a table; the shapes are the smallest that cross the 16-row slab, the first
row count that splits K, a second chunk that is no multiple of 16, and the 64-column tile.  (The floating-point diagonal of A is
p1_diag_kernel's and is pinned against a model of its own in test_p1_diag_gpu.py.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIDTHS = [(64, 56), (32, 28)]

# (name, n, d, c0, c1, with_y)
LOCAL = [
    ("one_row", 1, 3, 0, 3, True),
    ("slab_less_one", 15, 3, 0, 3, True),
    ("one_slab", 16, 3, 0, 3, True),
    ("slab_and_one", 17, 3, 0, 3, True),
    ("n511_last_unsplit", 511, 3, 1, 3, True),
    ("n512_two_chunks_of_256", 512, 3, 1, 3, True),
    ("n527_chunks_272_255", 527, 3, 1, 3, True),
    ("own63_one_ragged_tile", 17, 67, 2, 65, False),
    ("own64_y_two_tile_rows", 17, 68, 2, 66, True),          # L = 65: the skipped upper tile, a ragged tile of one column
]
# (n, own, k)
TARGETS = [(1, 1, 1), (16, 64, 64), (17, 65, 65), (527, 3, 2)]


def _data(rng, shape, w):
    lo, hi = (-2 ** 63, 2 ** 63) if w == 64 else (-2 ** 31, 2 ** 31)
    return rng.integers(lo, hi, shape, dtype=np.int64, endpoint=False)


def _wrap_gram(X, Y, w):
    """[X, Y]^T [X, Y] mod 2^w in numpy uint64 wrap-around arithmetic"""
    Z = np.column_stack([X, Y]).astype(np.uint64)
    with np.errstate(over="ignore"):
        G = (Z[:, :, None] * Z[:, None, :]).sum(axis=0, dtype=np.uint64)
    return G & np.uint64((1 << w) - 1)


def _check_A(A, G, c0, c1):
    """the off-diagonal words of the packed lower triangle"""
    own = c1 - c0
    assert A.shape == (own * (own + 1) // 2,)
    i, j = np.tril_indices(own, -1)
    assert A[i * (i + 1) // 2 + j].tolist() == G[c0 + i, c0 + j].tolist()


@pytest.mark.parametrize("w,p", WIDTHS)
@pytest.mark.parametrize("name,n,d,c0,c1,with_y", LOCAL, ids=[s[0] for s in LOCAL])
def test_local_against_numpy(lgc, name, n, d, c0, c1, with_y, w, p):
    rng = np.random.default_rng([n, d, c1 - c0, w])
    X, y = _data(rng, (n, d), w), _data(rng, n, w)
    G = _wrap_gram(X, y, w)
    h = lgc.Phase1(X, y, w, p)
    if with_y:
        A, b, yy = h.local_yy(c0, c1)
        assert b.tolist() == G[c0:c1, d].tolist()            # y is column d: cols[] is not contiguous when c1 < d
        assert int(yy) == int(G[d, d])
        A2, b2 = h.local(c0, c1, with_y=True)                # the older call: the same launches, yy dropped
        assert A2.tolist() == A.tolist() and b2.tolist() == b.tolist()
    else:
        A = h.local(c0, c1)
    _check_A(A, G, c0, c1)
    h.close()


@pytest.mark.parametrize("w,p", WIDTHS)
def test_local_folds_against_numpy_and_windowed_local(lgc, w, p):
    """K = 2 folds of 527 rows: the chunking of n527_chunks_272_255 above, reached through two table entries per fold"""
    n, d, c0, c1, K = 1054, 3, 1, 3, 2
    rng = np.random.default_rng([n, K, w])
    X, y = _data(rng, (n, d), w), _data(rng, n, w)
    h = lgc.Phase1(X, y, w, p)
    A, b, yy = h.local_folds_yy(c0, c1, K)
    assert A.shape == (K, 3) and b.shape == (K, 2) and yy.shape == (K,)
    for k in range(K):
        r0, r1 = lgc.fold_rows(n, K, k)
        assert r1 - r0 == 527
        G = _wrap_gram(X[r0:r1], y[r0:r1], w)
        _check_A(A[k], G, c0, c1)
        assert b[k].tolist() == G[c0:c1, d].tolist()
        assert int(yy[k]) == int(G[d, d])
        h.set_rows(r0, r1)
        wA, wb, wyy = h.local_yy(c0, c1)                     # every word, the floating-point diagonal included
        assert A[k].tolist() == wA.tolist() and b[k].tolist() == wb.tolist() and int(yy[k]) == int(wyy)
        h.set_rows(0, n)
    h.close()


@pytest.mark.parametrize("w,p", WIDTHS)
@pytest.mark.parametrize("n,own,k", TARGETS)
def test_local_targets_against_numpy(lgc, n, own, k, w, p):
    rng = np.random.default_rng([n, own, k, w])
    c0, d = 2, 2 + own + 1                                   # two columns before and one behind, owned by nobody here
    X, Y = _data(rng, (n, d), w), _data(rng, (n, k), w)
    G = _wrap_gram(X, Y, w)
    h = lgc.Phase1(X, Y, w, p, targets=k)
    A, B = h.local_targets(c0, c0 + own)
    assert B.shape == (k, own)
    assert B.tolist() == G[d:d + k, c0:c0 + own].tolist()    # B[t][i] = <column c0 + i, target t>
    _check_A(A, G, c0, c0 + own)
    h.close()
