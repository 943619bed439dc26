"""lgc_p1_local_folds_yy (include/linreg_gc_folds_yy.h) on the MI355X: the folds' y^T y against Python integers mod 2^64, and
out_A / out_b word for word lgc_p1_local_folds's.  Inputs are full-range words (sign-extended from 32 bits at w = 32), so
every sum wraps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# n, K, d, c0, c1: unequal folds of one split each; several splits per fold (a fold of 550 rows keeps 256 rows per split);
# own = 1; own = 65: the y column alone in a second tile
SHAPES = [(37, 3, 4, 0, 4), (1100, 2, 6, 1, 6), (37, 3, 3, 1, 2), (37, 3, 66, 0, 65)]


def _data(rng, n, d, w):
    b = 63 if w == 64 else 31
    return (rng.integers(-2 ** b, 2 ** b, (n, d), dtype=np.int64, endpoint=False),
            rng.integers(-2 ** b, 2 ** b, n, dtype=np.int64, endpoint=False))


@pytest.mark.parametrize("w,p", [(64, 56), (32, 28)])
@pytest.mark.parametrize("n,K,d,c0,c1", SHAPES)
def test_yy_is_the_integer_gram_entry(lgc, n, K, d, c0, c1, w, p):
    rng = np.random.default_rng([n, K, d, c1, w])
    X, y = _data(rng, n, d, w)
    h = lgc.Phase1(X, y, w, p)
    A, b, yy = h.local_folds_yy(c0, c1, K)
    A0, b0 = h.local_folds(c0, c1, K, with_y=True)
    assert A.tolist() == A0.tolist() and b.tolist() == b0.tolist()          # word for word the older call's
    m = (1 << w) - 1
    sizes = set()
    for k in range(K):
        r0, r1 = lgc.fold_rows(n, K, k)
        sizes.add(r1 - r0)
        assert int(yy[k]) == sum(int(v) * int(v) for v in y[r0:r1]) & m, k
    assert len(sizes) == (2 if n % K else 1)
    assert len(set(yy.tolist())) == K and (w == 64 or int(yy.max()) < 1 << 32)   # masked to the width
    h.close()


def test_yy_needs_y_and_its_output(lgc):
    X, _ = _data(np.random.default_rng(3), 12, 3, 64)
    h = lgc.Phase1(X, None, 64, 56)
    with pytest.raises(lgc.LgcError) as e:
        h.local_folds_yy(0, 3, 2)
    assert e.value.code == -1 and "needs y" in str(e.value)
    h.close()
    h = lgc.Phase1(X, X[:, 0].copy(), 64, 56)
    A = np.zeros((2, 6), dtype=np.uint64); b = np.zeros((2, 3), dtype=np.uint64)
    assert lgc.lib().lgc_p1_local_folds_yy(h._h, 0, 3, 2, lgc._vp(A), lgc._vp(b), None) == -1
    with pytest.raises(lgc.LgcError):
        h.local_folds_yy(0, 3, 17)
    h.close()
