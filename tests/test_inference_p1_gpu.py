"""lgc_p1_local_yy (include/linreg_gc_inference.h) on the MI355X: out_A and out_b are lgc_p1_local's word for word, out_yy is
sum y_q^2 in Python integers mod 2^w and the sum of lgc_p1_local_folds_yy's K words.  Inputs are full-range words (sign-extended
from 32 bits at w = 32), so every sum wraps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# n, d, c0, c1, K: rows that are no multiple of the 16-row slab, own = 3 of 5 columns, three folds (12 / 12 / 13 rows); one row
# and one column; two tile rows (own + 1 = 66 columns: the entry (y, y) lies in the second diagonal tile) and 1030 rows in splits
SHAPES = [(37, 5, 1, 4, 3), (1, 1, 0, 1, None), (1030, 70, 2, 67, 2)]


def _data(rng, n, d, w):
    lo, hi = (-2 ** 63, 2 ** 63) if w == 64 else (-2 ** 31, 2 ** 31)
    return rng.integers(lo, hi, (n, d), dtype=np.int64, endpoint=False), rng.integers(lo, hi, n, dtype=np.int64, endpoint=False)


@pytest.mark.parametrize("w,p", [(64, 56), (32, 28)])
@pytest.mark.parametrize("n,d,c0,c1,K", SHAPES)
def test_local_yy_is_local_plus_the_gram_entry(lgc, n, d, c0, c1, K, w, p):
    rng = np.random.default_rng([n, d, w])
    X, y = _data(rng, n, d, w)
    m = (1 << w) - 1
    h = lgc.Phase1(X, y, w, p)
    rA, rb = h.local(c0, c1, with_y=True)
    A, b, yy = h.local_yy(c0, c1)
    assert A.tolist() == rA.tolist() and b.tolist() == rb.tolist()               # word for word, the floating-point diagonal included
    assert int(yy) == sum(int(v) * int(v) for v in y) & m
    again = h.local(c0, c1, with_y=True)                                         # the older call is what it was, after the new one too
    assert again[0].tolist() == rA.tolist() and again[1].tolist() == rb.tolist()
    if K:
        fA, fb, fyy = h.local_folds_yy(c0, c1, K)
        assert sum(int(v) for v in fyy) & m == int(yy)
        assert [sum(int(fb[k][i]) for k in range(K)) & m for i in range(c1 - c0)] == [int(v) for v in b]
    h.close()


def test_local_yy_rejections(lgc):
    rng = np.random.default_rng(5)
    X, y = _data(rng, 9, 3, 64)
    no_y = lgc.Phase1(X, None, 64, 56)
    with pytest.raises(lgc.LgcError) as e:
        no_y.local_yy(0, 3)
    assert e.value.code == -1 and "the object has none" in str(e.value)
    no_y.close()
    h = lgc.Phase1(X, y, 64, 56)
    with pytest.raises(lgc.LgcError) as e:
        h.local_yy(2, 2)
    assert "bad column range" in str(e.value)
    A = np.zeros(6, dtype=np.uint64); b = np.zeros(3, dtype=np.uint64)
    assert lgc.lib().lgc_p1_local_yy(h._h, 0, 3, lgc._vp(A), lgc._vp(b), None) == -1
    h.close()
