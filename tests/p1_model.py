"""Plain models of two kernel families of csrc/phase1.hip, independent of the library.

The share arithmetic of the per-pair trusted-initializer protocol (lgc_p1_mask, lgc_p1_dot, lgc_p1_ti_a, lgc_p1_ti_a_batch) in
numpy uint64 wrap-around arithmetic: X is an int64 matrix whose columns are the provider's own (and y behind them), cast to uint64
so that a negative word is its two's complement (at w = 32 the sign extension of the stored word), every vector is a (pairs, n)
array of words below 2^w, and a result is reduced mod 2^w at the end, which commutes with the sums and products mod 2^64.

The floating-point diagonal word of X^T X (p1_diag_kernel; the oracle's diag_share) in Python floats, which are IEEE doubles with
one rounding per operation: k ascending, no fused multiply-add."""
import numpy as np


def _m(w):
    return np.uint64((1 << w) - 1)


def _u(a):
    return np.ascontiguousarray(a).astype(np.uint64)


def mask(X, cols, V, sign, w):
    """out[q][k] = (X[k][cols[q]] + sign * V[q][k]) mod 2^w"""
    x = _u(np.asarray(X, dtype=np.int64)[:, list(cols)].T)
    V = _u(V).reshape(x.shape)
    with np.errstate(over="ignore"):
        return ((x + V) if sign > 0 else (x - V)) & _m(w)


def dot(A, B, sub, w):
    """out[q] = (sum_k A[q][k] * B[q][k] - sub[q]) mod 2^w; B is a vector batch, or columns of X as columns(X, cols)"""
    A = _u(A); B = _u(B).reshape(A.shape)
    with np.errstate(over="ignore"):
        s = (A * B).sum(axis=1, dtype=np.uint64)
        if sub is not None:
            s = s - _u(sub).reshape(s.shape)
        return s & _m(w)


def columns(X, cols):
    """the columns cols[q] of X as the (pairs, n) batch that dot() takes for B"""
    return _u(np.asarray(X, dtype=np.int64)[:, list(cols)].T)


def ti_a(X, cols, y, inn, sub, w):
    """party a of inner_product_ti: ((X[:, cols[q]] - y[q]) mod 2^w, (sum_k inn[q][k] * y[q][k] - sub[q]) mod 2^w)"""
    return mask(X, cols, y, -1, w), dot(inn, y, sub, w)


def saturated(w):
    """the x86 "integer indefinite" word of an out-of-range double -> integer cast"""
    return 1 << (w - 1)


def diag_word(col, p, w, divisor):
    """xy += (x_k / 2^p)^2 * 2^p over the words x_k of `col`, k ascending; the word is (xy / divisor) * 2^p cast to a w-bit
    integer: truncated toward zero and reduced mod 2^w in range, saturated() out of range (and for a NaN)"""
    scale = float(1 << p)
    xy = 0.0
    for x in col:
        v = float(int(x)) / scale
        xy = xy + (v * v) * scale
    t = (xy / float(divisor)) * scale
    if w == 32:
        ok = -2147483649.0 < t < 2147483648.0
    else:
        ok = -9223372036854775808.0 <= t < 9223372036854775808.0
    if not ok:
        return saturated(w)
    return int(t) & ((1 << w) - 1)


def diag_words(X, c0, c1, p, w, divisor):
    """diag_word of the columns [c0, c1) of X"""
    X = np.asarray(X, dtype=np.int64)
    return [diag_word(X[:, c].tolist(), p, w, divisor) for c in range(c0, c1)]
