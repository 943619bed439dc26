"""An independent model of the lasso solver (include/linreg_gc_lasso.h) in Python integers.

It restates the definition and shares no code with the product: W-bit two's-complement words with p fractional bits,
mul(a, b) = wrap((a b) >> p) with an arithmetic shift, wrapping adds and subtracts, public reals quantised as (int64)(v 2^p).
"""
import math


def wrap(v, w):
    """v mod 2^w as a signed w-bit integer"""
    v &= (1 << w) - 1
    return v - (1 << w) if v >> (w - 1) else v


def mul(a, b, w, p):
    return wrap((a * b) >> p, w)


def to_fixed(v, p, w):
    """(fixed_t)(v * 2^p), truncated, as lambda is quantised"""
    t = v * float(2 ** p)
    if w == 32 and not (-2147483649.0 < t < 2147483648.0):
        return -(1 << 31)
    return wrap(int(t), w)


def coefficients(n, w, p):
    """FISTA's public c_k = (t_k - 1) / t_{k+1}, t_0 = 1, t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2, in IEEE double, quantised"""
    out, t = [], 1.0
    for _ in range(n):
        tn = (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0
        out.append(wrap(int(math.ldexp((t - 1.0) / tn, p)), w))
        t = tn
    return out


def full_matrix(a_packed, d, w):
    """the packed lower triangle (words as uint64 or int) -> d x d symmetric list of signed words"""
    M = [[0] * d for _ in range(d)]
    k = 0
    for i in range(d):
        for j in range(i + 1):
            M[i][j] = M[j][i] = wrap(int(a_packed[k]), w)
            k += 1
    return M


def step_exponent(M, d, w):
    """l = s + bitlen(max_i sum_j (|M_ij| >> s)), s = ceil(log2 d); the magnitudes are unsigned (|INT_MIN| = 2^(w-1))"""
    s = max(0, (d - 1).bit_length())
    m = max(sum(abs(v) >> s for v in row) for row in M)
    assert m < (1 << w)
    return s + m.bit_length()


def step(v, ell, w, p):
    """v 2^(p - l): an arithmetic right shift by l - p, or a left shift by p - l mod 2^w"""
    return v >> (ell - p) if ell >= p else wrap(v << (p - ell), w)


def soft(z, theta, w):
    """z - clamp(z, -theta, theta) for theta >= 0: exact 0 where |z| <= theta; signed compares"""
    nth = wrap(-theta, w)
    if z >= theta:
        return wrap(z - theta, w)
    if z >= nth:
        return 0
    return wrap(z - nth, w)


def lasso(a_packed, b, d, w, p, iters, l1):
    """(beta, trace, ell, theta): beta = x_N, trace[k] = x_{k+1}; a_packed / b: the words every solver sees after the prefix"""
    M = full_matrix(a_packed, d, w)
    b = [wrap(int(v), w) for v in b]
    ell = step_exponent(M, d, w)
    theta = step(to_fixed(l1, p, w), ell, w, p)
    c = coefficients(iters, w, p)
    x, y, trace = [0] * d, [0] * d, []
    for k in range(iters):
        xn, yn = [0] * d, [0] * d
        for i in range(d):
            g = wrap(sum(mul(M[i][j], y[j], w, p) for j in range(d)) - b[i], w)
            z = wrap(y[i] - step(g, ell, w, p), w)
            xn[i] = soft(z, theta, w)
            yn[i] = wrap(xn[i] + mul(wrap(xn[i] - x[i], w), c[k], w, p), w)
        x, y = xn, yn
        trace.append(list(x))
    return x, trace, ell, theta
