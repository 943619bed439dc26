"""An independent model of the lasso path (include/linreg_gc_lasso_path.h) in Python integers.

It restates the definition on top of the single-solve model (tests/lasso_model.py) and shares no code with the product.  A
path runs the single solve's FISTA recurrence once per value with its own theta_l; M, b, the step exponent and the FISTA
coefficients are common:
  absolute  theta_l = step(to_fixed(lambda1_l))                      -- exactly the single solve's theta
  ratio     theta_l = step(mul(lambda_max, to_fixed(r_l))), lambda_max = max_i |b_i| (unsigned magnitudes)
Ratios lie in [0, 2]; the range condition gains one clause: 2 lambda_max must fit (so that theta_l >= 0, which soft needs).
"""
import lasso_model as lm

ABSOLUTE, RATIO = 0, 1


def lambda_max(b, w):
    """max_i |b_i| with unsigned magnitudes (|INT_MIN| = 2^(w-1))"""
    return max(abs(lm.wrap(int(v), w)) for v in b)


def thetas(M, b, d, w, p, values, mode):
    """(ell, [theta_l]) of a path"""
    ell = lm.step_exponent(M, d, w)
    if mode == ABSOLUTE:
        return ell, [lm.step(lm.to_fixed(v, p, w), ell, w, p) for v in values]
    lmax = lambda_max(b, w)
    assert 2 * lmax < (1 << (w - 1)), "range condition: 2 lambda_max must fit"
    out = []
    for r in values:
        assert 0.0 <= r <= 2.0
        rf = lm.to_fixed(r, p, w)
        assert rf >= 0, "range condition: the ratio must fit the precision"
        out.append(lm.step(lm.mul(lmax, rf, w, p), ell, w, p))
    return ell, out


def fista(M, b, d, w, p, iters, ell, theta):
    """the single solve's recurrence with a given theta: beta = x_N"""
    c = lm.coefficients(iters, w, p)
    x, y = [0] * d, [0] * d
    for k in range(iters):
        xn, yn = [0] * d, [0] * d
        for i in range(d):
            g = lm.wrap(sum(lm.mul(M[i][j], y[j], w, p) for j in range(d)) - b[i], w)
            z = lm.wrap(y[i] - lm.step(g, ell, w, p), w)
            xn[i] = lm.soft(z, theta, w)
            yn[i] = lm.wrap(xn[i] + lm.mul(lm.wrap(xn[i] - x[i], w), c[k], w, p), w)
        x, y = xn, yn
    return x


def lasso_path(a_packed, b, d, w, p, iters, values, mode):
    """(betas, ell, thetas): betas[l] = x_N of value l; a_packed / b: the words every solver sees after the prefix"""
    M = lm.full_matrix(a_packed, d, w)
    b = [lm.wrap(int(v), w) for v in b]
    ell, th = thetas(M, b, d, w, p, values, mode)
    for t in th:
        assert t >= 0
    return [fista(M, b, d, w, p, iters, ell, t) for t in th], ell, th


def stepexp_ratio(m, lam, r, s, w, p):
    """the OP_STEPEXP record with cnt = 2 on integers: m (unsigned row-sum maximum), lam (the word lambda_max is read from),
    r (the 64-bit immediate), s = ceil(log2 d).  Returns (ell, theta, -theta) as signed w-bit words: theta =
    step(wrap((lam * (r mod 2^w)) >> p)), r read as an unsigned w-bit constant (Circ::mulc)"""
    m &= (1 << w) - 1
    ell = s + m.bit_length()
    prod = lm.wrap((lm.wrap(lam, w) * (r & ((1 << w) - 1))) >> p, w)
    th = lm.step(prod, ell, w, p)
    return ell, th, lm.wrap(-th, w)
