"""An independent model of the association scan (include/linreg_gc_scan.h) in Python integers: M candidate
columns, each fitted with the same c shared covariates, in systems of size D = c + 1.

mul, div and sqrt are the semantic oracle's scalar operations (through inference_model.Ops); everything else is written here
from the definition.  All mod 2^w; words are signed w-bit integers.  A share is
  [A (T_c)] [b (c)] [yy (1)] [h_0 (c)] .. [h_{M-1} (c)] [gg (M)] [gy (M)]
  assembly  share sums; normalize = 1: the off-diagonals of A, b, yy, every h_m[k] and every gy_m divided by D (truncating)
            and q(lambda) added to every A_kk and every gg_m; normalize = 0: the words as given
  L, y, E0  the Cholesky factor of the c x c block, the forward substitution of b, E0 = Y - sum_k mul(y_k, y_k)
  u_m[k]    div(h_m[k] - sum_{j<k} mul(L_kj, u_m[j]), L_kk)
  l_m       sqrt(gg_m - sum_k mul(u_m[k], u_m[k]));  t_m = div(gy_m - sum_k mul(u_m[k], y_k), l_m);  beta_m = div(t_m, l_m)
  SE:       z_m = div(2^p, l_m), v_m = mul(z_m, z_m), e_m = E0 - mul(t_m, t_m), s2_m = mulc(e_m, q(resid_scale)),
            w_m = sqrt(mul(s2_m, v_m))
The range condition (every u_m[k], v_m, s2_m and mul(s2_m, v_m) fits in w - 1 - p integer bits, with one bit to spare) is
asserted, so inputs outside it fail here instead of comparing garbage.
"""
import numpy as np

import inference_model as im
import lasso_model as lm

SE = 1


def in_words(c, M):
    return c * (c + 1) // 2 + c + 1 + M * (c + 2)


def assemble(shares, c, M, w, p, lam, normalize):
    """(A full symmetric c x c, b, Y, h (M x c), gg, gy) as the circuit holds them before the solve"""
    D, T = c + 1, c * (c + 1) // 2
    shares = np.asarray(shares, dtype=np.uint64)
    assert shares.shape[1] == in_words(c, M)
    tot = [lm.wrap(sum(int(v) for v in shares[:, i]), w) for i in range(shares.shape[1])]
    ql = lm.to_fixed(lam, p, w) if normalize else 0
    div = (lambda x: im.tdiv(x, D)) if normalize else (lambda x: x)
    A = [[0] * c for _ in range(c)]
    for i in range(c):
        for j in range(i + 1):
            x = tot[i * (i + 1) // 2 + j]
            A[i][j] = A[j][i] = lm.wrap(x + ql, w) if i == j else div(x)
    b = [div(x) for x in tot[T:T + c]]
    Y = div(tot[T + c])
    o = T + c + 1
    h = [[div(x) for x in tot[o + m * c:o + (m + 1) * c]] for m in range(M)]
    gg = [lm.wrap(x + ql, w) for x in tot[o + M * c:o + M * c + M]]
    gy = [div(x) for x in tot[o + M * c + M:o + M * c + 2 * M]]
    return A, b, Y, h, gg, gy


def scan(oracle, shares, c, M, w, p, lam, resid_scale, normalize, se=True):
    """every word of the definition, as signed integers: dict(beta, w, L, y, E0, u, l, t, z, v, e, s2)"""
    ops = im.Ops(oracle, w, p)
    A, b, Y, h, gg, gy = assemble(shares, c, M, w, p, lam, normalize)
    L = [row[:] for row in A]
    for j in range(c):
        for i in range(j, c):
            L[i][j] = ops.wrap(L[i][j] - ops.dot(L[i][:j], L[j][:j]))
        L[j][j] = ops.sqrt(L[j][j])
        for k in range(j + 1, c):
            L[k][j] = ops.div(L[k][j], L[j][j])
    y = [0] * c
    for j in range(c):
        y[j] = ops.div(ops.wrap(b[j] - ops.dot(L[j][:j], y[:j])), L[j][j])
    E0 = ops.wrap(Y - ops.dot(y, y))
    top = 1 << (w - 2)                                    # w - 1 - p integer bits, one to spare
    out = dict(beta=[], w=[], L=L, y=y, E0=E0, u=[], l=[], t=[], z=[], v=[], e=[], s2=[])
    qr = lm.to_fixed(resid_scale, p, w) if se else 0
    for m in range(M):
        u = [0] * c
        for k in range(c):
            u[k] = ops.div(ops.wrap(h[m][k] - ops.dot(L[k][:k], u[:k])), L[k][k])
            assert abs(u[k]) < top, ("range condition: u", m, k)
        l = ops.sqrt(ops.wrap(gg[m] - ops.dot(u, u)))
        assert l > 0, ("the candidate lies in the span of the covariates", m)
        t = ops.div(ops.wrap(gy[m] - ops.dot(u, y)), l)
        out["u"].append(u); out["l"].append(l); out["t"].append(t)
        out["beta"].append(ops.div(t, l))
        if se:
            z = ops.div(1 << p, l)
            v = ops.mul(z, z)
            e = ops.wrap(E0 - ops.mul(t, t))
            s2 = ops.mulc(e, qr)
            sv = ops.mul(s2, v)
            assert 0 < v < top and 0 < s2 < top and 0 < sv < top, ("range condition: v, s2, s2 v", m)
            out["z"].append(z); out["v"].append(v); out["e"].append(e); out["s2"].append(s2)
            out["w"].append(ops.sqrt(sv))
    return out


def revealed(m, se):
    """the words the program reveals, in order: beta_0 .. beta_{M-1}, [w_0 .. w_{M-1}]"""
    return list(m["beta"]) + (list(m["w"]) if se else [])


def augmented_words(tot, c, M, m):
    """the T_D + D words [A, b] of the plain system [C, g_m] (and its yy word behind them) from the words of a scan share"""
    T = c * (c + 1) // 2
    o = T + c + 1
    A = list(tot[:T]) + list(tot[o + m * c:o + (m + 1) * c]) + [tot[o + M * c + m]]
    b = list(tot[T:T + c]) + [tot[o + M * c + M + m]]
    return np.array(A + b + [tot[T + c]], dtype=np.uint64)
