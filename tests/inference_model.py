"""An independent model of the inference on the Cholesky solve (include/linreg_gc_inference.h) in Python
integers: standard errors, the residual variance and R^2.

mul, div and sqrt are the semantic oracle's scalar operations (oracle/liblinreg_oracle.so, a restatement of the reference);
the input assembly is the oracle's (sum_shares, circuit_input).  Everything else is written here from the definition.  All
mod 2^w; words are signed w-bit integers:
  M, b      share sums; normalize = 1: off-diagonals and b divided by d (truncating), q(lambda) added to the diagonal
  Y         the share sum of yy; normalize = 1: tdiv(Y, d)
  b0        b before the solve
  L, beta   Cholesky (cholesky.oc:51-93): column by column, forward and back substitution
  z_j       column j of L^-1: z_j[i] = 0 (i < j), z_j[j] = div(2^p, L_jj), z_j[i] = div(0 - sum_{k=j}^{i-1} mul(L_ik, z_j[k]), L_ii)
  v_j       sum_{i>=j} mul(z_j[i], z_j[i])
  e         Y - sum_i mul(b0_i, beta_i) - mulc(sum_i mul(beta_i, beta_i), q(lambda))     (no last term when q(lambda) = 0)
  s2        mulc(e, q(resid_scale));   u_j = sqrt(mul(s2, v_j));   r2 = 2^p - div(e, Y)
mulc(x, c) = wrap((x c) >> p) for the public constant c >= 0.
"""
import numpy as np

import lasso_model as lm

SE, FIT = 1, 2


def tdiv(x, c):
    """truncation toward zero by the public c >= 1"""
    q = abs(x) // c
    return -q if x < 0 else q


class Ops:
    def __init__(self, oracle, w, p):
        self.o, self.w, self.p = oracle, w, p

    def wrap(self, v):
        return lm.wrap(int(v), self.w)

    def mul(self, a, b):
        return int(self.o.mul(int(a), int(b), self.p, self.w))

    def div(self, a, b):
        return int(self.o.div(int(a), int(b), self.p, self.w))

    def sqrt(self, a):
        return int(self.o.sqrt(int(a), self.p, self.w))

    def mulc(self, a, c):
        assert c >= 0
        return self.wrap((int(a) * int(c)) >> self.p)

    def dot(self, xs, ys):
        return self.wrap(sum(self.mul(x, y) for x, y in zip(xs, ys)))


def assemble(oracle, shares, d, w, p, lam, normalize):
    """(M full symmetric, b, Y) as the circuit holds them before the solve; shares: (nshares, T + d + 1) words"""
    T = d * (d + 1) // 2
    shares = np.asarray(shares, dtype=np.uint64)
    a = oracle.sum_shares(shares[:, :T], w)
    b = oracle.sum_shares(shares[:, T:T + d], w)
    Y = lm.wrap(sum(int(v) for v in shares[:, T + d]), w)
    if normalize:
        a, b = oracle.circuit_input(a, b, d, lam, p, w)
        Y = tdiv(Y, d)
    return lm.full_matrix([int(v) for v in a], d, w), [int(v) for v in b], Y


def cholesky(ops, M, b, d):
    """(L lower triangular, beta) by the reference's three loops"""
    L = [row[:] for row in M]
    for j in range(d):
        for i in range(j, d):
            L[i][j] = ops.wrap(L[i][j] - ops.dot(L[i][:j], L[j][:j]))
        L[j][j] = ops.sqrt(L[j][j])
        for k in range(j + 1, d):
            L[k][j] = ops.div(L[k][j], L[j][j])
    y = [0] * d
    for j in range(d):
        y[j] = ops.div(ops.wrap(b[j] - ops.dot(L[j][:j], y[:j])), L[j][j])
    beta = [0] * d
    for i in reversed(range(d)):
        beta[i] = ops.div(ops.wrap(y[i] - ops.dot([L[k][i] for k in range(i + 1, d)], beta[i + 1:])), L[i][i])
    return L, beta


def inverse_columns(ops, L, d):
    """z[j][i] = (L^-1)_ij"""
    z = [[0] * d for _ in range(d)]
    for j in range(d):
        z[j][j] = ops.div(1 << ops.p, L[j][j])
        for i in range(j + 1, d):
            z[j][i] = ops.div(ops.wrap(0 - ops.dot(L[i][j:i], z[j][j:i])), L[i][i])
    return z


def inference(oracle, shares, d, w, p, lam, resid_scale, normalize):
    """every word of the definition, as signed integers: dict(beta, L, z, v, Y, e, s2, u, r2)"""
    ops = Ops(oracle, w, p)
    M, b, Y = assemble(oracle, shares, d, w, p, lam, normalize)
    b0 = b[:]
    L, beta = cholesky(ops, M, b, d)
    z = inverse_columns(ops, L, d)
    v = [ops.dot(z[j][j:], z[j][j:]) for j in range(d)]
    ql, qr = lm.to_fixed(lam, p, w), lm.to_fixed(resid_scale, p, w)
    e = ops.wrap(Y - ops.dot(b0, beta))
    if ql:
        e = ops.wrap(e - ops.mulc(ops.dot(beta, beta), ql))
    s2 = ops.mulc(e, qr)
    u = [ops.sqrt(ops.mul(s2, vj)) for vj in v]
    r2 = ops.wrap((1 << p) - ops.div(e, Y))
    return dict(beta=beta, L=L, z=z, v=v, Y=Y, bb=ops.dot(beta, beta), e=e, s2=s2, u=u, r2=r2)


def revealed(m, reveal):
    """the words the program reveals, in order: beta, [u], [s2, r2]"""
    return list(m["beta"]) + (list(m["u"]) if reveal & SE else []) + ([m["s2"], m["r2"]] if reveal & FIT else [])

