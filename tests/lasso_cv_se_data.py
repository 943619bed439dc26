"""Inputs for the tests of the one-standard-error rule (tests/test_lasso_cv_se_cpu.py, tests/test_lasso_cv_se_gpu.py): K folds
of rows of one planted model with their y^T y, shared additively, and the pinned cases both suites run."""
import zlib

import numpy as np

import lasso_cv_se_model as sem
from helpers import split_shares

# L values each, out of order so that pi is not the identity; ratios of lambda_max lie in [0, 2]
VALUES = {sem.ABSOLUTE: {3: [0.002, 0.05, 0.01], 9: [0.3, 0.05, 0.0005, 0.01, 0.1, 0.002, 0.02, 0.2, 0.005], 1: [0.01]},
          sem.RATIO: {3: [0.1, 1.0, 0.5], 9: [1.5, 0.5, 0.01, 0.1, 0.8, 0.03, 0.2, 1.0, 0.05], 1: [0.3]}}


def fold_words(rng, d, K, w, p, rows, sigma, density=0.6):
    """[(A_k, b_k, yy_k)] as words: A_k = X_k^T X_k / (n_k d) packed as the lower triangle row by row, b_k = X_k^T y_k / (n_k d),
    yy_k = y_k^T y_k / (n_k d): the three blocks of one Gram matrix over (X, y), in one scale"""
    beta = rng.random(d) * (rng.random(d) < density)
    m = (1 << w) - 1
    out = []
    for _ in range(K):
        X = rng.standard_normal((rows, d)); X /= np.abs(X).max(axis=0)
        y = X @ beta + sigma * rng.standard_normal(rows)
        M, v, yy = X.T @ X / (rows * d), X.T @ y / (rows * d), float(y @ y) / (rows * d)
        out.append((np.array([int(M[i][j] * 2.0 ** p) & m for i in range(d) for j in range(i + 1)], dtype=np.uint64),
                    np.array([int(x * 2.0 ** p) & m for x in v], dtype=np.uint64), int(yy * 2.0 ** p) & m))
    return out


def shares_of(rng, folds, nshares, w):
    """(shares (nshares, K (T + d) + K), [the (nshares, T + d) rows of fold k], the (nshares, K) rows of yy): the last share alone
    holds yy, as the provider that owns y does"""
    per = [split_shares(rng, A, b, nshares, w) for A, b, _ in folds]
    yy = np.zeros((nshares, len(folds)), dtype=np.uint64)
    yy[-1] = [v for _, _, v in folds]
    return np.ascontiguousarray(np.hstack(per + [yy])), per, yy


class Case:
    """one system and request: .shares, .per, .yy, .values, .kw (penalty factors and bounds) and model(N, rule)"""

    def __init__(self, w, p, normalize, mode, d, K, L, rows=None, sigma=0.3, seed=0, lam=0.05, kw=None, nshares=2):
        self.w, self.p, self.normalize, self.mode, self.d, self.K, self.L, self.lam = w, p, normalize, mode, d, K, L, lam
        rng = np.random.default_rng(zlib.crc32(("cv se %d %d %d %d %d %d %d" % (w, normalize, mode, d, K, L, seed)).encode()))
        self.folds = fold_words(rng, d, K, w, p, rows or 2 * d + 6, sigma)
        self.shares, self.per, self.yy = shares_of(rng, self.folds, nshares, w)
        self.values = VALUES[mode][L]
        self.kw = kw or {}
        self._models = {}

    def model(self, N, rule=sem.RULE_ONE_SE):
        if (N, rule) not in self._models:
            self._models[(N, rule)] = sem.lasso_cv_se(self.per, self.yy, self.d, self.w, self.p, N, self.values, self.mode, self.normalize,
                                                      self.lam, rule, self.kw.get("penalty_factors"), self.kw.get("lower"),
                                                      self.kw.get("upper"))
        return self._models[(N, rule)]

    def system(self, lgc, N):
        return lgc.make_system(self.d, self.w, self.p, "lasso", N, self.lam, self.shares.shape[0], self.normalize, 0, 0)

    def request(self, flags, rule="1se"):
        """the keyword arguments of linreg_gc.Program / Solver / Party"""
        key = "l1" if self.mode == sem.ABSOLUTE else "l1_ratios"
        return dict(self.kw, folds=self.K, rule=rule, reveal_index=bool(flags & sem.REVEAL_INDEX),
                    reveal_scores=bool(flags & sem.REVEAL_SCORES), reveal_curve=bool(flags & sem.REVEAL_CURVE), **{key: list(self.values)})
