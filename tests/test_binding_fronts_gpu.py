"""The three fronts of the Python binding agree on every program kind, on the MI355X: the Program, the two Parties and the
Solver made from one request are one program -- launches, AND gates, input bits, fingerprint -- and every word the Solver
reveals through its accessors is, bit for bit, what the CPU checker computes from the Program's records on the same shares.

Each of the twelve kinds at the smallest shape that lowers (d = 3, W = 32, p = 28, two shares; 2 iterations; L = 2, K = 2; a
scan of M = 2 candidates against c = 2 covariates; a sweep of 2 lambdas): an argument in the wrong place of a creation call
shows at any size.  One process, one solver at a time, the table ring of the library's default as in the other GPU tests."""
import numpy as np
import pytest

import test_ridge_cv_cpu as rcv
from helpers import split_shares, sx

pytestmark = pytest.mark.gpu

D, W, P, NSH, ITERS, K, M = 3, 32, 28, 2, 2, 2, 2
T = D * (D + 1) // 2
SEED = bytes(range(7, 23))
LAMS, RATIOS = [0.01, 0.1], [0.5, 0.1]
KINDS = {   # kind -> (algorithm, keywords)
    "": ("cgd", {}),
    "_targets": ("cholesky", dict(targets=2)),
    "_sweep_at": ("cgd", dict(lambdas=LAMS)),
    "_lasso": ("lasso", dict(l1=0.01)),
    "_lasso_path": ("lasso", dict(l1=[0.05, 0.01])),
    "_lasso_opts": ("lasso", dict(l1=0.01, positive=True, penalty_factors=[1.0, 0.5, 2.0])),
    "_lasso_select": ("lasso", dict(l1_ratios=RATIOS, validation=True, reveal_index=True, reveal_scores=True)),
    "_lasso_cv": ("lasso", dict(l1_ratios=RATIOS, folds=K, reveal_index=True, reveal_scores=True)),
    "_lasso_cv_se": ("lasso", dict(l1_ratios=RATIOS, folds=K, rule="1se", reveal_index=True, reveal_curve=True)),
    "_ridge_cv": ("cgd", dict(lambdas=LAMS, folds=K, reveal_index=True, reveal_scores=True)),
    "_inference": ("cholesky", dict(inference=("se", "fit"), resid_scale=1.25)),
    "_scan": ("cholesky", dict(scan=M, scan_se=True, resid_scale=1.25)),
}


def _gram(oracle, rng, cols, n=24):
    """the Gram matrix of [X, y], cols + 1 square, in words: helpers.synth_system's distribution (a well-conditioned system),
    with y as one more column so that (y, y) comes at the scale of the rest"""
    X = rng.standard_normal((n, cols)); X /= np.abs(X).max(axis=0)
    y = X @ rng.random(cols) + 0.1 * rng.standard_normal(n)
    Z = np.hstack([X, (y / np.abs(y).max())[:, None]])
    Zq = oracle.quantize(Z, P, n, W)
    A, _ = oracle.aggregate(Zq, Zq.reshape(n, cols + 1)[:, -1].copy(), n, cols + 1, P, W)
    G = np.zeros((cols + 1, cols + 1), dtype=np.uint64)
    G[np.tril_indices(cols + 1)] = A                                   # (packed lower triangle, row by row)
    return G


def _system_words(G, d, yy=False):
    """[A (T)] [b (d)] [yy] of a Gram matrix whose last column is y"""
    return np.concatenate([G[:d, :d][np.tril_indices(d)], G[-1, :d]] + ([G[-1:, -1]] if yy else []))


def _words(oracle, rng, kind):
    """one share's worth of total input words, in the layout of the kind's header"""
    g = lambda: _gram(oracle, rng, D)
    if kind == "_targets":                                             # (the second target: the y of another draw)
        return np.concatenate([_system_words(g(), D), g()[-1, :D]])
    if kind == "_lasso_select":
        return np.concatenate([_system_words(g(), D), _system_words(g(), D)])
    if kind in ("_lasso_cv", "_ridge_cv", "_lasso_cv_se"):
        folds = [g() for _ in range(K)]
        return np.concatenate([_system_words(G, D) for G in folds] + ([np.array([G[-1, -1] for G in folds])] if kind == "_lasso_cv_se" else []))
    if kind == "_inference":
        return _system_words(g(), D, yy=True)
    if kind == "_scan":                                                # columns c_0 c_1 g_0 g_1 y: [A] [b] [yy] [h_0] [h_1] [gg] [gy]
        c = D - 1
        G = _gram(oracle, rng, c + M)
        return np.concatenate([_system_words(G, c, yy=True)] + [G[c + m, :c] for m in range(M)] + [np.diag(G)[c:c + M], G[-1, c:c + M]])
    return _system_words(g(), D)


def _plain(gccpu, prog, shares):
    """the decode slots of the program run record by record on the CPU checker (test_lasso_cv_cpu.run_plain)"""
    info = prog.info
    words = np.zeros(info.n_words, dtype=np.uint64)
    words[info.in_base:info.in_base + shares.size] = shares.ravel() & np.uint64((1 << W) - 1)
    dec = np.zeros(info.n_reveal + 1, dtype=np.uint64)
    steps, gates = gccpu.plain_run(prog.records(), info.n_records, W, P, words, dec)
    assert steps == info.total_steps and gates == info.total_gates
    return dec


def _accessors(s, kind):
    """every word the solver reveals, through its public accessors, in the order the kind's header gives them"""
    out = np.asarray(s.beta()).ravel().tolist()
    if kind in ("_lasso_select", "_lasso_cv", "_ridge_cv"):            # beta*, l*, the L scores
        out += [s.selected_index()] + s.scores().tolist()
    if kind == "_lasso_cv_se":                                         # beta+, l+, l*, mean (L), se (L)
        mean, se = s.cv_curve()
        assert s.scores() is None
        out += [s.selected_index(), s.min_index()] + mean.tolist() + se.tolist()
    if kind == "_inference":                                           # beta, u (d), s2, r2
        out += s.std_err_words().tolist() + [s.sigma2_word(), s.r2_word()]
    if kind == "_scan":                                                # beta (M), w (M)
        out += s.scan_std_err_words().tolist()
    return out


@pytest.mark.parametrize("kind", list(KINDS))
def test_program_parties_and_solver_are_one_program(lgc, gccpu, oracle, kind):
    alg, kw = KINDS[kind]
    rng = np.random.default_rng(1000 + list(KINDS).index(kind))
    sysm = lgc.make_system(D, W, P, alg, ITERS if alg in ("cgd", "lasso") else 0, 0.01, NSH, 1, 0, 0)
    prog = lgc.Program(sysm, **kw)
    words = _words(oracle, rng, kind)
    in_words = {"": T + D, "_targets": T + 2 * D, "_sweep_at": T + D, "_lasso": T + D, "_lasso_path": T + D, "_lasso_opts": T + D,
                "_lasso_select": 2 * (T + D), "_lasso_cv": K * (T + D), "_lasso_cv_se": K * (T + D) + K, "_ridge_cv": K * (T + D),
                "_inference": T + D + 1, "_scan": 3 + 2 + 1 + M * 4}[kind]
    assert words.size == in_words
    shares = split_shares(rng, words, np.zeros(0, dtype=np.uint64), NSH, W)
    # ---- the two parties (a plain sweep has no party in Python)
    if kind != "_sweep_at":
        G = lgc.Party(sysm, lgc.GARBLER, seed=SEED, **kw)
        E = lgc.Party(sysm, lgc.EVALUATOR, **kw)
        try:
            for party in (G, E):
                assert party.num_launches == prog.info.n_launches and party.and_gates == prog.info.total_gates
                assert party.input_bits == W * in_words                # (lgc_party_input_bits counts one share's inputs)
                assert (party.path, party.folds, party.select, party.rule) == ((prog.path or 1) if prog.select is not None else prog.path,
                                                                               prog.folds, prog.select, prog.rule)
            assert G.program_fingerprint() == E.program_fingerprint()
        finally:
            G.close(); E.close()
    # ---- the solver against the CPU checker on the Program's records
    dec = rcv.run_plain(gccpu, prog, W, P, shares)[0] if kind == "_ridge_cv" else _plain(gccpu, prog, shares)
    info = prog.info
    if kind == "_sweep_at":
        want = [v for t in range(len(LAMS)) for v in sx(dec[info.rv_beta + t * info.reveal_stride:info.rv_beta + t * info.reveal_stride + D], W).tolist()]
    else:
        want = sx(dec[info.rv_beta:info.n_reveal], W).tolist()
    s = lgc.Solver(sysm, seed=SEED, **kw)
    try:
        s.set_shares(shares)
        s.run()
        got = _accessors(s, kind)
        st = s.stats()
        shape = np.asarray(s.beta()).shape
    finally:
        s.close()
    print(kind, got)
    assert got == want and any(got)
    assert shape == {"_targets": (2, D), "_sweep_at": (2, D), "_lasso_path": (2, D), "_scan": (M,)}.get(kind, (D,))
    assert st["and_gates"] == info.total_gates and st["launches"] == info.n_launches
