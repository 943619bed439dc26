"""In-circuit K-fold cross-validation of the ridge lambda sweep (include/linreg_gc_ridge_cv.h) on the CPU: the lowered program,
run record by record by the CPU checker and garbled + evaluated by its CPU backends, against the independent model of
tests/ridge_cv_model.py; beta* and the fold fits against the existing single-solve programs; the tie rule; a float64
restatement; the structure of the lowering; the rejections of the library, the binding and bin/linreg.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import lasso_model as lm
import lasso_select_model as lsm
import ridge_cv_model as rcm
import test_lasso_cv_cpu as cvt
import test_lasso_select_cpu as sel
from helpers import sx

ROOT = sel.ROOT
INDEX, SCORES = rcm.REVEAL_INDEX, rcm.REVEAL_SCORES
OP_SUM, OP_MAC, OP_MAC2, OP_IDIVC, OP_REVEAL, OP_MACK, OP_MAX, OP_EQ = 2, 1, 19, 15, sel.OP_REVEAL, sel.OP_MACK, sel.OP_MAX, sel.OP_EQ   # gc_exec.h
STRIDE = 1 << 36                                  # kSweepCircuitStride (gc_program.h)
LAMBDAS = [0.05, 0.001, 0.2, 0.01, 0.5, 0.002, 0.1, 0.02, 0.005]
ITERS = {"cgd": 4, "cholesky": 0, "ldlt": 0}


def circuits(K, L):
    return (K + 1) * L if L > 1 else 1


def program(lgc, sysm, K, lambdas, flags):
    return lgc.Program(sysm, lambdas=list(lambdas), folds=K, reveal_index=bool(flags & INDEX), reveal_scores=bool(flags & SCORES))


def tail_start(prog):
    """index of the first record of the scoring and selection tail: its gate steps begin behind the last circuit's range"""
    st = sel._recs(prog)[:, 8:10].copy().view(np.uint64).ravel()
    at = np.nonzero(st >= prog.info.prefix_steps + STRIDE)[0]
    return int(at[0]) if at.size else len(st)


def run_plain(gccpu, prog, w, p, shares):
    """(decode slots, word file) of the program run record by record, as test_lasso_cv_cpu.run_plain.  The plaintext machine
    counts gate steps from zero without gaps, so the jump to the tail's range is closed in a copy of the records first (the
    plaintext values do not depend on step numbers): the prefix and the circuits run as lowered, then the tail's step0 are
    moved down by the width of the gap"""
    info = prog.info
    rec = sel._recs(prog).copy()
    st = rec[:, 8:10].copy().view(np.uint64).ravel()
    k = tail_start(prog)
    words = np.zeros(info.n_words, dtype=np.uint64)
    words[info.in_base:info.in_base + shares.size] = shares.ravel() & np.uint64((1 << w) - 1)
    dec = np.zeros(info.n_reveal + 1, dtype=np.uint64)
    head, _ = gccpu.plain_run(np.frombuffer(rec[:k].tobytes(), dtype=np.uint8).copy(), k, w, p, words.copy(), dec.copy())
    assert int(st[k]) >= head
    st[k:] -= st[k] - np.uint64(head)
    rec[:, 8:10] = st.view(np.uint32).reshape(-1, 2)
    steps, gates = gccpu.plain_run(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy(), info.n_records, w, p, words, dec)
    assert steps == info.total_steps and gates == info.total_gates
    return dec, words


def case(rng, d, K, w, p, **kw):
    return cvt.fold_shares(rng, cvt.fold_words(rng, d, K, w, p, **kw), 2, w)


# ---- the model
@pytest.mark.parametrize("alg", ["cgd", "cholesky", "ldlt"])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_program_reveals_the_model(lgc, gccpu, oracle, w, p, normalize, alg):
    """every revealed word of the lowered program, run record by record, is the model's: d in {1, 4, 6}, K in {2, 3, 5},
    L in {1, 2, 4, 9} (9: the two-level minimum tree), every reveal combination in turn"""
    n = 0
    for d in (1, 4, 6):
        for K in (2, 3, 5):
            for L in (1, 2, 4, 9):
                rng = np.random.default_rng(zlib.crc32(("ridge cv %d %d %s %d %d %d" % (w, normalize, alg, d, K, L)).encode()))
                shares, per = case(rng, d, K, w, p)
                lams = LAMBDAS[:L]
                sysm = lgc.make_system(d, w, p, alg, ITERS[alg], 0.7, 2, normalize, 0, 0)     # (sys.lambda is ignored)
                best, idx, cv, _, _ = rcm.ridge_cv(oracle, per, d, w, p, alg, ITERS[alg], lams, normalize)
                for flags in ((INDEX | SCORES, 0) if n % 2 else (INDEX, SCORES)):
                    prog = program(lgc, sysm, K, lams, flags)
                    assert sel.shown(prog, run_plain(gccpu, prog, w, p, shares)[0], w, flags, L) == rcm.revealed(best, idx, cv, flags), (d, K, L, flags)
                n += 1


@pytest.mark.parametrize("alg,d,K,L", [("cgd", 4, 3, 4), ("cholesky", 6, 2, 2), ("ldlt", 4, 5, 9), ("cgd", 1, 2, 1)])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_cpu_garble_evaluate_gives_the_model(lgc, gccpu, oracle, w, p, normalize, alg, d, K, L):
    """garbled and evaluated on the CPU, launch by launch at the gate steps the lowering assigned: the circuits' ranges and
    the tail's range behind them under one R"""
    rng = np.random.default_rng(zlib.crc32(("ridge cv ge %d %d %s %d %d %d" % (w, normalize, alg, d, K, L)).encode()))
    shares, per = case(rng, d, K, w, p)
    lams = LAMBDAS[:L]
    N = 2 if alg == "cgd" else 0
    sysm = lgc.make_system(d, w, p, alg, N, 0.0, 2, normalize, 0, 0)
    best, idx, cv, _, _ = rcm.ridge_cv(oracle, per, d, w, p, alg, N, lams, normalize)
    prog = program(lgc, sysm, K, lams, INDEX | SCORES)
    dec, gates, _ = gccpu.garble_eval(prog, shares)
    assert gates == prog.info.total_gates
    assert sel.shown(prog, dec, w, INDEX | SCORES, L) == rcm.revealed(best, idx, cv, INDEX | SCORES)


# ---- independent of the new lowering: the existing single-solve programs
def _single_solve(lgc, gccpu, alg, N, a_packed, b, d, w, p):
    """beta of the EXISTING single-solve program on the normalize = 0 two-share path: share 1 = the system, share 2 = 0"""
    one = lgc.make_system(d, w, p, alg, N, 0.0, 2, 0, 0, 0)
    prog = lgc.Program(one)
    m = (1 << w) - 1
    sh = np.zeros((2, len(a_packed) + d), dtype=np.uint64)
    sh[0] = [int(v) & m for v in list(a_packed) + list(b)]
    dec = cvt.run_plain(gccpu, prog, w, p, sh)[0]
    return sx(dec[prog.info.rv_beta:prog.info.rv_beta + d], w).tolist()


@pytest.mark.parametrize("alg,K", [("cgd", 3), ("cholesky", 2), ("ldlt", 3)])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_refit_and_fold_fits_are_existing_single_solves(lgc, gccpu, w, p, normalize, alg, K):
    """beta* is what the existing single-solve Program reveals on (M_{K,l*}, b_K) assembled by the model; and the revealed
    cv_l, recomputed from the existing Program's fits of the K training systems at l, is the circuit's -- for every l"""
    d, L = 6, 4
    N = ITERS[alg]
    rng = np.random.default_rng(zlib.crc32(("ridge single %d %d %s %d" % (w, normalize, alg, K)).encode()))
    shares, per = case(rng, d, K, w, p)
    lams = LAMBDAS[:L]
    sysm = lgc.make_system(d, w, p, alg, N, 0.0, 2, normalize, 0, 0)
    prog = program(lgc, sysm, K, lams, INDEX | SCORES)
    got = sel.shown(prog, run_plain(gccpu, prog, w, p, shares)[0], w, INDEX | SCORES, L)
    folds, train = rcm.systems(per, d, w, normalize)
    q = [lm.to_fixed(v, p, w) for v in lams]
    idx = got[d]
    assert 0 <= idx < L
    assert got[:d] == _single_solve(lgc, gccpu, alg, N, rcm.with_lambda(train[K][0], d, w, q[idx]), train[K][1], d, w, p) and any(got[:d])
    for l in range(L):
        fits = [_single_solve(lgc, gccpu, alg, N, rcm.with_lambda(train[k][0], d, w, q[l]), train[k][1], d, w, p) for k in range(K)]
        cv = lm.wrap(sum(lsm.score(folds[k][0], folds[k][1], fits[k], d, w, p) for k in range(K)), w)
        assert got[d + 1 + l] == cv, l
    assert idx == lsm.argmin_first(got[d + 1:])
    assert len(set(got[d + 1:])) == L                      # (the values differ, so do their sums)


def test_two_equal_values_select_the_first(lgc, gccpu, oracle):
    """equal lambdas have equal cv words: the selection takes the first of them -- where they are the minimum, behind a heavily
    over-regularised value, and where they are the whole grid"""
    w, p, d, K = 64, 56, 4, 3
    rng = np.random.default_rng(77)
    shares, per = case(rng, d, K, w, p, sigma=0.01)
    sysm = lgc.make_system(d, w, p, "cholesky", 0, 0.0, 2, 1, 0, 0)
    for lams, want in (([50.0, 0.001, 0.001, 0.001], 1), ([0.001, 0.001], 0), ([0.001, 50.0, 0.001], 0)):
        prog = program(lgc, sysm, K, lams, INDEX | SCORES)
        got = sel.shown(prog, run_plain(gccpu, prog, w, p, shares)[0], w, INDEX | SCORES, len(lams))
        cv = got[d + 1:]
        same = [l for l, v in enumerate(lams) if v == 0.001]
        assert len({cv[l] for l in same}) == 1 and min(cv) == cv[same[0]] and len(set(cv)) == len(set(lams))     # the tie is at the minimum
        assert got[d] == want
        assert got == rcm.revealed(*rcm.ridge_cv(oracle, per, d, w, p, "cholesky", 0, lams, 1)[:3], INDEX | SCORES)


# ---- float64 restatement
FLOAT_SEED = 1                                    # chosen on the CPU: see test_float_restatement
FLOAT_MARGIN = 0.05                               # relative gap between the best and the second-best float cv, at least


def _float_case(seed, n, d, K, sigma):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)); X /= np.abs(X).max(axis=0)
    beta = rng.uniform(-1.0, 1.0, d)
    y = X @ beta + sigma * rng.standard_normal(n)
    bounds = [(k * n // K, (k + 1) * n // K) for k in range(K)]      # contiguous row folds
    return [(X[a:b].T @ X[a:b] / (b - a), X[a:b].T @ y[a:b] / (b - a)) for a, b in bounds]


def _float_cv(folds, d, lams):
    """(cv curve, the refits): K-fold ridge cross-validation in float64 numpy on the fold systems, as the circuit forms them"""
    K = len(folds)
    totM, totb = sum(M for M, _ in folds), sum(b for _, b in folds)
    cv, refit = [], []
    for lam in lams:
        fits = [np.linalg.solve((totM - M) / (K - 1) + lam * np.eye(d), (totb - b) / (K - 1)) for M, b in folds]
        cv.append(sum(f @ M @ f - 2.0 * b @ f for f, (M, b) in zip(fits, folds)))
        refit.append(np.linalg.solve(totM / K + lam * np.eye(d), totb / K))
    return np.array(cv), refit


def test_float_restatement(lgc, gccpu, oracle):
    """W = 64, p = 56, cholesky: n = 60 rows of a planted model with noise sigma = 0.5, d = 6, K = 5 contiguous folds, a grid
    from under- to over-regularisation.  The float cv curve of seed FLOAT_SEED has an interior minimum whose relative gap to
    the second-best value exceeds FLOAT_MARGIN (5 %; measured: 11.5 %, against ~1e-15 between the integer and float curves); l* is the float
    arg-min and beta* is numpy's refit to atol = 1e-6, the tolerance tests/test_host.py and tests/test_wrapper.py hold the
    direct solvers to against a float solve"""
    w, p, d, K, n = 64, 56, 6, 5, 60
    lams = [1e-5, 1e-3, 0.01, 0.03, 0.1, 0.3, 1.0, 3.0]
    L = len(lams)
    fl = _float_case(FLOAT_SEED, n, d, K, 0.5)
    m = (1 << w) - 1
    words = [(np.array([int(M[i][j] * 2.0 ** p) & m for i in range(d) for j in range(i + 1)], dtype=np.uint64),
              np.array([int(x * 2.0 ** p) & m for x in b], dtype=np.uint64)) for M, b in fl]
    shares, per = cvt.fold_shares(np.random.default_rng(5), words, 2, w)
    fq = [(np.array(lm.full_matrix(A, d, w), dtype=np.float64) / 2.0 ** p, sx(b, w).astype(np.float64) / 2.0 ** p) for A, b in words]
    cv, refit = _float_cv(fq, d, [float(lm.to_fixed(v, p, w)) / 2.0 ** p for v in lams])
    order = np.sort(cv)
    gap = (order[1] - order[0]) / abs(order[0])
    print("float cv:", cv, "relative gap best / second best: %.4f" % gap)
    assert gap > FLOAT_MARGIN and 0 < int(cv.argmin()) < L - 1
    sysm = lgc.make_system(d, w, p, "cholesky", 0, 0.0, 2, 0, 0, 0)
    prog = program(lgc, sysm, K, lams, INDEX | SCORES)
    got = sel.shown(prog, run_plain(gccpu, prog, w, p, shares)[0], w, INDEX | SCORES, L)
    best, idx, cvm, _, _ = rcm.ridge_cv(oracle, per, d, w, p, "cholesky", 0, lams, 0)
    assert got == rcm.revealed(best, idx, cvm, INDEX | SCORES)
    assert idx == int(cv.argmin())
    assert np.abs(np.array(cvm, dtype=np.float64) / 2.0 ** p - cv).max() < 1e-9
    assert np.allclose(np.array(best, dtype=np.float64) / 2.0 ** p, refit[idx], atol=1e-6)


# ---- structure of the lowering
def _launch_steps(prog):
    return [(Lc["step0"], Lc["step0"] + Lc["steps"]) for Lc in prog.launches()]


@pytest.mark.parametrize("alg", ["cgd", "cholesky"])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_structure_of_the_lowering(lgc, w, p, alg):
    """d = 6.  The prefix -- launches, records and words below shared_end -- does not depend on the values of lambda; the launch
    count is the same for (K, L) = (2, 2) and (3, 4); the launches' gate-step ranges are pairwise disjoint, the merged circuits
    lie inside [prefix, prefix + circuits x 2^36) and the tail begins at its end; the divisions are by d, K - 1 and K; with
    L = 1 nothing is scored"""
    d = 6
    T = d * (d + 1) // 2
    sysm = lgc.make_system(d, w, p, alg, ITERS[alg], 0.0, 2, 1, 0, 0)
    a, b = program(lgc, sysm, 3, [0.1, 0.2, 0.3, 0.4], INDEX), program(lgc, sysm, 3, [0.5, 0.01, 0.7, 0.02], INDEX)
    ia, ib = a.info, b.info
    assert (ia.shared_end, ia.prefix_launches, ia.prefix_steps, ia.n_words) == (ib.shared_end, ib.prefix_launches, ib.prefix_steps, ib.n_words)
    assert ia.shared_end == 1 + 2 * 3 * (T + d) + 3 * (T + d) + 4 * (T + d)     # zero, inputs, folds, differences and tot
    npre = sum(Lc["nrec"] for Lc in a.launches()[:ia.prefix_launches])
    ra, rb = sel._recs(a), sel._recs(b)
    assert ia.prefix_launches == 5 and (ra[:npre] == rb[:npre]).all() and not (ra[npre:] == rb[npre:]).all()
    assert ra[:npre, 2].max() < ia.shared_end and ra[npre:tail_start(a), 2].min() >= ia.shared_end     # what the prefix writes
    small, big = program(lgc, sysm, 2, [0.1, 0.2], INDEX | SCORES), program(lgc, sysm, 3, [0.1, 0.2, 0.3, 0.4], INDEX | SCORES)
    assert small.info.n_launches == big.info.n_launches
    for prog, K, L in ((small, 2, 2), (big, 3, 4)):
        info = prog.info
        spans = [s for s in _launch_steps(prog) if s[1] > s[0]]
        assert all(x[1] <= y[0] for x, y in zip(spans, spans[1:]))                 # in order and disjoint
        r = sel._recs(prog)
        k = tail_start(prog)
        st = r[:, 8:10].copy().view(np.uint64).ravel()
        end = info.prefix_steps + circuits(K, L) * STRIDE
        first_circuit = sum(Lc["nrec"] for Lc in prog.launches()[:info.prefix_launches])
        assert int(st[k]) == end and int(st[k - 1]) < end and int(st[first_circuit]) == info.prefix_steps
        # circuit-major side by side: the lambda constants of the (K + 1) L circuits are one launch of equal records
        first = prog.launches()[info.prefix_launches]
        assert first["nrec"] == circuits(K, L) and len(set(r[first["first_rec"]:first["first_rec"] + first["nrec"], 2].tolist())) == circuits(K, L)
        div = r[r[:, 0] == OP_IDIVC]
        want = {d: K * T, K: T + d}
        if K > 2:
            want[K - 1] = K * (T + d)
        assert {int(c): int((div[:, 5] == c).sum()) for c in set(div[:, 5].tolist())} == want
        # the tail: two batches of plain products (never Karatsuba records), the sums, the minimum, the first match, the select
        tail_ops = r[k:, 0]
        assert (tail_ops == OP_MACK).sum() == 0 and ((tail_ops == OP_MAC) | (tail_ops == OP_MAC2)).sum() >= K * L * (d + 1)
        assert (tail_ops == OP_EQ).sum() == 1 and (tail_ops == OP_MAX).sum() == 1
        assert (tail_ops == OP_REVEAL).sum() == d + 1 + L == info.n_reveal and (r[:k, 0] == OP_REVEAL).sum() == 0
    one = program(lgc, sysm, 3, [0.1], INDEX | SCORES)
    r1 = sel._recs(one)
    k = tail_start(one)
    assert set(r1[k:, 0].tolist()) == {OP_REVEAL} and one.info.n_reveal == d + 2
    assert r1[-1, 3] == 0 and r1[-2, 3] == 0               # l* and cv_0 are read from word 0, the constant zero
    div = r1[r1[:, 0] == OP_IDIVC]
    assert set(div[:, 5].tolist()) == {d, 3} and one.info.n_words < a.info.n_words // 4     # only the full system is assembled and fitted
    assert lgc.Program(sysm, lambdas=[0.1, 0.2]).info.replicas == 2        # (the plain sweep is what it was)


def test_programs_differ_with_every_public_parameter(lgc):
    d = 4
    sysm = lgc.make_system(d, 64, 56, "cgd", 3, 0.0, 2, 1, 0, 0)
    chol = lgc.make_system(d, 64, 56, "cholesky", 0, 0.0, 2, 1, 0, 0)
    progs = [program(lgc, sysm, 2, [0.1, 0.2], 0), program(lgc, sysm, 3, [0.1, 0.2], 0), program(lgc, sysm, 2, [0.1, 0.3], 0),
             program(lgc, sysm, 2, [0.1, 0.2], INDEX), program(lgc, chol, 2, [0.1, 0.2], 0), program(lgc, sysm, 2, [0.1, 0.2, 0.3], 0)]
    assert len({zlib.crc32(pr.records().tobytes()) for pr in progs}) == len(progs)


# ---- rejections and the interface
def test_rejections(lgc):
    d = 4
    sysm = lgc.make_system(d, 64, 56, "cgd", 5, 0.01, 2, 1, 0, 0)
    lasso = lgc.make_system(d, 64, 56, "lasso", 5, 0.01, 2, 1, 0, 0)
    Lb = lgc.lib()
    makers = (lambda s, **k: lgc.Program(s, **k), lambda s, **k: lgc.Solver(s, **k),
              lambda s, **k: lgc.Party(s, lgc.GARBLER, seed=bytes(16), **k))

    def bad(want, s, **k):
        for make in makers:                               # (every check precedes the look for a GPU)
            with pytest.raises(lgc.LgcError) as e:
                make(s, **dict(dict(lambdas=[0.1, 0.2], folds=3), **k))
            assert e.value.code == -1 and want in str(e.value), str(e.value)

    for K in (0, 1, 17, 1000):
        bad("a ridge cross-validation takes 2..16 folds", sysm, folds=K)
    bad("takes 1..256 values of lambda", sysm, lambdas=[])
    bad("takes 1..256 values of lambda", sysm, lambdas=[0.1] * 257)
    bad("ridge lambda 1 must be finite and >= 0", sysm, lambdas=[0.1, -0.2])
    bad("ridge lambda 0 must be finite and >= 0", sysm, lambdas=[float("nan"), 0.2])
    bad("ridge lambda 2 must be finite and >= 0", sysm, lambdas=[0.1, 0.2, float("inf")])
    bad("trace reveals every iterate: it is not for a ridge cross-validation", lgc.make_system(d, 64, 56, "cgd", 5, 0.01, 2, 1, 0, 1))
    bad("reveal_inputs is not lowered for a ridge cross-validation", lgc.make_system(d, 64, 56, "cgd", 5, 0.01, 2, 1, 1, 0))
    bad("the dimension check is not cross-validated", lgc.make_system(1, 64, 56, "dimcheck", 0, 0.0, 2, 0, 0, 0))
    bad("width must be 32 or 64", lgc.make_system(d, 48, 40, "cgd", 5, 0.01, 2, 1, 0, 0))
    bad("ridge cross-validation too large", lgc.make_system(100, 64, 56, "cgd", 5, 0.01, 1 << 20, 1, 0, 0), folds=16)
    bad("ridge cross-validation too large", lgc.make_system(4096, 64, 56, "cgd", 5, 0.01, 2, 1, 0, 0), lambdas=[0.1] * 256, folds=16)
    # the binding: what is new, and what stays as it was -- messages included
    bad("a lasso system takes l1 or l1_ratios with folds", lasso)
    bad("exclude each other", sysm, validation=True)
    bad("rule and reveal_curve belong to the cross-validation of a lasso path", sysm, rule="1se")
    for make in makers[:2]:
        with pytest.raises(lgc.LgcError) as e:
            make(sysm, lambdas=[0.1, 0.2], folds=3, first=1)
        assert "first must be 0" in str(e.value)
        with pytest.raises(lgc.LgcError) as e:
            make(lasso, folds=3)
        assert "needs l1 or l1_ratios" in str(e.value)
        with pytest.raises(lgc.LgcError) as e:
            make(sysm, folds=3)
        assert "needs l1 or l1_ratios" in str(e.value)
    for make in makers:
        with pytest.raises(lgc.LgcError) as e:
            make(lasso, lambdas=[0.1, 0.2], l1=[0.1], folds=3)
        assert "l1 (lasso) cannot be combined with a lambda sweep or with targets" in str(e.value)
        with pytest.raises(lgc.LgcError) as e:
            make(sysm, lambdas=[0.1, 0.2], targets=2, folds=3)
        assert "targets cannot be combined with a lambda sweep" in str(e.value)
        with pytest.raises(lgc.LgcError) as e:
            make(lasso, l1=[0.1], validation=True, folds=3)
        assert "exclude each other" in str(e.value)
    with pytest.raises(lgc.LgcError) as e:
        lgc.Party(sysm, lgc.GARBLER, seed=bytes(16), lambdas=[0.1, 0.2])
    assert "only with folds=K" in str(e.value)
    # the C calls: the lasso algorithm, unknown flag bits, null lambdas
    vals = (C.c_double * 2)(0.1, 0.2)
    out = C.c_void_p()
    assert Lb.lgc_program_build_ridge_cv(C.byref(out), C.byref(lasso), 2, vals, 3, 0) == -1
    assert b"a lasso path is cross-validated by the calls of linreg_gc_lasso_cv.h" in Lb.lgc_last_error()
    for flags in (4, 8 | 1, -1):
        assert Lb.lgc_program_build_ridge_cv(C.byref(out), C.byref(sysm), 2, vals, 3, flags) == -1
        assert b"unknown ridge reveal flags" in Lb.lgc_last_error()
    assert Lb.lgc_program_build_ridge_cv(C.byref(out), C.byref(sysm), 2, None, 3, 0) == -1 and b"null lambdas" in Lb.lgc_last_error()
    assert Lb.lgc_program_build_ridge_cv(C.byref(out), None, 2, vals, 3, 0) == -1 and b"null system" in Lb.lgc_last_error()
    assert Lb.lgc_program_build_ridge_cv(C.byref(out), C.byref(sysm), 2, vals, 16, 3) == 0
    Lb.lgc_program_destroy(out)


def test_header_is_exported_and_documented(lgc):
    hdr = open(os.path.join(ROOT, "include", "linreg_gc_ridge_cv.h")).read()
    names = set(re.findall(r"^[a-z][^\n(]*?\b(lgc_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    assert names == {"lgc_program_build_ridge_cv", "lgc_solver_create_ridge_cv", "lgc_party_create_ridge_cv"}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for nme in names:
        assert hasattr(lgc.lib(), nme), nme
        assert nme in doc, nme
    for word in ("LGC_MAX_RIDGE_CV_VALUES 256", "K (T + d)", "lgc_p1_", "BOTH", "Range condition", "bit for bit"):
        assert word in hdr, word
    assert "linreg_gc_ridge_cv.h" in doc and "### 1.14" in doc
    assert "2.7" in design and "lgc_program_build_ridge_cv" in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--lambdas=" in readme and "--folds=" in readme and "lambdas=[" in readme


# ---- bin/linreg and the wrapper
def _linreg(*args):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "linreg-mpc_amd", "host")], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "linreg-mpc_amd", "host", "bin", "linreg")
    inp = os.path.join(ROOT, "tests", "golden", "readme_example.in")             # n = 10, d = 5
    return subprocess.run([exe, inp, "56", "3"] + list(args), capture_output=True, timeout=60)


GRID = "--lambdas=0.1,0.01,0.001"


@pytest.mark.parametrize("args,want", [
    # new: every check precedes device use
    (["cgd", "10", "0.001", GRID, "--folds=1"], b"--folds wants 2..16"),
    (["cholesky", "10", "0.001", GRID, "--folds=17"], b"--folds wants 2..16"),
    (["ldlt", "10", "0.001", GRID, "--folds=11"], b"--folds=11: more folds than the 10 rows"),
    (["cgd", "10", "0.001", GRID, "--folds=2", "--ti_ring"], b"--folds and --ti_ring"),
    (["cgd", "10", "0.001", GRID, "--folds=2", "--ot_ring"], b"--folds and --ot_ring"),
    (["cgd", "10", "0.001", GRID, "--folds=2", "--input_ring"], b"--folds and --input_ring"),
    (["cgd", "10", "0.001", GRID, "--folds=2", "--table_ring", "--devices=0,0"], b"--folds and --devices"),
    (["cgd", "10", "0.001", GRID, "--folds=2", "--one_se"], b"--one_se and --reveal_curve are for the cross-validation of a lasso path"),
    (["cgd", "10", "0.001", GRID, "--folds=2", "--reveal_curve"], b"--one_se and --reveal_curve are for the cross-validation of a lasso path"),
    (["cgd", "10", "0.001", "--lambdas=" + ",".join(["0.1"] * 257), "--folds=2"], b"--folds cross-validates at most 256 values"),
    (["cgd", "10", "0.001", GRID, "--reveal_index"], b"--reveal_index belongs to --folds"),
    # kept, verbatim
    (["cgd", "10", "0.001", "--folds=2"], b"--folds is for Algorithm lasso"),
    (["cholesky", "10", "0.001", "--folds=2", "--reveal_index"], b"--folds is for Algorithm lasso"),
    (["lasso", "10", "0.001", "--l1_ratios=1,0.5,0.1", "--folds=2", GRID], b"--folds and --lambdas exclude each other"),
])
def test_bin_linreg_rejections(args, want):
    r = _linreg(*args)
    assert r.returncode != 0 and want in r.stdout + r.stderr, (args, r.stdout[-300:], r.stderr[-300:])
    assert b"Party 3 finished phase 1" not in r.stdout


def test_wrapper_reads_the_selected_line():
    import mpc_linear_regression as m
    out = ["Folds: 2", "Selected index: 2 (lambda: 0.001)", "Result:    0.250000000000000   -1.500000000000000 "]
    assert m.parse_selected_line(out) == (2, 0.001)
    assert m.parse_selected_line(["Selected index: 1 (L1 ratio: 0.5)"]) == (1, 0.5)          # its existing inputs parse as before
    assert m.parse_selected_line(["Selected index: 3 (L1: 0.002)"]) == (3, 0.002)
    assert m.parse_selected_line(["Selected index: 3 (mu: 0.002)"]) is None and m.parse_selected_line(out[2:]) is None
    r = m.MPCLinearRegression("127.0.0.1:1", "127.0.0.1:2", mpc_args=["56", "cgd", "10", "0.001", GRID, "--folds=2", "--reveal_index"])
    assert r.mpc_args[-3:] == [GRID, "--folds=2", "--reveal_index"] and r.selected is None
