"""Penalty factors and bounds of the lasso (include/linreg_gc_lasso_opts.h) on the CPU: the lowered program, run record by record
by the CPU checker and garbled + evaluated by its CPU backends, against the independent model of tests/lasso_bounds_model.py;
the defaults against today's programs; the structure and the cost of a bounded record; convergence against float64
projected FISTA, NNLS and sklearn's positive lasso; the rejections, bin/linreg's options and the header.  No GPU needed."""
import math
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import lasso_bounds_model as lbm
import lasso_model as lm
import linreg_gc
from helpers import split_shares, sx, synth_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OP_CONST, OP_STEPEXP, OP_PROX = 16, 25, 26          # gc_exec.h
INF = math.inf
FACTORS = [1.0, 0.0, 0.5, 2.0, 1.5, 0.25]


def _recs(prog):
    return np.frombuffer(prog.records().tobytes(), dtype=np.uint32).reshape(-1, 10)


def _inputs(oracle, A, b, d, w, p, lam, normalize):
    a = oracle.sum_shares(np.asarray(A, dtype=np.uint64)[None, :], w)
    bb = oracle.sum_shares(np.asarray(b, dtype=np.uint64)[None, :], w)
    if normalize:
        a, bb = oracle.circuit_input(a, bb, d, lam, p, w)
    return sx(a, w).tolist(), sx(bb, w).tolist()


def _plain(gccpu, prog, w, p, shares):
    info = prog.info
    words = np.zeros(info.n_words, dtype=np.uint64)
    words[info.in_base:info.in_base + shares.size] = shares.ravel() & np.uint64((1 << w) - 1)
    dec = np.zeros(info.n_reveal + 1, dtype=np.uint64)
    steps, gates = gccpu.plain_run(prog.records(), info.n_records, w, p, words, dec)
    assert steps == info.total_steps and gates == info.total_gates
    return dec


def _beta(prog, dec, w, rows):
    info, d = prog.info, prog.system.d
    return sx(dec[info.rv_beta:info.rv_beta + rows * d], w).reshape(rows, d).tolist()


def _case(oracle, rng, d, w, p, scale=1):
    A, b = synth_system(oracle, rng, 3 * d + 20, d, w, p)
    with np.errstate(over="ignore"):
        return A * np.uint64(scale), b * np.uint64(scale)


def _options(d, scale=1.0):
    """factors including 0, and per coordinate: no bound, lower only, upper only, both sides, lo = hi, lower 0"""
    kinds = [(-INF, INF), (0.0, INF), (-INF, 0.05), (-0.02, 0.03), (0.01, 0.01), (-0.3, 0.0)]
    lower = [kinds[i % 6][0] * scale for i in range(d)]
    upper = [kinds[i % 6][1] * scale for i in range(d)]
    return [FACTORS[(i + 1) % len(FACTORS)] for i in range(d)], lower, upper


def _inside(beta, lower, upper, w, p):
    lo, hi, _ = lbm.bound_words(lower, upper, len(lower), w, p)
    return all(lo[i] <= v <= hi[i] for row in beta for i, v in enumerate(row))


@pytest.mark.parametrize("d", [1, 5, 17])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 28)])
def test_bounded_program_reveals_the_model(lgc, gccpu, oracle, w, p, normalize, d):
    """beta of the lowered program with factors and bounds, run record by record, is the model's, and lies in the bounds;
    scale 8 on the two-party path makes the step a right shift (l > p)"""
    for scale in ((1, 8) if normalize == 0 else (1,)):
        rng = np.random.default_rng(zlib.crc32(("bounds %d %d %d %d" % (w, normalize, d, scale)).encode()))
        N, lam, l1 = 7, 0.05, 0.003
        A, b = _case(oracle, rng, d, w, p, scale)
        shares = split_shares(rng, A, b, 2, w)
        f, lo, hi = _options(d, scale)
        if d == 1:
            f, lo, hi = [0.5], [-0.01 * scale], [0.02 * scale]
        prog = lgc.Program(lgc.make_system(d, w, p, "lasso", N, lam, 2, normalize, 0, 0), l1=l1, penalty_factors=f, lower=lo,
                           upper=hi)
        got = _beta(prog, _plain(gccpu, prog, w, p, shares), w, 1)
        a, bb = _inputs(oracle, A, b, d, w, p, lam, normalize)
        betas, ell, _ = lbm.lasso_opts(a, bb, d, w, p, N, [l1], lbm.ABSOLUTE, f, lo, hi)
        assert got == betas
        assert _inside(got, lo, hi, w, p)
        assert (ell > p) == (scale > 1 and d > 1) or d == 1
        if d == 17 and scale == 1:
            assert any(got[0][i] in (lbm.bound_words(lo, hi, d, w, p)[0][i], lbm.bound_words(lo, hi, d, w, p)[1][i])
                       for i in range(d) if lbm.bound_words(lo, hi, d, w, p)[2][i])      # some bound is active


@pytest.mark.parametrize("d", [1, 5])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 28)])
def test_cpu_garble_evaluate_gives_the_model(lgc, gccpu, oracle, w, p, d):
    rng = np.random.default_rng(zlib.crc32(("bounds ge %d %d" % (w, d)).encode()))
    N, lam, l1 = 4, 0.05, 0.003
    A, b = _case(oracle, rng, d, w, p)
    shares = split_shares(rng, A, b, 2, w)
    f, lo, hi = _options(d)
    prog = lgc.Program(lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0), l1=l1, penalty_factors=f, lower=lo, upper=hi)
    dec, gates, _ = gccpu.garble_eval(prog, shares)
    assert gates == prog.info.total_gates
    a, bb = _inputs(oracle, A, b, d, w, p, lam, 1)
    assert _beta(prog, dec, w, 1) == lbm.lasso_opts(a, bb, d, w, p, N, [l1], lbm.ABSOLUTE, f, lo, hi)[0]


def test_karatsuba_size_matches_the_model(lgc, gccpu, oracle):
    """d = 96 at w = 64: the products run through OP_MACK on the hdiff(y) words that bounded OP_PROX records form"""
    rng = np.random.default_rng(961)
    w, p, d, N, lam, l1 = 64, 56, 96, 3, 0.01, 0.0005
    A, b = _case(oracle, rng, d, w, p)
    shares = split_shares(rng, A, b, 2, w)
    f, lo, hi = _options(d)
    prog = lgc.Program(lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0), l1=l1, penalty_factors=f, lower=lo, upper=hi)
    recs = _recs(prog)
    prox = recs[recs[:, 0] == OP_PROX]
    assert (recs[:, 0] == 20).any() and (prox[:, 7] != 0).all() and (prox[:, 1] >> 31).any() and not (prox[:, 1] >> 31).all()
    got = _beta(prog, _plain(gccpu, prog, w, p, shares), w, 1)
    a, bb = _inputs(oracle, A, b, d, w, p, lam, 1)
    assert got == lbm.lasso_opts(a, bb, d, w, p, N, [l1], lbm.ABSOLUTE, f, lo, hi)[0]


@pytest.mark.parametrize("mode", [lbm.ABSOLUTE, lbm.RATIO])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 28)])
def test_path_with_options_matches_the_model(lgc, gccpu, oracle, w, p, mode):
    """a path of three values in either mode: one group per distinct (value, factor, bounds), every beta_l the model's"""
    d, N, lam = 6, 6, 0.05
    rng = np.random.default_rng(zlib.crc32(("bounds path %d %d" % (w, mode)).encode()))
    A, b = _case(oracle, rng, d, w, p)
    shares = split_shares(rng, A, b, 2, w)
    f, lo, hi = _options(d)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0)
    values = [0.0005, 0.002, 0.006] if mode == lbm.ABSOLUTE else [0.05, 0.2, 0.5]
    kw = dict(penalty_factors=f, lower=lo, upper=hi)
    prog = lgc.Program(sysm, l1=values, **kw) if mode == lbm.ABSOLUTE else lgc.Program(sysm, l1_ratios=values, **kw)
    a, bb = _inputs(oracle, A, b, d, w, p, lam, 1)
    betas, _, th = lbm.lasso_opts(a, bb, d, w, p, N, values, mode, f, lo, hi)
    assert _beta(prog, _plain(gccpu, prog, w, p, shares), w, 3) == betas
    assert len({t for row in th for t in row}) > 3
    # one OP_STEPEXP per distinct (l, q(v w_i), lo_i, hi_i)
    lw, hw, bx = lbm.bound_words(lo, hi, d, w, p)
    groups = {(l, lm.to_fixed(v * f[i], p, w), lw[i] if bx[i] else 0, hw[i] if bx[i] else 0, bx[i])
              for l, v in enumerate(values) for i in range(d)}
    assert (_recs(prog)[:, 0] == OP_STEPEXP).sum() == len(groups)
    if w == 64:
        dec, gates, _ = gccpu.garble_eval(prog, shares)
        assert gates == prog.info.total_gates and _beta(prog, dec, w, 3) == betas


@pytest.mark.parametrize("w,p", [(64, 56), (32, 28)])
def test_bounds_at_the_extreme_words(lgc, gccpu, oracle, w, p):
    """a lower bound at the most negative word, an upper bound one ulp-of-double below the top, one-sided bounds whose
    missing side is the extreme word, and lo = hi = 0 (the coordinate is pinned to 0)"""
    d, N, lam, l1 = 5, 5, 0.05, 0.002
    rng = np.random.default_rng(zlib.crc32(("extreme %d" % w).encode()))
    A, b = _case(oracle, rng, d, w, p)
    shares = split_shares(rng, A, b, 2, w)
    top = 2.0 ** (w - 1 - p)
    lo = [-top, -INF, 0.0, -top, 0.0]
    hi = [math.nextafter(top, 0), 0.01, INF, INF, 0.0]
    prog = lgc.Program(lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0), l1=l1, lower=lo, upper=hi)
    lw, hw, _ = lbm.bound_words(lo, hi, d, w, p)
    assert lw[0] == -(1 << (w - 1)) and hw[0] >= (1 << (w - 1)) - (1 << 11)
    consts = {int(r[3]) | int(r[4]) << 32 for r in _recs(prog) if r[0] == OP_CONST}
    assert {lw[0] & wm_mask(w), (1 << (w - 1)) - 1, 1 << (w - 1)} <= consts
    got = _beta(prog, _plain(gccpu, prog, w, p, shares), w, 1)
    a, bb = _inputs(oracle, A, b, d, w, p, lam, 1)
    assert got == lbm.lasso_opts(a, bb, d, w, p, N, [l1], lbm.ABSOLUTE, None, lo, hi)[0]
    assert got[0][4] == 0 and got[0][2] >= 0 and got[0][1] <= lm.to_fixed(0.01, p, w)


def wm_mask(w):
    return (1 << w) - 1


@pytest.mark.parametrize("d,w,p", [(5, 64, 56), (100, 64, 56), (17, 32, 28)])
def test_defaults_are_todays_program(lgc, d, w, p):
    """every factor 1 and every bound infinite, through the new calls: the records, launches and every lgc_program_info field
    of lgc.Program(sysm, l1=...) and of the path"""
    fields = [f for f, _ in lgc.ProgramInfo._fields_]
    for normalize in (0, 1):
        sysm = lgc.make_system(d, w, p, "lasso", 4, 0.01, 2, normalize, 0, 0)
        kw = dict(penalty_factors=[1.0] * d, lower=[-INF] * d, upper=[INF] * d)
        for a, b in ((lgc.Program(sysm, l1=0.003), lgc.Program(sysm, l1=0.003, **kw)),
                     (lgc.Program(sysm, l1=0.003), lgc.Program(sysm, l1=0.003, upper=[INF] * d)),
                     (lgc.Program(sysm, l1=[0.001, 0.003]), lgc.Program(sysm, l1=[0.001, 0.003], **kw)),
                     (lgc.Program(sysm, l1_ratios=[0.2, 0.5]), lgc.Program(sysm, l1_ratios=[0.2, 0.5], **kw))):
            assert a.records().tobytes() == b.records().tobytes()
            assert a.launches() == b.launches()
            assert [getattr(a.info, f) for f in fields] == [getattr(b.info, f) for f in fields]


def test_structure_and_cost_at_d100(lgc):
    """d = 100, N = 15, every coordinate boxed: the launches of the unbounded program, N launches of d OP_PROX records each,
    all flagged; the bounds enter as OP_CONST records only"""
    d, N = 100, 15
    sysm = lgc.make_system(d, 64, 56, "lasso", N, 0.001, 2, 1, 0, 0)
    one = lgc.Program(sysm, l1=0.001)
    box = lgc.Program(sysm, l1=0.001, lower=[-0.5] * d, upper=[0.5] * d)
    r1, rb = _recs(one), _recs(box)
    assert box.info.n_launches == one.info.n_launches
    def prox_sizes(prog, ops):
        return [Lc["nrec"] for Lc in prog.launches() if (ops[Lc["first_rec"]:Lc["first_rec"] + Lc["nrec"]] == OP_PROX).any()]
    assert prox_sizes(box, rb[:, 0]) == prox_sizes(one, r1[:, 0]) == [d] * N
    assert (rb[rb[:, 0] == OP_PROX, 1] >> 31).all() and not (r1[r1[:, 0] == OP_PROX, 1] >> 31).any()
    assert (rb[:, 0] == OP_CONST).sum() == (r1[:, 0] == OP_CONST).sum() + 2
    assert (rb[:, 0] == OP_STEPEXP).sum() == 1
    extra = box.info.total_gates - one.info.total_gates
    assert extra == N * d * 898, extra


@pytest.mark.parametrize("w,p,gates", [(64, 56, (6218, 7116)), (32, 28, (2633, 3019))])
def test_flagged_record_cost(w, p, gates):
    """a bounded OP_PROX record costs two w-bit compares and the selection more than an unbounded one (pinned)"""
    c = 0x0123456789abcdef & ((1 << p) - 1)
    def cost(flag):
        rec = (OP_PROX, (c >> 32) | flag, 10, 12, c & 0xFFFFFFFF, 1, 0, 2)
        return linreg_gc.RecordProgram(w, p, [rec], [1], n_inputs=0, n_words=20).info.total_gates
    assert (cost(0), cost(lbm.BOUNDED)) == gates


def _planted(oracle, rng, w, p, d, n, beta_true, noise=0.01):
    X = rng.standard_normal((n, d)); X /= np.abs(X).max(axis=0)
    y = X @ beta_true + noise * rng.standard_normal(n)
    return X, y, oracle.aggregate(oracle.quantize(X, p, n, w), oracle.quantize(y, p, n, w), n, d, p, w)


def _projected_fista(a, bb, d, p, ell, theta, lo, hi, c):
    """float64 projected FISTA with the circuit's step 2^(p - l), per-coordinate thresholds and bounds, its quantised c_k"""
    M = np.array(lm.full_matrix(a, d, 64), dtype=float) / 2.0 ** p
    b = np.array(bb, dtype=float) / 2.0 ** p
    alpha = 2.0 ** (p - ell)
    x = np.zeros(d); y = np.zeros(d); z = np.zeros(d)
    for ck in c:
        z = y - alpha * (M @ y - b)
        xn = np.clip(np.sign(z) * np.maximum(np.abs(z) - theta, 0.0), lo, hi)
        y = xn + (ck / 2.0 ** p) * (xn - x)
        x = xn
    return x


def test_converges_towards_projected_fista(lgc, gccpu, oracle):
    """a planted model with signs the bounds cut off: beta agrees with float64 projected FISTA (same step, same c_k) within
    1e-9, bounds active on several coordinates, an unpenalised coordinate non-zero"""
    rng = np.random.default_rng(4242)
    w, p, d, n, N, lam, l1 = 64, 56, 10, 400, 60, 0.01, 0.001
    bt = np.array([0.9, -0.7, 0.5, -0.4, 0.3, 0.0, 0.05, -0.05, 0.2, 0.0])
    _, _, (A, b) = _planted(oracle, rng, w, p, d, n, bt)
    shares = split_shares(rng, A, b, 2, w)
    f = [1.0, 1.0, 1.0, 1.0, 0.5, 2.0, 0.0, 1.0, 1.0, 1.0]
    lo = [0.0, 0.0, -INF, -0.01, -INF, -INF, -INF, -INF, 0.0, -INF]
    hi = [0.1, INF, INF, INF, 0.01, INF, INF, INF, INF, INF]
    prog = lgc.Program(lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0), l1=l1, penalty_factors=f, lower=lo, upper=hi)
    got = np.array(_beta(prog, _plain(gccpu, prog, w, p, shares), w, 1)[0]) / 2.0 ** p
    a, bb = _inputs(oracle, A, b, d, w, p, lam, 1)
    ell = lm.step_exponent(lm.full_matrix(a, d, w), d, w)
    theta = np.array([l1 * fi for fi in f]) * 2.0 ** (p - ell)
    x = _projected_fista(a, bb, d, p, ell, theta, np.array(lo), np.array(hi), lm.coefficients(N, w, p))
    assert np.abs(got - x).max() < 1e-9, (got, x)
    lw, hw, bx = lbm.bound_words(lo, hi, d, w, p)
    active = [i for i in range(d) if bx[i] and got[i] * 2.0 ** p in (lw[i], hw[i])]
    assert len(active) >= 3, (got, active)
    assert got[6] != 0                                   # unpenalised


def test_nnls_near_scipy(lgc, gccpu, oracle):
    """lambda1 = 0, positive, a small lambda2, large n, small d: non-negative least squares, near scipy.optimize.nnls"""
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(31)
    w, p, d, n, N, lam = 64, 56, 5, 2000, 400, 1e-6
    bt = np.array([0.8, -0.5, 0.3, -0.2, 0.6])
    X, y, (A, b) = _planted(oracle, rng, w, p, d, n, bt)
    shares = split_shares(rng, A, b, 2, w)
    prog = lgc.Program(lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0), l1=0.0, positive=True)
    got = np.array(_beta(prog, _plain(gccpu, prog, w, p, shares), w, 1)[0]) / 2.0 ** p
    ref, _ = opt.nnls(X, y)
    assert (got >= 0).all() and (got[[1, 3]] == 0).all()
    assert np.abs(got - ref).max() < 1e-3, (got, ref)


def test_positive_lasso_near_sklearn(lgc, gccpu, oracle):
    """positive lasso against sklearn's Lasso(positive=True) on the same data (its objective 1/(2n) |y - X beta|^2 +
    alpha |beta|_1 is ours with lambda1 = alpha and lambda2 -> 0)"""
    lin = pytest.importorskip("sklearn.linear_model")
    rng = np.random.default_rng(57)
    w, p, d, n, N, lam, l1 = 64, 56, 6, 1000, 400, 1e-6, 0.01
    bt = np.array([0.7, -0.6, 0.4, 0.0, 0.3, -0.1])
    X, y, (A, b) = _planted(oracle, rng, w, p, d, n, bt)
    shares = split_shares(rng, A, b, 2, w)
    prog = lgc.Program(lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0), l1=l1, positive=True)
    got = np.array(_beta(prog, _plain(gccpu, prog, w, p, shares), w, 1)[0]) / 2.0 ** p
    # the circuit's M is s X^T X / n + lambda2 I and its b is s X^T y / n for the scale s of the input path: alpha = l1 / s
    a, _ = _inputs(oracle, A, b, d, w, p, lam, 1)
    s = (a[0] / 2.0 ** p - lam) / (X[:, 0] @ X[:, 0] / n)
    ref = lin.Lasso(alpha=l1 / s, positive=True, fit_intercept=False, tol=1e-12, max_iter=100000).fit(X, y).coef_
    assert (got >= 0).all() and ((got == 0) == (ref == 0)).all(), (got, ref)
    assert np.abs(got - ref).max() < 1e-3, (got, ref)


# ---- rejections, bin/linreg, the header
def test_rejections(lgc):
    import ctypes as C
    d = 4
    sysm = lgc.make_system(d, 64, 56, "lasso", 5, 0.01, 2, 1, 0, 0)
    L = lgc.lib()

    def bad(want, *a, **k):
        with pytest.raises(lgc.LgcError) as e:
            lgc.Program(*a, **k)
        assert e.value.code == -1 and want in str(e.value), str(e.value)

    for v in (-0.5, INF, math.nan):
        bad("penalty factor 2 must be finite and >= 0", sysm, l1=0.1, penalty_factors=[1, 1, v, 1])
    bad("bound 1 is NaN", sysm, l1=0.1, lower=[0, math.nan, 0, 0])
    bad("bound 3 is NaN", sysm, l1=0.1, upper=[1, 1, 1, math.nan])
    bad("above its upper bound", sysm, l1=0.1, lower=[0, 0.5, 0, 0], upper=[1, 0.4, 1, 1])
    bad("no value lies in them", sysm, l1=0.1, lower=[0, INF, 0, 0])
    bad("no value lies in them", sysm, l1=0.1, upper=[0, -INF, 0, 0])
    bad("bound 0 is 256: precision 56", sysm, l1=0.1, upper=[256.0, INF, INF, INF])
    bad("bound 0 is -256.5", sysm, l1=0.1, lower=[-256.5, 0, 0, 0])
    bad("lambda1 0 times penalty factor 1", sysm, l1=100.0, penalty_factors=[1, 3, 1, 1])
    bad("lambda1 ratio 1 times penalty factor 2", sysm, l1_ratios=[0.5, 2.0], penalty_factors=[1, 1, 64, 1])
    bad("LGC_ALG_LASSO", lgc.make_system(d, 64, 56, "cgd", 5, 0.01, 2, 1, 0, 0), l1=0.1, positive=True)
    bad("exclude", sysm, l1=0.1, positive=True, lower=[0] * d)
    bad("need l1", lgc.make_system(d, 64, 56, "cgd", 5, 0.01, 2, 1, 0, 0), positive=True)
    bad("need l1", sysm, targets=2, upper=[1] * d)
    bad("sweep", sysm, l1=0.1, lambdas=[0.1, 0.2], positive=True)
    bad("targets", sysm, l1=0.1, targets=2, positive=True)
    bad("d = 4 entries", sysm, l1=0.1, lower=[0] * 3)
    bad("[0, 2]", sysm, l1_ratios=[2.5], positive=True)                  # a path's own checks come first
    # 32 bits, p = 28: 3 integer bits; a bound of 8 does not fit, -8 does
    s32 = lgc.make_system(d, 32, 28, "lasso", 5, 0.01, 2, 1, 0, 0)
    bad("precision 28", s32, l1=0.1, upper=[8.0, INF, INF, INF])
    lgc.Program(s32, l1=0.1, lower=[-8.0, 0, 0, 0]).close()
    lgc.Program(s32, l1=0.1, penalty_factors=[0, 0, 0, 0]).close()
    # the C calls: a null opts
    out = C.c_void_p()
    assert L.lgc_program_build_lasso_opts(C.byref(out), C.byref(sysm), None) == -1 and b"null opts" in L.lgc_last_error()
    # (refused before a GPU is looked for)
    with pytest.raises(lgc.LgcError) as e:
        lgc.Solver(sysm, l1=0.1, penalty_factors=[-1, 1, 1, 1])
    assert "penalty factor 0" in str(e.value)
    with pytest.raises(lgc.LgcError) as e:
        lgc.Party(sysm, lgc.GARBLER, seed=bytes(16), l1=0.1, lower=[1, 0, 0, 0], upper=[0, 1, 1, 1])
    assert "above its upper bound" in str(e.value)


def _linreg(*args):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "linreg-mpc_amd", "host")], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "linreg-mpc_amd", "host", "bin", "linreg")
    inp = os.path.join(ROOT, "tests", "golden", "readme_example.in")
    return subprocess.run([exe, inp, "56", "3"] + list(args), capture_output=True, timeout=60)


def test_bin_linreg_options():
    """the options need lasso, lists are numbers with d (= 5 in the example) entries, --positive excludes --lower"""
    for args, want in ((["cgd", "10", "0.001", "--positive"], b"--positive is for Algorithm lasso"),
                       (["cholesky", "10", "0.001", "--upper=1,1,1,1,1"], b"--upper is for Algorithm lasso"),
                       (["cgd", "10", "0.001", "--penalty_factors=1,1,1,1,1"], b"--penalty_factors is for Algorithm lasso"),
                       (["lasso", "10", "0.001", "--l1=0.1", "--positive", "--lower=0,0,0,0,0"], b"exclude"),
                       (["lasso", "10", "0.001", "--l1=0.1", "--lower=0,x,0,0,0"], b"--lower wants"),
                       (["lasso", "10", "0.001", "--l1=0.1", "--upper=1,1,1"], b"--upper wants d = 5 entries"),
                       (["lasso", "10", "0.001", "--l1=0.1", "--penalty_factors=1,1,1,1,1,1"], b"--penalty_factors wants d = 5")):
        r = _linreg(*args)
        assert r.returncode != 0 and want in r.stdout + r.stderr, (args, r.stdout[-300:], r.stderr[-300:])


def test_lasso_opts_header_is_exported_and_documented(lgc):
    hdr = open(os.path.join(ROOT, "include", "linreg_gc_lasso_opts.h")).read()
    names = set(re.findall(r"^[a-z][^\n(]*?\b(lgc_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    assert names == {"lgc_program_build_lasso_opts", "lgc_solver_create_lasso_opts", "lgc_party_create_lasso_opts"}
    for field in ("l1_count", "l1_mode", "penalty_factors", "lower", "upper"):
        assert re.search(r"\b%s;" % field, hdr), field
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for nme in names:
        assert hasattr(lgc.lib(), nme), nme
        assert nme in doc, nme
    assert "linreg_gc_lasso_opts.h" in doc and "penalty factor" in design and "clamp" in design
    assert "--positive" in open(os.path.join(ROOT, "README.md")).read()
    assert len(re.findall(r"^\s*(?:int|size_t|void|const char \*|uint64_t|double)\s+\**lgc_\w+\s*\(",
                          open(os.path.join(ROOT, "include", "linreg_gc.h")).read(), flags=re.M)) <= 70
