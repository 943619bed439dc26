"""Standard errors, residual variance and R^2 from the Cholesky solve (include/linreg_gc_inference.h) on the CPU: the lowered
program, run record by record by the CPU checker and garbled + evaluated by its CPU backends, against the independent model of
tests/inference_model.py; beta against the existing plain Cholesky program; the model against numpy float64; the structure of
the lowering; the rejections of the library, the binding and bin/linreg.  No GPU needed."""
import math
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import inference_model as im
import test_lasso_select_cpu as sel
from helpers import sx

ROOT = sel.ROOT
SE, FIT = im.SE, im.FIT
SUBSETS = {SE: ("se",), FIT: ("fit",), SE | FIT: ("se", "fit")}
OP_MAC, OP_SUM, OP_MUL, OP_DIV, OP_SQRT, OP_CONST, OP_REVEAL, OP_MAC2, OP_MACK = 1, 2, 7, 13, 14, 16, 18, 19, 20     # gc_exec.h
LAM = 0.001


def data(rng, n, d, sigma=0.4):
    """studentised X (n x d) and y with noise: every column has mean 0 and mean square 1"""
    X = rng.standard_normal((n, d))
    X = (X - X.mean(axis=0)) / X.std(axis=0)
    y = X @ (rng.random(d) / math.sqrt(d)) + sigma * rng.standard_normal(n)
    y = (y - y.mean()) / y.std()
    return X, y


def system_words(X, y, d, w, p, lam, normalize):
    """the T + d + 1 words [A, b, yy] of X^T X / n, X^T y / n, y^T y / n as a share sum holds them.  normalize = 1: the circuit
    divides the off-diagonals, b and yy by d and adds q(lambda), so the diagonal comes divided by d already (phase 1's rule)
    and the rest as it is; normalize = 0: the system as the solver reads it, lambda included"""
    n = X.shape[0]
    G, b, yy = X.T @ X / n, X.T @ y / n, float(y @ y) / n
    q = lambda v: int(v * 2.0 ** p) & ((1 << w) - 1)
    if normalize:
        vals = [G[i, j] / d if i == j else G[i, j] for i in range(d) for j in range(i + 1)] + list(b) + [yy]
    else:
        vals = [G[i, j] + lam if i == j else G[i, j] for i in range(d) for j in range(i + 1)] + list(b) + [yy]
    return np.array([q(v) for v in vals], dtype=np.uint64)


def split(rng, tot, nshares, w):
    """additive shares mod 2^w of a vector of words; the word yy comes from the last share alone (the provider holding y)"""
    m = np.uint64((1 << w) - 1)
    sh = (rng.integers(0, 2 ** 63, size=(nshares, tot.size), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(nshares, tot.size), dtype=np.uint64)) & m
    with np.errstate(over="ignore"):
        sh[0] = (tot - sh[1:].sum(axis=0, dtype=np.uint64)) & m
    sh[:, -1] = 0
    sh[-1, -1] = tot[-1]
    return sh


def case(rng, d, w, p, normalize, n=None, lam=LAM, nshares=2):
    """(shares (nshares, T + d + 1), X, y) of a studentised system with n = 4 d + 40 rows"""
    X, y = data(rng, n or 4 * d + 40, d)
    return split(rng, system_words(X, y, d, w, p, lam, normalize), nshares, w), X, y


def program(lgc, sysm, reveal, resid_scale):
    return lgc.Program(sysm, inference=SUBSETS[reveal], resid_scale=resid_scale)


def shown(prog, dec, w, reveal):
    """the words the program reveals from rv_beta: beta, [u], [s2, r2]"""
    d = prog.system.d
    n = d + (d if reveal & SE else 0) + (2 if reveal & FIT else 0)
    assert prog.info.n_reveal == prog.info.rv_beta + n
    return sx(dec[prog.info.rv_beta:prog.info.rv_beta + n], w).tolist()


def plain_beta(lgc, gccpu, sysm, shares):
    """beta of the EXISTING plain Cholesky program on the same (A, b): the shares without their last word"""
    prog = lgc.Program(sysm)
    d, w = sysm.d, sysm.width
    dec = sel.plain(gccpu, prog, w, sysm.precision, np.ascontiguousarray(shares[:, :-1]))
    return sx(dec[prog.info.rv_beta:prog.info.rv_beta + d], w).tolist()


# ---- the model
@pytest.mark.parametrize("d", [1, 2, 5, 33])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_program_reveals_the_model(lgc, gccpu, oracle, w, p, normalize, d):
    """every revealed word of the lowered program, run record by record on the plaintext backend, is the model's, for each
    reveal subset; beta is the plain cholesky program's on the same (A, b), and the oracle's"""
    rng = np.random.default_rng(zlib.crc32(("inference %d %d %d" % (w, normalize, d)).encode()))
    shares, X, _ = case(rng, d, w, p, normalize, nshares=3)
    rs = X.shape[0] / (X.shape[0] - d)
    sysm = lgc.make_system(d, w, p, "cholesky", 0, LAM, 3, normalize, 0, 0)
    m = im.inference(oracle, shares, d, w, p, LAM, rs, normalize)
    assert any(m["beta"]) and all(v > 0 for v in m["u"]) and m["s2"] > 0 and 0 < m["r2"] < (1 << p)
    assert m["beta"] == plain_beta(lgc, gccpu, sysm, shares)
    for reveal in (SE, FIT, SE | FIT):
        prog = program(lgc, sysm, reveal, rs)
        assert shown(prog, sel.plain(gccpu, prog, w, p, shares), w, reveal) == im.revealed(m, reveal), (d, reveal)


@pytest.mark.parametrize("d,normalize,reveal", [(1, 0, SE | FIT), (1, 1, SE), (2, 1, SE | FIT), (2, 0, FIT), (5, 0, SE | FIT), (5, 1, SE | FIT),
                                                (5, 1, SE), (5, 0, FIT), (33, 1, SE | FIT)])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_cpu_garble_evaluate_gives_the_model(lgc, gccpu, oracle, w, p, d, normalize, reveal):
    """garbled and evaluated on the CPU, launch by launch at the gate steps the lowering assigned"""
    rng = np.random.default_rng(zlib.crc32(("inference ge %d %d %d %d" % (w, normalize, d, reveal)).encode()))
    shares, X, _ = case(rng, d, w, p, normalize)
    rs = X.shape[0] / (X.shape[0] - d)
    sysm = lgc.make_system(d, w, p, "cholesky", 0, LAM, 2, normalize, 0, 0)
    prog = program(lgc, sysm, reveal, rs)
    dec, gates, _ = gccpu.garble_eval(prog, shares)
    assert gates == prog.info.total_gates
    assert shown(prog, dec, w, reveal) == im.revealed(im.inference(oracle, shares, d, w, p, LAM, rs, normalize), reveal)


def test_zero_lambda_has_no_penalty_term_and_inputs_reveal_y(lgc, gccpu, oracle):
    """q(lambda) = 0: no beta^T beta product is lowered and e = Y - b0^T beta; reveal_inputs shows T + d + 1 words, Y last"""
    w, p, d = 64, 56, 4
    rng = np.random.default_rng(11)
    for normalize in (0, 1):
        shares, X, _ = case(rng, d, w, p, normalize, lam=0.0)
        rs = X.shape[0] / (X.shape[0] - d)
        m = im.inference(oracle, shares, d, w, p, 0.0, rs, normalize)
        sysm = lgc.make_system(d, w, p, "cholesky", 0, 0.0, 2, normalize, 1, 0)
        prog, with_lam = program(lgc, sysm, SE | FIT, rs), program(lgc, lgc.make_system(d, w, p, "cholesky", 0, LAM, 2, normalize, 1, 0), SE | FIT, rs)
        assert with_lam.info.n_launches == prog.info.n_launches + 1
        assert (sel._recs(with_lam)[:, 0] == OP_MUL).sum() == (sel._recs(prog)[:, 0] == OP_MUL).sum() + 1
        dec = sel.plain(gccpu, prog, w, p, shares)
        assert shown(prog, dec, w, SE | FIT) == im.revealed(m, SE | FIT)
        T = d * (d + 1) // 2
        assert int(sx(dec[prog.info.rv_inputs + T + d:prog.info.rv_inputs + T + d + 1], w)[0]) == m["Y"]


# ---- the model against float64
REL = {64: 2.0 ** -46, 32: 2.0 ** -16}


def _float_reference(X, y, lam, rs):
    n, d = X.shape
    beta = np.linalg.solve(X.T @ X / n + lam * np.eye(d), X.T @ y / n)
    res = y - X @ beta
    mse = float(res @ res) / n
    s2 = rs * mse
    se = np.sqrt(s2 * np.diag(np.linalg.inv(X.T @ X + n * lam * np.eye(d))))
    return se, s2, 1.0 - mse / (float(y @ y) / n), mse


@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_model_against_float64(oracle, w, p):
    """n = 200, d = 5, lambda in {0, 0.001}, resid_scale = n / (n - d), both input paths, seeded studentised data with noise:
    u_j / sqrt(n), s2 and r2 of the model against numpy float64 on the unquantised data (np.linalg.inv, the residual, R^2),
    every coefficient compared.  Largest relative errors measured on these fixtures: W = 64 / p = 56: 1.7e-15 (u / sqrt(n)),
    2.6e-15 (s2), 1.1e-15 (r2) -- a few ulps of the float64 reference itself; W = 32 / p = 24: 1.1e-6, 2.3e-6, 1.4e-6 -- the
    inputs carry up to 2^-24 = 6e-8 of absolute error each and s2 is a difference of order 0.15 of sums of order 1.  The bound
    per width is 4 x its largest figure, rounded up to a power of two (the margin covers other seeds of the same shape):
    4 x 2.6e-15 -> 2^-46 (1.4e-14) and 4 x 2.3e-6 -> 2^-16 (1.5e-5).  Every range clause holds on these fixtures and e > 0;
    both are asserted"""
    n, d = 200, 5
    rs = n / (n - d)
    worst = {"se": 0.0, "s2": 0.0, "r2": 0.0}
    for lam in (0.0, 0.001):
        for normalize in (0, 1):
            rng = np.random.default_rng(zlib.crc32(("inference float %g %d" % (lam, normalize)).encode()))
            X, y = data(rng, n, d)
            shares = split(rng, system_words(X, y, d, w, p, lam, normalize), 2, w)
            m = im.inference(oracle, shares, d, w, p, lam, rs, normalize)
            f = lambda v: v / 2.0 ** p
            # normalize = 1: the system is the caller's divided by d, and so is s2; lambda counts in those units
            unit = d if normalize else 1
            se, s2, r2, mse = _float_reference(X, y, lam * unit, rs)
            # the range condition, on the float values of what the words hold: w - 1 - p integer bits
            top = 2.0 ** (w - 1 - p)
            Li = np.linalg.inv(np.linalg.cholesky(X.T @ X / n / unit + lam * np.eye(d)))
            assert max(np.abs(Li).max(), (Li ** 2).sum(axis=0).max(), float(y @ y) / n / unit, rs * mse / unit,
                       rs * mse / unit * (Li ** 2).sum(axis=0).max()) < top
            assert all(abs(f(v)) < top / 2 for col in m["z"] for v in col) and all(0 < f(v) < top / 2 for v in m["v"])
            assert 0 < f(m["Y"]) < top / 2 and 0 <= f(m["bb"]) < top / 2 and m["e"] > 0 and mse > 0
            got_se = np.array([f(v) for v in m["u"]]) / math.sqrt(n)
            worst["se"] = max(worst["se"], float(np.abs(got_se / se - 1).max()))
            worst["s2"] = max(worst["s2"], abs(f(m["s2"]) * unit / s2 - 1))
            worst["r2"] = max(worst["r2"], abs(f(m["r2"]) / r2 - 1))
    print("W = %d: largest relative errors %r" % (w, worst))
    assert max(worst.values()) < REL[w], worst


# ---- the structure of the lowering
def _launch_ops(prog):
    r = sel._recs(prog)
    return [(int(r[L["first_rec"], 0]), L["nrec"]) for L in prog.launches()]


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_fit_alone_lowers_no_inverse_column(lgc, w, p, normalize):
    """LGC_INFER_FIT alone: the factorisation's launches are the plain solve's record for record in size (no inverse-column
    record anywhere: every division launch has the plain solve's count, and no word beyond the plain layout is divided), and
    the program is the plain solve's launches plus SIX -- the tail's batch of two dot products (products, merge), e (two
    launches: the penalty term is subtracted in the second), s2 beside div(e, Y), r2 -- or plus FIVE when q(lambda) = 0;
    the reveal launch is the plain solve's with two more records.  With LGC_INFER_SE every division launch of the
    factorisation has d + 1 records and ONE more launch joins the tail: the d square roots (the d products mul(s2, v_j) ride
    beside r2)"""
    d = 7
    for lam, extra in ((LAM, 6), (0.0, 5)):
        sysm = lgc.make_system(d, w, p, "cholesky", 0, lam, 2, normalize, 0, 0)
        progs = lgc.Program(sysm), program(lgc, sysm, FIT, 1.25), program(lgc, sysm, SE | FIT, 1.25)
        plain, fit, full = [_launch_ops(q) for q in progs]
        ndiv = [int((sel._recs(q)[:, 0] == OP_DIV).sum()) for q in progs]
        assert len(fit) == len(plain) + extra and len(full) == len(fit) + 1
        head = len(plain) - 1                             # everything but the reveal
        for k in range(head):
            (op0, n0), (op1, n1) = plain[k], fit[k]
            assert op0 == op1, k
            if op0 in (OP_DIV, OP_MAC, OP_MAC2):
                assert n0 == n1, (k, plain[k], fit[k])    # no record joined a column's batch or division launch
        assert plain[-1] == (OP_REVEAL, d) and fit[-1] == (OP_REVEAL, d + 2) and full[-1] == (OP_REVEAL, 2 * d + 2)
        assert ndiv[1] == ndiv[0] + 1 and ndiv[2] == ndiv[1] + d * (d + 1) // 2     # div(e, Y); the inverse columns' d (d + 1) / 2
        fact_divs = [n for op, n in full[:head] if op == OP_DIV][:d]
        assert fact_divs == [d + 1] * d
        assert [n for op, n in plain[:head] if op == OP_DIV][:d] == [d - j for j in range(d)]


def test_karatsuba_shadow_holds_the_inverse_columns(lgc):
    """d = 184, W = 64 reaches fact_karatsuba: the column batches hold OP_MACK records that read the inverse columns, whose
    half-difference words the division records form (cnt = 2) inside the one shadow: every such store lies inside the word
    file and past the batches' partial sums, behind which the shadow is allocated.  Every multiply-accumulate launch of the
    factorisation past the 4 096-product threshold holds Karatsuba records only, so no plain product reads an inverse column
    there; the small columns and the tail (beta has no half-difference words) keep plain products"""
    d, w, p = 184, 64, 56
    sysm = lgc.make_system(d, w, p, "cholesky", 0, LAM, 2, 1, 0, 0)
    prog = program(lgc, sysm, SE | FIT, 1.25)
    r = sel._recs(prog)
    z_div = r[(r[:, 0] == OP_DIV) & (r[:, 2] == r[:, 3]) & (r[:, 5] == 0)]      # in place, no mirror: step i of an inverse column
    assert len(z_div) == d * (d - 1) // 2 and (z_div[:, 1] == 2).all()
    Z0, Z1 = int(z_div[:, 2].min()) - 1, int(z_div[:, 2].max()) + 1 + d         # the block of inverse columns: z_0[1] is the first word divided in place, z_{d-2}[d-1] the last
    assert Z1 - Z0 == d * d
    mack = r[r[:, 0] == OP_MACK]
    reads_z = mack[(mack[:, 4] >= Z0) & (mack[:, 4] < Z1)]
    assert len(reads_z) > d and len(set(reads_z[:, 5].tolist())) == 1           # one kdelta serves them all
    kdelta = int(reads_z[0, 5])
    assert (z_div[:, 6].astype(np.int64) == kdelta).all()
    fact_end = int(np.nonzero((r[:, 0] == OP_DIV) & (r[:, 2] >= Z0) & (r[:, 2] < Z1))[0][-1])      # the last column's division launch
    fact = [Lc for Lc in prog.launches() if Lc["mac_only"] and Lc["first_rec"] < fact_end]
    plain_reads_z = mack_reads_z = 0
    partial_end = 0
    for Lc in fact:
        q = r[Lc["first_rec"]:Lc["first_rec"] + Lc["nrec"]]
        assert len(set(q[:, 0].tolist())) == 1                                  # a launch is plain or Karatsuba, never both
        z = int(((q[:, 4] >= Z0) & (q[:, 4] < Z1)).sum())
        partial_end = max(partial_end, int(q[:, 2].max()) + 2)
        if q[0, 0] == OP_MACK:
            mack_reads_z += z
        else:
            assert int(q[:, 1].sum()) <= 4096, Lc                               # only a batch below the threshold keeps plain products
            plain_reads_z += z
    assert mack_reads_z > 100 * plain_reads_z > 0                               # (the first columns' few short jobs are plain)
    hd = z_div[:, 2].astype(np.int64) + kdelta                                  # where the z divisions store their half differences
    assert partial_end <= int(hd.min()) and int(hd.max()) < prog.info.n_words
    diag = r[(r[:, 0] == OP_DIV) & (r[:, 2] >= Z0) & (r[:, 2] < Z1) & (r[:, 2] != r[:, 3])]      # z_j[j] = div(2^p, L_jj)
    assert len(diag) == d and (diag[:, 1] == 2).all() and int(diag[:, 2].max()) + kdelta < prog.info.n_words


# ---- rejections and coverage
def test_rejections(lgc):
    d = 4
    chol = lgc.make_system(d, 64, 56, "cholesky", 0, 0.01, 2, 1, 0, 0)
    makers = (lambda s, **k: lgc.Program(s, **k), lambda s, **k: lgc.Solver(s, **k),
              lambda s, **k: lgc.Party(s, lgc.GARBLER, seed=bytes(16), **k))

    def bad(want, s, **k):
        for make in makers:                               # (every check precedes the look for a GPU)
            with pytest.raises(lgc.LgcError) as e:
                make(s, **dict(dict(inference=("se", "fit"), resid_scale=1.25), **k))
            assert e.value.code == -1 and want in str(e.value), str(e.value)

    for alg in ("cgd", "ldlt", "lasso"):
        bad("inference is lowered for algorithm = LGC_ALG_CHOLESKY only", lgc.make_system(d, 64, 56, alg, 3, 0.01, 2, 1, 0, 0))
    bad("trace is not lowered for an inference program", lgc.make_system(d, 64, 56, "cholesky", 0, 0.01, 2, 1, 0, 1))
    for v in (0.0, -1.0, float("nan"), float("inf")):
        bad("resid_scale must be finite and > 0", chol, resid_scale=v)
    bad("precision 56 cannot hold it in a 64-bit word", chol, resid_scale=128.0)
    bad("precision 24 cannot hold it in a 32-bit word", lgc.make_system(d, 32, 24, "cholesky", 0, 0.01, 2, 1, 0, 0), resid_scale=128.0)
    bad("width must be 32 or 64", lgc.make_system(d, 48, 40, "cholesky", 0, 0.01, 2, 1, 0, 0))
    bad("inference too large", lgc.make_system(4096, 64, 56, "cholesky", 0, 0.01, 300, 1, 0, 0))
    bad("inference too large", lgc.make_system(100, 64, 56, "cholesky", 0, 0.01, 1 << 20, 1, 0, 0))
    # the binding
    bad("unknown inference 'r2'", chol, inference=("se", "r2"))
    bad("inference needs resid_scale=", chol, resid_scale=None)
    bad("does not combine with targets", chol, targets=2)
    bad("does not combine with folds, lambdas", chol, lambdas=[0.1, 0.2], folds=2)
    for make in makers:
        with pytest.raises(lgc.LgcError) as e:
            make(chol, resid_scale=1.25)
        assert "resid_scale belongs to inference=" in str(e.value)
    # the library's own check of the reveal bits (the binding never sends a bad word)
    Lb, C = lgc.lib(), lgc.C
    for bits in (0, 4, 7, -1):
        h = C.c_void_p()
        assert Lb.lgc_program_build_inference(C.byref(h), C.byref(chol), 1.25, bits) == -1
        assert "inference reveal flags" in Lb.lgc_last_error().decode()
        assert Lb.lgc_solver_create_inference(C.byref(h), 0, C.byref(chol), bytes(16), 1.25, bits) == -1
        assert Lb.lgc_party_create_inference(C.byref(h), 0, C.byref(chol), lgc.GARBLER, bytes(16), 0, 1.25, bits) == -1
    assert Lb.lgc_program_build_inference(None, C.byref(chol), 1.25, 3) == -1 and "null out" in Lb.lgc_last_error().decode()
    assert Lb.lgc_program_build_inference(C.byref(C.c_void_p()), None, 1.25, 3) == -1 and "null system" in Lb.lgc_last_error().decode()


def test_sizes_and_words(lgc):
    """in_words = T + d + 1 and the revealed word counts, through the binding"""
    for d in (1, 6):
        sysm = lgc.make_system(d, 64, 56, "cholesky", 0, 0.01, 3, 1, 0, 0)
        assert lgc._in_words(sysm, None, infer=True) == d * (d + 1) // 2 + d + 1
        for reveal, names in SUBSETS.items():
            prog = lgc.Program(sysm, inference=names, resid_scale=1.5)
            assert prog.info.n_reveal == d + (d if reveal & SE else 0) + (2 if reveal & FIT else 0)
        assert lgc.Program(sysm, inference="fit", resid_scale=1.5).info.n_reveal == d + 2      # a single name is a subset too
    words = np.arange(1, 15, dtype=np.int64)
    b, u, s2, r2 = lgc._infer_split(words, 6, SE | FIT)
    assert b.tolist() == [1, 2, 3, 4, 5, 6] and u.tolist() == [7, 8, 9, 10, 11, 12] and (s2, r2) == (13, 14)
    b, u, s2, r2 = lgc._infer_split(words, 6, FIT)
    assert u is None and (s2, r2) == (7, 8)
    s = lgc._infer_summary((None, np.array([1 << 55, 1 << 56]), 1 << 54, 1 << 55), 4, lgc.make_system(6, 64, 56, "cholesky", 0, 0.0, 2, 1, 0, 0))
    assert s["std_err"].tolist() == [0.25, 0.5] and s["sigma2"] == 1.5 and s["r2"] == 0.5      # normalize = 1: sigma2 = s2 d
    s = lgc._infer_summary((None, None, 1 << 54, 1 << 55), 4, lgc.make_system(6, 64, 56, "cholesky", 0, 0.0, 2, 0, 0, 0))
    assert s["std_err"] is None and s["sigma2"] == 0.25


def test_header_is_exported_and_documented(lgc):
    hdr = open(os.path.join(ROOT, "include", "linreg_gc_inference.h")).read()
    names = set(re.findall(r"^[a-z][^\n(]*?\b(lgc_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    assert names == {"lgc_program_build_inference", "lgc_solver_create_inference", "lgc_party_create_inference", "lgc_p1_local_yy"}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for nme in names:
        assert hasattr(lgc.lib(), nme), nme
        assert nme in doc, nme
    for word in ("LGC_INFER_SE  1", "LGC_INFER_FIT 2", "T + d + 1", "Range condition", "bit for bit", "sandwich", "variance-inflation"):
        assert word in hdr, word
    assert "linreg_gc_inference.h" in doc and "### 1.15" in doc
    assert "### 2.8" in design and "lgc_program_build_inference" in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--inference" in readme and "inference=(" in readme


# ---- bin/linreg and the wrapper
def _linreg(*args, inp="readme_example.in"):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "linreg-mpc_amd", "host")], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "linreg-mpc_amd", "host", "bin", "linreg")
    return subprocess.run([exe, os.path.join(ROOT, "tests", "golden", inp), "56", "3"] + list(args), capture_output=True, timeout=60)


@pytest.mark.parametrize("args,want", [
    (["cgd", "10", "0.001", "--inference"], b"--inference is for Algorithm cholesky"),
    (["ldlt", "0", "0.001", "--inference"], b"--inference is for Algorithm cholesky"),
    (["lasso", "10", "0.001", "--l1=0.01", "--inference"], b"--inference is for Algorithm cholesky"),
    (["cholesky", "0", "0.001", "--no_se"], b"--no_se belongs to --inference"),
    (["cholesky", "0", "0.001", "--inference", "--lambdas=0.1,0.01"], b"--inference and --lambdas"),
    (["cholesky", "0", "0.001", "--inference", "--lambdas=0.1,0.01", "--folds=2"], b"--inference and --folds"),
    (["cholesky", "0", "0.001", "--inference", "--table_ring", "--devices=0,0"], b"--inference and --devices"),
    (["cholesky", "0", "0.001", "--inference", "--ti_ring"], b"--inference and --ti_ring"),
    (["cholesky", "0", "0.001", "--inference", "--ot_ring"], b"--inference and --ot_ring"),
    (["cholesky", "0", "0.001", "--inference", "--input_ring"], b"--inference and --input_ring"),
])
def test_bin_linreg_rejections(args, want):
    r = _linreg(*args)
    assert r.returncode != 0 and want in r.stdout + r.stderr, (args, r.stdout[-300:], r.stderr[-300:])
    assert b"Party 3 finished phase 1" not in r.stdout


def test_bin_linreg_needs_more_rows_than_columns(tmp_path):
    """resid_scale = n / (n - d): n <= d is refused before any party connects"""
    tok = open(os.path.join(ROOT, "tests", "golden", "readme_example.in")).read().split("\n")
    n, d, P_ = map(int, tok[0].split())
    rows, ys = tok[2 + P_ + 2:2 + P_ + 2 + n], tok[2 + P_ + 2 + n + 1].split()
    k = d                                                 # keep d rows
    path = str(tmp_path / "short.in")
    open(path, "w").write("\n".join(["%d %d %d" % (k, d, P_)] + tok[1:1 + P_ + 2] + ["%d %d" % (k, d)] + rows[:k] + ["%d" % k, " ".join(ys[:k]), ""]))
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "linreg-mpc_amd", "host")], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "linreg-mpc_amd", "host", "bin", "linreg")
    r = subprocess.run([exe, path, "56", "3", "cholesky", "0", "0.001", "--inference"], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"--inference needs more rows than columns" in r.stdout + r.stderr, (r.stdout[-300:], r.stderr[-300:])


def test_wrapper_reads_the_inference_lines():
    import mpc_linear_regression as m
    out = ["Algorithm: cholesky", "Result:    0.250000000000000   -1.500000000000000 ", "Standard errors:    0.031250000000000    0.062500000000000 ",
           "Residual variance: 0.125000000000000 R^2: 0.875000000000000"]
    assert m.parse_inference_lines(out) == ([0.03125, 0.0625], 0.125, 0.875)
    assert m.parse_inference_lines(out[:2] + out[3:]) == (None, 0.125, 0.875)                 # --no_se
    assert m.parse_inference_lines(out[:2]) == (None, None, None)
    assert m.parse_result_line(out[1]) == [0.25, -1.5]                                          # the Result line parses as before
    r = m.MPCLinearRegression("127.0.0.1:1", "127.0.0.1:2", mpc_args=["56", "cholesky", "0", "0.001", "--inference"])
    assert r.mpc_args[-1] == "--inference" and r.std_errors is None and r.sigma2 is None and r.r2 is None
