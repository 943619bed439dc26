"""The association scan (include/linreg_gc_scan.h) on the CPU: the lowered program, run record by record by the CPU checker and
garbled + evaluated by its CPU backends, against the independent model of tests/scan_model.py; every coefficient against the
EXISTING plain Cholesky program on the augmented system [C, g_m]; the scan words against the existing inference program; the
model against numpy float64; the structure of the lowering; the rejections of the library, the binding and bin/linreg.  No GPU
needed."""
import math
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import inference_model as im
import scan_model as sm
import test_inference_cpu as ti
import test_lasso_select_cpu as sel
from helpers import sx

ROOT = sel.ROOT
OP_MAC, OP_SUM, OP_MUL, OP_DIV, OP_SQRT, OP_CONST, OP_REVEAL, OP_MAC2, OP_MACK = 1, 2, 7, 13, 14, 16, 18, 19, 20     # gc_exec.h
LAM = 0.001
WIDTHS = [(64, 56), (32, 24)]


def total_words(X, y, c, M, w, p, lam, normalize):
    """the words of a scan share as a share sum holds them, from X = [C (c), G (M)] and y: Gram entries over n.  normalize = 1:
    the circuit divides everything but the diagonals by D = c + 1 and adds q(lambda), so the diagonals (A_kk, gg_m) come divided
    by D already (phase 1's rule) and the rest as it is; normalize = 0: the system as the solver reads it, lambda included"""
    n, D = X.shape[0], c + 1
    G = X.T @ X / n
    b = X.T @ y / n
    yy = float(y @ y) / n
    q = lambda v: int(v * 2.0 ** p) & ((1 << w) - 1)
    dg = (lambda v: v / D) if normalize else (lambda v: v + lam)
    vals = [dg(G[i, i]) if i == j else G[i, j] for i in range(c) for j in range(i + 1)] + list(b[:c]) + [yy]
    vals += [G[c + m, k] for m in range(M) for k in range(c)] + [dg(G[c + m, c + m]) for m in range(M)] + [b[c + m] for m in range(M)]
    return np.array([q(v) for v in vals], dtype=np.uint64)


def split(rng, tot, nshares, w):
    """additive shares mod 2^w of a vector of words"""
    m = np.uint64((1 << w) - 1)
    sh = (rng.integers(0, 2 ** 63, size=(nshares, tot.size), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(nshares, tot.size), dtype=np.uint64)) & m
    with np.errstate(over="ignore"):
        sh[0] = (tot - sh[1:].sum(axis=0, dtype=np.uint64)) & m
    return sh


def case(rng, c, M, w, p, normalize, lam=LAM, nshares=3, n=None):
    """(shares, total words, X, y): independent studentised columns and y with noise, n = 4 D + 40 rows"""
    X, y = ti.data(rng, n or 4 * (c + 1) + 40, c + M)
    tot = total_words(X, y, c, M, w, p, lam, normalize)
    return split(rng, tot, nshares, w), tot, X, y


def program(lgc, sysm, M, se, rs):
    return lgc.Program(sysm, scan=M, scan_se=bool(se), resid_scale=rs if se else None)


def shown(prog, dec, w, M, se):
    n = M * (2 if se else 1)
    assert prog.info.n_reveal == prog.info.rv_beta + n
    return sx(dec[prog.info.rv_beta:prog.info.rv_beta + n], w).tolist()


def resid(X, c):
    return X.shape[0] / (X.shape[0] - (c + 1))


# ---- the model
@pytest.mark.parametrize("M", [1, 3, 40])
@pytest.mark.parametrize("c", [1, 2, 5])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", WIDTHS)
def test_program_reveals_the_model(lgc, gccpu, oracle, w, p, normalize, c, M):
    """every revealed word of the lowered program, run record by record on the plaintext backend, is the model's, with and
    without the standard errors, nshares = 3"""
    rng = np.random.default_rng(zlib.crc32(("scan %d %d %d %d" % (w, normalize, c, M)).encode()))
    shares, _, X, _ = case(rng, c, M, w, p, normalize)
    rs = resid(X, c)
    sysm = lgc.make_system(c + 1, w, p, "cholesky", 0, LAM, 3, normalize, 0, 0)
    m = sm.scan(oracle, shares, c, M, w, p, LAM, rs, normalize)
    assert any(m["beta"]) and all(v > 0 for v in m["w"])
    for se in (0, 1):
        prog = program(lgc, sysm, M, se, rs)
        assert shown(prog, sel.plain(gccpu, prog, w, p, shares), w, M, se) == sm.revealed(m, se), (c, M, se)


@pytest.mark.parametrize("c,M", [(1, 1), (2, 3), (5, 40)])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", WIDTHS)
def test_beta_is_the_plain_solve_of_the_augmented_system(lgc, gccpu, oracle, w, p, normalize, c, M):
    """beta_m is bit for bit the last coefficient the EXISTING plain Cholesky program reveals on [C, g_m]: the D-system's words
    are taken from the same share sums and run through lgc.Program(system) as it has always been"""
    rng = np.random.default_rng(zlib.crc32(("scan plain %d %d %d %d" % (w, normalize, c, M)).encode()))
    shares, tot, X, _ = case(rng, c, M, w, p, normalize)
    D = c + 1
    sysm = lgc.make_system(D, w, p, "cholesky", 0, LAM, 3, normalize, 0, 0)
    prog = program(lgc, sysm, M, 0, None)
    got = shown(prog, sel.plain(gccpu, prog, w, p, shares), w, M, 0)
    plain = lgc.Program(sysm)
    for m in range(M):
        aug = split(rng, sm.augmented_words(tot, c, M, m)[:-1], 3, w)
        dec = sel.plain(gccpu, plain, w, p, aug)
        assert int(sx(dec[plain.info.rv_beta + D - 1:plain.info.rv_beta + D], w)[0]) == got[m], m


@pytest.mark.parametrize("c,M,normalize,se", [(1, 1, 0, 1), (1, 1, 1, 0), (2, 3, 1, 1), (5, 3, 0, 1), (5, 40, 1, 1), (2, 40, 0, 0)])
@pytest.mark.parametrize("w,p", WIDTHS)
def test_cpu_garble_evaluate_gives_the_model(lgc, gccpu, oracle, w, p, c, M, normalize, se):
    """garbled and evaluated on the CPU, launch by launch at the gate steps the lowering assigned"""
    rng = np.random.default_rng(zlib.crc32(("scan ge %d %d %d %d %d" % (w, normalize, c, M, se)).encode()))
    shares, _, X, _ = case(rng, c, M, w, p, normalize, nshares=2)
    rs = resid(X, c)
    sysm = lgc.make_system(c + 1, w, p, "cholesky", 0, LAM, 2, normalize, 0, 0)
    prog = program(lgc, sysm, M, se, rs)
    dec, gates, _ = gccpu.garble_eval(prog, shares)
    assert gates == prog.info.total_gates
    assert shown(prog, dec, w, M, se) == sm.revealed(sm.scan(oracle, shares, c, M, w, p, LAM, rs, normalize), se)


def test_karatsuba_batches_give_the_model(lgc, gccpu, oracle):
    """c = 5, M = 420 at W = 64: the tail's batch holds 2 M c + c = 4 205 > 4 096 products, so P.dots makes them Karatsuba pairs
    reading the half-difference words the division records left in the shadow; the column batches (at most M (c - 1) = 1 680
    products) stay plain.  The revealed words are the model's all the same"""
    w, p, c, M = 64, 56, 5, 420
    rng = np.random.default_rng(77)
    shares, _, X, _ = case(rng, c, M, w, p, 1, nshares=2, n=4 * (c + 1) + 40)
    rs = resid(X, c)
    sysm = lgc.make_system(c + 1, w, p, "cholesky", 0, LAM, 2, 1, 0, 0)
    prog = program(lgc, sysm, M, 1, rs)
    r = sel._recs(prog)
    assert (r[:, 0] == OP_MACK).sum() > M and (r[:, 0] == OP_MAC).sum() > M
    assert shown(prog, sel.plain(gccpu, prog, w, p, shares), w, M, 1) == sm.revealed(sm.scan(oracle, shares, c, M, w, p, LAM, rs, 1), 1)


# ---- the scan words against the existing inference program
ULPS = {64: 4 * 10, 32: 4 * 13}


@pytest.mark.parametrize("w,p", WIDTHS)
def test_scan_words_against_the_inference_program(lgc, gccpu, oracle, w, p):
    """lambda = 0: w_m against u_{D-1} of the EXISTING inference program (linreg_gc_inference.h) on the augmented system [C, g_m],
    both input paths, (c, M) = (1, 1), (2, 3), (5, 40).  Both approximate sqrt(s2 (M^-1)_DD), but round in different places: the
    inference forms e = Y - b0^T beta from the back-substituted beta and v as |z|^2 over one entry, the scan e = E0 - t^2 from
    the forward substitution.  Largest difference measured over these cases on the CPU: 10 ulps at W = 64 / p = 56 and 13 ulps
    at W = 32 / p = 24 (of words of order 2^p: w_m is of order 1).  The bound is four times that: 40 and 52 ulps"""
    worst = 0
    for normalize in (0, 1):
        for c, M in ((1, 1), (2, 3), (5, 40)):
            rng = np.random.default_rng(zlib.crc32(("scan infer %d %d %d %d" % (w, normalize, c, M)).encode()))
            shares, tot, X, _ = case(rng, c, M, w, p, normalize, lam=0.0)
            D, rs = c + 1, resid(X, c)
            sysm = lgc.make_system(D, w, p, "cholesky", 0, 0.0, 3, normalize, 0, 0)
            prog = program(lgc, sysm, M, 1, rs)
            got = shown(prog, sel.plain(gccpu, prog, w, p, shares), w, M, 1)
            inf = lgc.Program(sysm, inference=("se",), resid_scale=rs)
            for m in range(M):
                aug = ti.split(rng, sm.augmented_words(tot, c, M, m), 3, w)
                dec = sel.plain(gccpu, inf, w, p, aug)
                words = sx(dec[inf.info.rv_beta:inf.info.rv_beta + 2 * D], w).tolist()
                assert words[D - 1] == got[m]                      # (beta_m once more, through the inference program)
                worst = max(worst, abs(words[2 * D - 1] - got[M + m]))
    print("W = %d: largest |w_m - u_{D-1}| = %d ulps" % (w, worst))
    assert worst <= ULPS[w], worst


# ---- the model against float64
@pytest.mark.parametrize("w,p", WIDTHS)
def test_model_against_float64(oracle, w, p):
    """beta_m and w_m / sqrt(n) of the model against numpy float64 OLS per candidate on the unquantised data (lambda = 0, both
    input paths, c = 5, M = 8, n = 4 D + 40), with the tolerances tests/test_inference_cpu.py uses for its model against numpy
    (REL: 2^-46 at W = 64 and 2^-16 at W = 32), every candidate compared.  The standard errors are compared relatively, as
    there; a coefficient may lie arbitrarily close to zero, so the coefficients are compared absolutely against the same
    figure -- the data are studentised and no coefficient exceeds 1 in magnitude, so this asks no less than a relative bound
    on a coefficient of order 1 would.  Largest errors measured on these fixtures: W = 64: 3.0e-16 (beta), 2.2e-16 (se);
    W = 32: 9.9e-7 (beta), 7.5e-7 (se).  The model asserts its range condition on the way"""
    c, M = 5, 8
    D = c + 1
    worst = {"beta": 0.0, "se": 0.0}
    for normalize in (0, 1):
        rng = np.random.default_rng(zlib.crc32(("scan float %d" % normalize).encode()))
        shares, _, X, y = case(rng, c, M, w, p, normalize, lam=0.0, nshares=2)
        n = X.shape[0]
        rs = n / (n - D)
        m = sm.scan(oracle, shares, c, M, w, p, 0.0, rs, normalize)
        f = lambda v: v / 2.0 ** p
        for k in range(M):
            Z = np.column_stack([X[:, :c], X[:, c + k]])
            beta = np.linalg.solve(Z.T @ Z, Z.T @ y)
            res = y - Z @ beta
            s2 = rs * float(res @ res) / n
            se = math.sqrt(s2 * np.linalg.inv(Z.T @ Z)[c, c])
            worst["beta"] = max(worst["beta"], abs(f(m["beta"][k]) - beta[c]))
            assert abs(beta[c]) < 1
            worst["se"] = max(worst["se"], abs(f(m["w"][k]) / math.sqrt(n) / se - 1))
    print("W = %d: largest errors %r" % (w, worst))
    assert max(worst.values()) < ti.REL[w], worst


# ---- the structure of the lowering
def _launch_ops(prog):
    r = sel._recs(prog)
    return [(int(r[L["first_rec"], 0]), L["nrec"]) for L in prog.launches()]


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", WIDTHS)
def test_structure(lgc, w, p, normalize):
    """without SE no z, v or e record exists: no OP_MUL at all, and the divisions and square roots are the shared prefix's plus
    c + 2 and 1 per candidate (SE: one more of each and four products per candidate).  The covariate factorisation appears
    once whatever M: c square roots and c (c - 1) / 2 + c divisions of the prefix.  No launch count grows with M: M = 3 and
    M = 40 have the same number of launches, with and without SE.  Step k of the candidates rides in column k's division launch:
    c - k records of the prefix plus M"""
    c = 5
    sysm = lgc.make_system(c + 1, w, p, "cholesky", 0, LAM, 2, normalize, 0, 0)
    for se in (0, 1):
        counts = []
        for M in (3, 40):
            prog = program(lgc, sysm, M, se, 1.25)
            r = sel._recs(prog)
            ops = _launch_ops(prog)
            counts.append(len(ops))
            nsqrt, ndiv, nmul = [int((r[:, 0] == op).sum()) for op in (OP_SQRT, OP_DIV, OP_MUL)]
            assert nsqrt == c + M + (M if se else 0)
            assert ndiv == c * (c - 1) // 2 + c + M * c + 2 * M + (M if se else 0)
            assert nmul == (4 * M if se else 0)
            assert int((r[:, 0] == OP_CONST).sum()) == (1 if normalize else 0) + (2 if se else 0)
            fact_divs = [nrec for op, nrec in ops if op == OP_DIV][:c]
            assert fact_divs == [c - k + M for k in range(c)]
            assert ops[-1] == (OP_REVEAL, M * (2 if se else 1))
        assert counts[0] == counts[1], counts
    # the caps cut an M-record launch exactly as every launch: more launches only where a launch outgrows the cap
    big, small = program(lgc, sysm, 40, 1, 1.25), program(lgc, sysm, 3, 1, 1.25)
    assert big.info.n_launches == small.info.n_launches and big.info.max_launch_steps > small.info.max_launch_steps


def test_sizes_through_the_binding(lgc):
    for c, M in ((1, 1), (5, 40)):
        sysm = lgc.make_system(c + 1, 64, 56, "cholesky", 0, 0.01, 3, 1, 0, 0)
        assert lgc._scan_in_words(sysm, M) == c * (c + 1) // 2 + c + 1 + M * (c + 2) == sm.in_words(c, M)
        assert lgc.Program(sysm, scan=M).info.n_reveal == M
        assert lgc.Program(sysm, scan=M, scan_se=True, resid_scale=1.5).info.n_reveal == 2 * M
    s = lgc._scan_summary(np.array([1 << 55, -(1 << 56)]), np.array([1 << 55, 1 << 56]), 4, lgc.make_system(3, 64, 56, "cholesky", 0, 0.0, 2, 1, 0, 0))
    assert s["beta"].tolist() == [0.5, -1.0] and s["std_err"].tolist() == [0.25, 0.5]
    assert lgc._scan_summary(np.array([1 << 55]), None, 4, lgc.make_system(3, 64, 56, "cholesky", 0, 0.0, 2, 1, 0, 0))["std_err"] is None


# ---- rejections and coverage
def test_rejections(lgc):
    d = 4
    chol = lgc.make_system(d, 64, 56, "cholesky", 0, 0.01, 2, 1, 0, 0)
    makers = (lambda s, **k: lgc.Program(s, **k), lambda s, **k: lgc.Solver(s, **k),
              lambda s, **k: lgc.Party(s, lgc.GARBLER, seed=bytes(16), **k))

    def bad(want, s, **k):
        for make in makers:                               # (every check precedes the look for a GPU)
            with pytest.raises(lgc.LgcError) as e:
                make(s, **dict(dict(scan=3, scan_se=True, resid_scale=1.25), **k))
            assert e.value.code == -1 and want in str(e.value), str(e.value)

    for alg in ("cgd", "ldlt", "lasso"):
        bad("a scan is lowered for algorithm = LGC_ALG_CHOLESKY only", lgc.make_system(d, 64, 56, alg, 3, 0.01, 2, 1, 0, 0))
    bad("a scan needs d >= 2", lgc.make_system(1, 64, 56, "cholesky", 0, 0.01, 2, 1, 0, 0))
    bad("a scan takes 1..1048576 candidate columns", chol, scan=0)
    bad("a scan takes 1..1048576 candidate columns", chol, scan=(1 << 20) + 1)
    bad("trace is not lowered for a scan", lgc.make_system(d, 64, 56, "cholesky", 0, 0.01, 2, 1, 0, 1))
    bad("reveal_inputs is not lowered for a scan", lgc.make_system(d, 64, 56, "cholesky", 0, 0.01, 2, 1, 1, 0))
    for v in (0.0, -1.0, float("nan"), float("inf")):
        bad("resid_scale must be finite and > 0", chol, resid_scale=v)
    bad("precision 56 cannot hold it in a 64-bit word", chol, resid_scale=128.0)
    bad("precision 24 cannot hold it in a 32-bit word", lgc.make_system(d, 32, 24, "cholesky", 0, 0.01, 2, 1, 0, 0), resid_scale=128.0)
    bad("width must be 32 or 64", lgc.make_system(d, 48, 40, "cholesky", 0, 0.01, 2, 1, 0, 0))
    bad("scan too large", lgc.make_system(4096, 64, 56, "cholesky", 0, 0.01, 2, 1, 0, 0), scan=1 << 20)
    bad("scan too large", lgc.make_system(3, 64, 56, "cholesky", 0, 0.01, 600, 1, 0, 0), scan=1 << 20)
    # the binding
    bad("scan_se needs resid_scale=", chol, resid_scale=None)
    bad("resid_scale belongs to scan_se=True", chol, scan_se=False)
    bad("does not combine with targets", chol, targets=2)
    bad("does not combine with folds, lambdas", chol, lambdas=[0.1, 0.2], folds=2)
    bad("does not combine with inference", chol, inference=("se",))
    for make in makers:
        with pytest.raises(lgc.LgcError) as e:
            make(chol, scan_se=True)
        assert "scan_se belongs to scan=M" in str(e.value)
    # the library's own check of the reveal bits (the binding never sends a bad word)
    Lb, C = lgc.lib(), lgc.C
    for bits in (2, 3, -1):
        h = C.c_void_p()
        assert Lb.lgc_program_build_scan(C.byref(h), C.byref(chol), 3, 1.25, bits) == -1
        assert "scan reveal flags" in Lb.lgc_last_error().decode()
        assert Lb.lgc_solver_create_scan(C.byref(h), 0, C.byref(chol), bytes(16), 3, 1.25, bits) == -1
        assert Lb.lgc_party_create_scan(C.byref(h), 0, C.byref(chol), lgc.GARBLER, bytes(16), 0, 3, 1.25, bits) == -1
    h = C.c_void_p()
    assert Lb.lgc_program_build_scan(C.byref(h), C.byref(chol), 3, float("nan"), 0) == 0      # resid_scale is not read without SE
    Lb.lgc_program_destroy(h)
    assert Lb.lgc_program_build_scan(None, C.byref(chol), 3, 1.25, 1) == -1 and "null out" in Lb.lgc_last_error().decode()
    assert Lb.lgc_program_build_scan(C.byref(C.c_void_p()), None, 3, 1.25, 1) == -1 and "null system" in Lb.lgc_last_error().decode()


def test_fingerprint_covers_the_scan(lgc):
    """the header promises it; Party objects need a GPU, so the promise is checked where one is (tests/test_scan_gpu.py); here:
    the programs of different M, reveal bits and resid_scale are different programs"""
    sysm = lgc.make_system(3, 64, 56, "cholesky", 0, 0.01, 2, 1, 0, 0)
    recs = [lgc.Program(sysm, scan=M, scan_se=se, resid_scale=rs).records().tobytes()
            for M, se, rs in ((3, False, None), (4, False, None), (3, True, 1.25), (3, True, 1.5))]
    assert len(set(recs)) == 4


def test_header_is_exported_and_documented(lgc):
    hdr = open(os.path.join(ROOT, "include", "linreg_gc_scan.h")).read()
    names = set(re.findall(r"^[a-z][^\n(]*?\b(lgc_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    assert names == {"lgc_program_build_scan", "lgc_solver_create_scan", "lgc_party_create_scan", "lgc_p1_set_divisor", "lgc_p1_local_scan"}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for nme in names:
        assert hasattr(lgc.lib(), nme), nme
        assert nme in doc, nme
    for word in ("LGC_SCAN_SE 1", "LGC_MAX_SCAN (1u << 20)", "T_c + c + 1 + M (c + 2)", "Range condition", "bit for bit", "variance-inflation"):
        assert word in hdr, word
    assert "linreg_gc_scan.h" in doc and "### 1.16" in doc
    assert "### 2.9" in design and "lgc_program_build_scan" in design and "p1_scan_kernel" in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--scan=" in readme and "scan=" in readme


# ---- bin/linreg
def _linreg(*args, inp="readme_example.in"):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "linreg-mpc_amd", "host")], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "linreg-mpc_amd", "host", "bin", "linreg")
    return subprocess.run([exe, os.path.join(ROOT, "tests", "golden", inp), "56", "3"] + list(args), capture_output=True, timeout=60)


@pytest.mark.parametrize("args,want", [
    (["cgd", "10", "0.001", "--scan=2"], b"--scan is for Algorithm cholesky"),
    (["ldlt", "0", "0.001", "--scan=2"], b"--scan is for Algorithm cholesky"),
    (["cholesky", "0", "0.001", "--scan_se"], b"--scan_se belongs to --scan"),
    (["cholesky", "0", "0.001", "--scan=0"], b"--scan wants a candidate count"),
    (["cholesky", "0", "0.001", "--scan=1000"], b"--scan needs at least one covariate column"),
    (["cholesky", "0", "0.001", "--scan=2", "--lambdas=0.1,0.01"], b"--scan and --lambdas"),
    (["cholesky", "0", "0.001", "--scan=2", "--lambdas=0.1,0.01", "--folds=2"], b"--scan and --lambdas"),
    (["cholesky", "0", "0.001", "--scan=2", "--inference"], b"--scan and --inference"),
    (["cholesky", "0", "0.001", "--scan=2", "--table_ring", "--devices=0,0"], b"--scan and --devices"),
    (["cholesky", "0", "0.001", "--scan=2", "--ti_ring"], b"--scan and --ti_ring"),
    (["cholesky", "0", "0.001", "--scan=2", "--ot_ring"], b"--scan and --ot_ring"),
    (["cholesky", "0", "0.001", "--scan=2", "--input_ring"], b"--scan and --input_ring"),
])
def test_bin_linreg_rejections(args, want):
    r = _linreg(*args)
    assert r.returncode != 0 and want in r.stdout + r.stderr, (args, r.stdout[-300:], r.stderr[-300:])
    assert b"Party 3 finished phase 1" not in r.stdout


def test_bin_linreg_scan_se_needs_more_rows_than_columns(tmp_path):
    """resid_scale = n / (n - D): n <= c + 1 is refused before any party connects"""
    tok = open(os.path.join(ROOT, "tests", "golden", "readme_example.in")).read().split("\n")
    n, d, P_ = map(int, tok[0].split())
    rows, ys = tok[2 + P_ + 2:2 + P_ + 2 + n], tok[2 + P_ + 2 + n + 1].split()
    M = 1
    k = d - M + 1                                         # keep c + 1 rows
    path = str(tmp_path / "short.in")
    open(path, "w").write("\n".join(["%d %d %d" % (k, d, P_)] + tok[1:1 + P_ + 2] + ["%d %d" % (k, d)] + rows[:k] + ["%d" % k, " ".join(ys[:k]), ""]))
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "linreg-mpc_amd", "host")], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "linreg-mpc_amd", "host", "bin", "linreg")
    r = subprocess.run([exe, path, "56", "3", "cholesky", "0", "0.001", "--scan=%d" % M, "--scan_se"], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"--scan_se needs more rows than columns" in r.stdout + r.stderr, (r.stdout[-300:], r.stderr[-300:])
