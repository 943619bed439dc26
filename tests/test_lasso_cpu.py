"""The lasso solver (include/linreg_gc_lasso.h) on the CPU: the lowered program, run record by record by the CPU checker and
garbled + evaluated by its CPU backends, against the independent model of tests/lasso_model.py; its sparsity and its
convergence against float64 FISTA and the oracle's ridge solve; its launch shape and gate count at d = 500; the rejections.
No GPU needed."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import lasso_model
from helpers import oracle_solve, split_shares, sx, synth_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OP_MAC, OP_SUM, OP_MAC2, OP_MACK, OP_PROX = 1, 2, 19, 20, 26        # gc_exec.h


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


def _case(oracle, rng, d, w, p, scale=1):
    A, b = synth_system(oracle, rng, 3 * d + 20, d, w, p)
    with np.errstate(over="ignore"):
        return A * np.uint64(scale), b * np.uint64(scale)


@pytest.mark.parametrize("d", [1, 5, 17])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 28)])
def test_lowered_program_reveals_the_model(lgc, gccpu, oracle, w, p, normalize, d):
    """beta and the trace (x after every iteration) of the lowered program, run record by record, are the model's;
    scale 8 on the two-party path makes the step a right shift (l > p)"""
    for scale in ((1, 8) if normalize == 0 else (1,)):
        rng = np.random.default_rng(zlib.crc32(("%d %d %d %d" % (w, normalize, d, scale)).encode()))
        N, lam, l1 = 7, 0.05, 0.003
        A, b = _case(oracle, rng, d, w, p, scale)
        shares = split_shares(rng, A, b, 2, w)
        sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, normalize, 0, 1)
        prog = lgc.Program(sysm, l1=l1)
        dec = _plain(gccpu, prog, w, p, shares)
        a, bb = _inputs(oracle, A, b, d, w, p, lam, normalize)
        beta, trace, ell, _ = lasso_model.lasso(a, bb, d, w, p, N, l1)
        info = prog.info
        assert sx(dec[info.rv_beta:info.rv_beta + d], w).tolist() == beta
        assert sx(dec[info.rv_trace:info.rv_trace + N * d], w).reshape(N, d).tolist() == trace
        assert (ell > p) == (scale > 1 and d > 1) or d == 1


@pytest.mark.parametrize("d", [1, 5, 17])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 28)])
def test_cpu_garble_evaluate_gives_the_model(lgc, gccpu, oracle, w, p, normalize, d):
    rng = np.random.default_rng(zlib.crc32(("ge %d %d %d" % (w, normalize, d)).encode()))
    N, lam, l1 = 4, 0.05, 0.003
    A, b = _case(oracle, rng, d, w, p)
    shares = split_shares(rng, A, b, 2, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, normalize, 0, 0)
    prog = lgc.Program(sysm, l1=l1)
    dec, gates, _ = gccpu.garble_eval(prog, shares)
    assert gates == prog.info.total_gates
    a, bb = _inputs(oracle, A, b, d, w, p, lam, normalize)
    assert sx(dec[prog.info.rv_beta:prog.info.rv_beta + d], w).tolist() == lasso_model.lasso(a, bb, d, w, p, N, l1)[0]


def test_karatsuba_size_matches_the_model(lgc, gccpu, oracle):
    """d = 96: the products run through OP_MACK, on the hdiff(y) words the OP_PROX records of the previous iteration formed"""
    rng = np.random.default_rng(96)
    w, p, d, N, lam, l1 = 64, 56, 96, 3, 0.01, 0.0005
    A, b = _case(oracle, rng, d, w, p)
    shares = split_shares(rng, A, b, 2, w)
    prog = lgc.Program(lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0), l1=l1)
    recs = np.frombuffer(prog.records().tobytes(), dtype=np.uint32).reshape(-1, 10)
    assert (recs[:, 0] == OP_MACK).any() and (recs[recs[:, 0] == OP_PROX, 7] != 0).all()
    dec = _plain(gccpu, prog, w, p, shares)
    a, bb = _inputs(oracle, A, b, d, w, p, lam, 1)
    beta = lasso_model.lasso(a, bb, d, w, p, N, l1)[0]
    assert sx(dec[prog.info.rv_beta:prog.info.rv_beta + d], w).tolist() == beta
    assert 0 < beta.count(0) < d


def _fista_float(a, bb, d, p, ell, l1, c):
    """float64 FISTA with the circuit's step 2^(p - l) and its quantised c_k; returns the last x and the last z"""
    M = np.array(lasso_model.full_matrix(a, d, 64), dtype=float) / 2.0 ** p
    b = np.array(bb, dtype=float) / 2.0 ** p
    alpha, theta = 2.0 ** (p - ell), l1 * 2.0 ** (p - ell)
    x = np.zeros(d); y = np.zeros(d); z = np.zeros(d)
    for ck in c:
        z = y - alpha * (M @ y - b)
        xn = np.sign(z) * np.maximum(np.abs(z) - theta, 0.0)
        y = xn + (ck / 2.0 ** p) * (xn - x)
        x = xn
    return x, z, theta


def test_planted_sparse_beta(lgc, gccpu, oracle):
    """a sparse planted beta and a large lambda1: the coordinates float64 FISTA (same step, same c_k) sets to zero with margin
    are the word 0 exactly; the others agree within 1e-9"""
    rng = np.random.default_rng(2024)
    w, p, d, n, N, lam, l1 = 64, 56, 12, 400, 60, 0.01, 0.004
    X = rng.standard_normal((n, d)); X /= np.abs(X).max(axis=0)
    beta_true = np.zeros(d); beta_true[[1, 4, 9]] = [0.9, -0.7, 0.5]
    y = X @ beta_true + 0.01 * rng.standard_normal(n)
    A, b = oracle.aggregate(oracle.quantize(X, p, n, w), oracle.quantize(y, p, n, w), n, d, p, w)
    shares = split_shares(rng, A, b, 2, w)
    prog = lgc.Program(lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0), l1=l1)
    dec = _plain(gccpu, prog, w, p, shares)
    got = sx(dec[prog.info.rv_beta:prog.info.rv_beta + d], w)
    a, bb = _inputs(oracle, A, b, d, w, p, lam, 1)
    M = lasso_model.full_matrix(a, d, w)
    ell = lasso_model.step_exponent(M, d, w)
    x, z, theta = _fista_float(a, bb, d, p, ell, l1, lasso_model.coefficients(N, w, p))
    zero = np.abs(z) < theta - 1e-6
    assert zero.sum() >= d // 2 and (~zero).sum() >= 2, zero
    assert (got[zero] == 0).all()
    assert np.abs(got[~zero] / 2.0 ** p - x[~zero]).max() < 1e-9
    assert {1, 4} <= set(np.flatnonzero(~zero)) <= {1, 4, 9}                # (the smallest planted coefficient may go too)


def test_without_l1_converges_to_the_ridge_solution(lgc, gccpu, oracle):
    """lambda1 = 0, N = 400, d = 6: beta is within 1e-6 of the oracle's ridge solve (Cholesky on the same M, b)"""
    rng = np.random.default_rng(6)
    w, p, d, N, lam = 64, 56, 6, 400, 0.3
    A, b = _case(oracle, rng, d, w, p)
    shares = split_shares(rng, A, b, 2, w)
    prog = lgc.Program(lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0), l1=0.0)
    dec = _plain(gccpu, prog, w, p, shares)
    got = sx(dec[prog.info.rv_beta:prog.info.rv_beta + d], w) / 2.0 ** p
    ridge, _, _ = oracle_solve(oracle, A, b, d, w, p, "cholesky", 0, lam, 1)
    assert np.abs(got - np.asarray(ridge) / 2.0 ** p).max() < 1e-6


def test_d500_gate_count_and_one_launch_per_iteration(lgc):
    """d = 500, N = 15: fewer AND gates than CGD-15 (14 products against 15, no dividers in the loop); an iteration is the
    product's launches (Karatsuba MAC, merge of the partial sums) and then exactly one launch of d OP_PROX records"""
    d, N = 500, 15
    la = lgc.Program(lgc.make_system(d, 64, 56, "lasso", N, 0.001, 2, 1, 0, 0), l1=0.001)
    cg = lgc.Program(lgc.make_system(d, 64, 56, "cgd", N, 0.001, 2, 1, 0, 0))
    assert la.info.total_gates < cg.info.total_gates
    ops = np.frombuffer(la.records().tobytes(), dtype=np.uint32).reshape(-1, 10)[:, 0]
    kinds = [set(ops[L["first_rec"]:L["first_rec"] + L["nrec"]].tolist()) for L in la.launches()]
    prox = [i for i, k in enumerate(kinds) if OP_PROX in k]
    assert len(prox) == N
    for k, i in enumerate(prox):
        assert kinds[i] == {OP_PROX} and la.launches()[i]["nrec"] == d
        if k == 0:
            continue
        between = kinds[prox[k - 1] + 1:i]
        assert between and all(s <= {OP_MACK, OP_MAC, OP_SUM} for s in between)
        assert OP_MACK in between[0] and kinds[i - 1] == {OP_SUM}           # the merge of the product, then OP_PROX
    assert len(kinds) - 1 == prox[-1] + 1                                  # then only the reveal of beta


def test_rejections(lgc):
    sysm = lgc.make_system(4, 64, 56, "lasso", 5, 0.01, 2, 1, 0, 0)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(lgc.LgcError) as e:
            lgc.Program(sysm, l1=bad)
        assert e.value.code == -1 and "lambda1" in str(e.value)
    with pytest.raises(lgc.LgcError) as e:                                  # the plain calls carry no lambda1
        lgc.Program(sysm)
    assert "lambda1" in str(e.value)
    with pytest.raises(lgc.LgcError) as e:                                  # (the solver and party refuse before they look for a GPU)
        lgc.Solver(sysm)
    assert "lambda1" in str(e.value)
    with pytest.raises(lgc.LgcError) as e:
        lgc.Party(sysm, lgc.GARBLER, seed=bytes(16))
    assert "lambda1" in str(e.value)
    with pytest.raises(lgc.LgcError) as e:                                  # lasso with several targets
        lgc.Program(sysm, targets=2)
    assert "target" in str(e.value)
    with pytest.raises(lgc.LgcError) as e:                                  # lasso in a lambda sweep
        lgc.Program(sysm, lambdas=[0.1, 0.2])
    assert "sweep" in str(e.value)
    with pytest.raises(lgc.LgcError):
        lgc.Program(lgc.make_system(4, 64, 56, "cgd", 5, 0.01, 2, 1, 0, 0), l1=0.1)   # the lasso calls need LGC_ALG_LASSO
    lgc.Program(sysm, l1=0.0).close()


def test_bin_linreg_wants_l1_for_lasso():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "linreg-mpc_amd", "host")], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "linreg-mpc_amd", "host", "bin", "linreg")
    inp = os.path.join(ROOT, "tests", "golden", "readme_example.in")
    r = subprocess.run([exe, inp, "56", "3", "lasso", "10", "0.001"], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"--l1" in r.stdout + r.stderr
    r = subprocess.run([exe, inp, "56", "3", "cgd", "10", "0.001", "--l1=0.1"], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"--l1" in r.stdout + r.stderr


def test_lasso_header_is_exported_and_documented(lgc):
    hdr = open(os.path.join(ROOT, "include", "linreg_gc_lasso.h")).read()
    names = set(re.findall(r"^[a-z][^\n(]*?\b(lgc_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    assert names == {"lgc_program_build_lasso", "lgc_solver_create_lasso", "lgc_party_create_lasso"}
    assert re.search(r"#define LGC_ALG_LASSO 4\b", hdr)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for nme in names:
        assert hasattr(lgc.lib(), nme), nme
        assert nme in doc, nme
    assert "linreg_gc_lasso.h" in doc and "OP_PROX" in design
    base = open(os.path.join(ROOT, "include", "linreg_gc.h")).read()
    assert "lasso" not in base.lower()                                     # the drop-in header is unchanged
    assert lgc.ALG["lasso"] == 4
