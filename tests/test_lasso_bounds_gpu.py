"""Penalty factors and bounds of the lasso (include/linreg_gc_lasso_opts.h) on the MI355X: the co-located solver against the CPU
checker and the model (tests/lasso_bounds_model.py) at both widths; a d = 300 path whose bounded OP_PROX launches reach the
4-wave and wide kernels; the two roles apart, with fingerprints that follow the options; bin/linreg's five processes with
--positive over the table ring; MPCLinearRegression with --positive in mpc_args.  At most six processes hold the GPU at once
(the five parties of the README configuration and this one)."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import lasso_bounds_model as lbm
import test_lasso_bounds_cpu as cpu
from helpers import free_ports, split_shares, synth_system

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "linreg-mpc_amd", "host")
SEED = bytes(range(7, 23))
INF = math.inf


def _run(lgc, sysm, shares, **kw):
    s = lgc.Solver(sysm, seed=SEED, **kw)
    s.set_shares(shares)
    s.run()
    beta = s.beta().tolist()
    gates, _ = s.iterations()
    s.close()
    return beta, gates


@pytest.mark.parametrize("w,p", [(64, 56), (32, 28)])
def test_solver_matches_checker_and_model(lgc, oracle, gccpu, w, p):
    rng = np.random.default_rng(w + 3)
    d, n, N, lam, l1 = 12, 60, 9, 0.05, 0.003
    A, b = synth_system(oracle, rng, n, d, w, p)
    shares = split_shares(rng, A, b, 2, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0)
    f, lo, hi = cpu._options(d)
    beta, gates = _run(lgc, sysm, shares, l1=l1, penalty_factors=f, lower=lo, upper=hi)
    assert len(gates) == N
    prog = lgc.Program(sysm, l1=l1, penalty_factors=f, lower=lo, upper=hi)
    assert [beta] == cpu._beta(prog, cpu._plain(gccpu, prog, w, p, shares), w, 1)
    a, bb = cpu._inputs(oracle, A, b, d, w, p, lam, 1)
    assert [beta] == lbm.lasso_opts(a, bb, d, w, p, N, [l1], lbm.ABSOLUTE, f, lo, hi)[0]
    assert cpu._inside([beta], lo, hi, w, p)
    pos, _ = _run(lgc, sysm, shares, l1=l1, positive=True)
    assert min(pos) >= 0 and pos == lbm.lasso_opts(a, bb, d, w, p, N, [l1], lbm.ABSOLUTE, None, [0.0] * d, None)[0][0]


def test_d300_path_reaches_the_4wave_and_wide_kernels(lgc, oracle):
    """d = 300, every coordinate boxed: one value's 300 OP_PROX records per launch (the 4-wave kernel's size) and a path's
    1 200 (the wide kernel's), with Karatsuba products on every y_l"""
    rng = np.random.default_rng(301)
    w, p, d, N, lam = 64, 56, 300, 3, 0.01
    A, b = synth_system(oracle, rng, 2 * d, d, w, p)
    shares = split_shares(rng, A, b, 2, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0)
    f = [(0.0, 0.5, 1.0, 2.0)[i % 4] for i in range(d)]
    lo, hi = [-0.02] * d, [(0.01, 0.05, INF)[i % 3] for i in range(d)]
    a, bb = cpu._inputs(oracle, A, b, d, w, p, lam, 1)
    c = lgc.launch_constants()
    for ratios in ([0.1], [0.01, 0.05, 0.2, 1.0625]):
        prog = lgc.Program(sysm, l1_ratios=ratios, penalty_factors=f, lower=lo, upper=hi)
        recs = cpu._recs(prog)
        ops = recs[:, 0]
        prox = [L for L in prog.launches() if (ops[L["first_rec"]:L["first_rec"] + L["nrec"]] == cpu.OP_PROX).all()]
        assert len(prox) == N and all(L["nrec"] == len(ratios) * d for L in prox)
        assert (recs[ops == cpu.OP_PROX, 1] >> 31).all()
        assert (len(ratios) * d >= c["wide_launch"]) == (len(ratios) > 1)
        beta, _ = _run(lgc, sysm, shares, l1_ratios=ratios, penalty_factors=f, lower=lo, upper=hi)
        exp = lbm.lasso_opts(a, bb, d, w, p, N, ratios, lbm.RATIO, f, lo, hi)[0]
        assert beta == exp
        assert cpu._inside(exp, lo, hi, w, p)


def test_parties_apart(lgc, oracle):
    """garbler and evaluator in one process through host buffers; the defaults give the plain lasso's fingerprint, other
    factors or bounds another one (bin/linreg then refuses to run)"""
    rng = np.random.default_rng(19)
    w, p, d, N, P, l1 = 64, 56, 7, 6, 3, 0.002
    A, b = synth_system(oracle, rng, 50, d, w, p)
    shares = split_shares(rng, A, b, P, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, 0.01, P, 1, 0, 0)
    f, lo, hi = cpu._options(d)
    kw = dict(l1=l1, penalty_factors=f, lower=lo, upper=hi)
    G = lgc.Party(sysm, lgc.GARBLER, seed=bytes(range(5, 21)), **kw)
    E = lgc.Party(sysm, lgc.EVALUATOR, **kw)
    assert G.program_fingerprint() == E.program_fingerprint()
    plain = lgc.Party(sysm, lgc.EVALUATOR, l1=l1)
    dflt = lgc.Party(sysm, lgc.EVALUATOR, l1=l1, penalty_factors=[1.0] * d, lower=[-INF] * d, upper=[INF] * d)
    assert plain.program_fingerprint() == dflt.program_fingerprint() != E.program_fingerprint()
    plain.close(); dflt.close()
    for other in (dict(kw, penalty_factors=f[::-1]), dict(kw, upper=[INF] * d), dict(kw, lower=[v - 0.001 for v in lo])):
        o = lgc.Party(sysm, lgc.EVALUATOR, **other)
        assert o.program_fingerprint() != E.program_fingerprint()
        o.close()
    for s in range(P):
        E.set_input_labels(s, G.encode_inputs(s, shares[s]))
    for k in range(G.num_launches):
        E.evaluate(k, G.garble(k))
    beta, _, _ = E.finish(G.decode_bits())
    G.close(); E.close()
    a, bb = cpu._inputs(oracle, A, b, d, w, p, 0.01, 1)
    assert [beta.tolist()] == lbm.lasso_opts(a, bb, d, w, p, N, [l1], lbm.ABSOLUTE, f, lo, hi)[0]


def _readme(tmp_path, golden_dir):
    tok = open(os.path.join(golden_dir, "readme_example.in")).read().split("\n")
    n, d, P = map(int, tok[0].split())
    ports = free_ports(P + 2)
    for i in range(P + 2):
        parts = tok[1 + i].split()
        parts[0] = "127.0.0.1:%d" % ports[i]
        tok[1 + i] = " ".join(parts)
    path = str(tmp_path / "readme.in")
    open(path, "w").write("\n".join(tok))
    return path, P


def _file_inputs(oracle, path, p, w, lam2):
    inp = oracle.read_input(path)
    n, d = inp["n"], inp["d"]
    A, b = oracle.aggregate(oracle.quantize(inp["X"], p, n, w), oracle.quantize(inp["y"], p, n, w), n, d, p, w)
    a, bb = cpu._inputs(oracle, A, b, d, w, p, lam2, 1)
    return a, bb, d


def test_five_process_positive_over_the_table_ring(tmp_path, golden_dir, oracle):
    """bin/linreg <file> 56 <party> lasso 40 0.001 --l1=0.005 --positive --upper=0.5,inf,inf,inf,inf
    --penalty_factors=1,1,2,1,0 --table_ring: the Result line is the model's, the upper bound active, nothing negative"""
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    path, P = _readme(tmp_path, golden_dir)
    exe = os.path.join(HOST, "bin", "linreg")
    opts = ["--l1=0.005", "--positive", "--upper=0.5,inf,inf,inf,inf", "--penalty_factors=1,1,2,1,0", "--table_ring"]
    procs = [subprocess.Popen([exe, path, "56", str(k), "lasso", "40", "0.001"] + opts, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE) for k in range(1, P + 3)]
    outs = [q.communicate(timeout=300) for q in procs]
    assert all(q.returncode == 0 for q in procs), [e.decode()[-400:] for _, e in outs]
    ev = outs[1][0].decode()
    assert "Algorithm: lasso" in ev
    got = re.findall("-?[0-9]+\\.[0-9]+", ev.strip().splitlines()[-1])
    a, bb, d = _file_inputs(oracle, path, 56, 64, 0.001)
    f, lo, hi = [1, 1, 2, 1, 0], [0.0] * d, [0.5, INF, INF, INF, INF]
    exp = lbm.lasso_opts(a, bb, d, 64, 56, 40, [0.005], lbm.ABSOLUTE, f, lo, hi)[0][0]
    assert got == ["%.15f" % (v / 2.0 ** 56) for v in exp]
    assert min(exp) >= 0 and exp[0] == lbm.lm.to_fixed(0.5, 56, 64) and exp[4] != 0
    assert exp != lbm.lasso_opts(a, bb, d, 64, 56, 40, [0.005])[0][0]


def _fit_side(own, other, csv_path, spec, args, q):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "linreg-mpc_amd", "python"))
    import mpc_linear_regression as m
    r = m.MPCLinearRegression(own, other, mpc_args=args)
    kept = {}
    make_csv = r.make_csv

    def keep(matrix):
        path = make_csv(matrix)
        kept["text"] = open(path).read()
        return path
    r.make_csv = keep
    r.fit(csv_path, spec)
    q.put((spec, r.result, kept["text"]))


def test_wrapper_fits_positive_lasso(tmp_path, oracle):
    """MPCLinearRegression with mpc_args [..., "--l1=0.02", "--positive"]: the studentised coefficients equal the model's on
    the combined data set, none negative (sigma > 0 keeps the signs)"""
    import multiprocessing as mp
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(12)
    n = 60
    age = rng.integers(20, 70, n).astype(float); sex = rng.integers(0, 2, n)
    height = 1.5 + 0.4 * rng.random(n); weight = 50 + 40 * rng.random(n)
    income = 800 + 35 * age + 400 * sex - 6 * weight + 50 * rng.standard_normal(n)
    csvf = tmp_path / "people.csv"
    with open(csvf, "w") as f:
        f.write("age;sex;height;weight;income\n")
        for i in range(n):
            f.write("%r;%s;%r;%r;%r\n" % (float(age[i]), "mw"[1 - int(sex[i])], float(height[i]), float(weight[i]), float(income[i])))
    base = free_ports(1)[0]
    a_ip, b_ip = "127.0.0.1:%d" % base, "127.0.0.1:%d" % (base + 100)
    args = ["56", "lasso", "100", "0.0", "--l1=0.02", "--positive"]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    pa = ctx.Process(target=_fit_side, args=(a_ip, b_ip, str(csvf), "0 c1", args, q))
    pb = ctx.Process(target=_fit_side, args=(b_ip, a_ip, str(csvf), "2 3 r4", args, q))
    pa.start(); pb.start()
    try:
        outs = dict((o[0], o[1:]) for o in (q.get(timeout=120), q.get(timeout=120)))
    finally:
        pa.join(20); pb.join(20)
        for pr in (pa, pb):
            if pr.is_alive():
                pr.kill()
    assert pa.exitcode == 0 and pb.exitcode == 0
    res_a, file_a = outs["0 c1"]
    res_b, file_b = outs["2 3 r4"]
    assert res_a == res_b and len(res_b) == 4
    ta, tb = file_a.split("\n"), file_b.split("\n")
    rows = [ra.split()[:2] + rb.split()[2:] for ra, rb in zip(ta[6:6 + n], tb[6:6 + n])]
    comb = tmp_path / "combined.in"
    comb.write_text("\n".join(ta[:6] + [" ".join(r) for r in rows] + tb[6 + n:]))
    a, bb, d = _file_inputs(oracle, str(comb), 56, 64, 0.0)
    exp = lbm.lasso_opts(a, bb, d, 64, 56, 100, [0.02], lbm.ABSOLUTE, None, [0.0] * d, None)[0][0]
    assert res_b == [float("%.15f" % (v / 2.0 ** 56)) for v in exp]
    assert min(res_b) >= 0 and min(lbm.lasso_opts(a, bb, d, 64, 56, 100, [0.02])[0][0]) < 0
