"""The lasso solver (include/linreg_gc_lasso.h) on the MI355X: the co-located solver against the CPU checker and the
independent model (tests/lasso_model.py) at both widths, on every generic record kernel (column-split, 4-wave, wide), the
two roles apart (in one process through host buffers; as bin/linreg's CSP and Evaluator over the hipIpc table ring), and
the wrapper's path.  At most six processes hold the GPU at once
(the five parties of the README configuration and this one)."""
import os
import re
import subprocess

import numpy as np
import pytest

import lasso_model
from helpers import free_ports, split_shares, sx, synth_system

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "linreg-mpc_amd", "host")
OP_PROX = 26                               # gc_exec.h


def _circuit_input(oracle, A, b, d, w, p, lam, normalize):
    a = oracle.sum_shares(np.asarray(A, dtype=np.uint64)[None, :], w)
    bb = oracle.sum_shares(np.asarray(b, dtype=np.uint64)[None, :], w)
    if normalize:
        a, bb = oracle.circuit_input(a, bb, d, lam, p, w)
    return a, bb


def _plain(gccpu, prog, w, p, shares):
    info = prog.info
    words = np.zeros(info.n_words, dtype=np.uint64)
    words[info.in_base:info.in_base + shares.size] = shares.ravel() & np.uint64((1 << w) - 1)
    dec = np.zeros(info.n_reveal + 1, dtype=np.uint64)
    gccpu.plain_run(prog.records(), info.n_records, w, p, words, dec)
    return sx(dec[info.rv_beta:info.rv_beta + int(prog.system.d)], w).tolist()


def _solve(lgc, sysm, shares, l1):
    s = lgc.Solver(sysm, seed=bytes(range(3, 19)), l1=l1)
    s.set_shares(shares)
    s.run()
    beta, trace = s.beta().tolist(), (s.trace().tolist() if sysm.trace else None)
    gates, secs = s.iterations()
    s.close()
    return beta, trace, gates


@pytest.mark.parametrize("w,p,normalize,scale", [(64, 56, 1, 1), (32, 28, 1, 1), (64, 56, 0, 1), (32, 28, 0, 1), (64, 56, 0, 16),
                                                 (32, 28, 0, 4)])
def test_solver_matches_checker_and_model(lgc, oracle, gccpu, w, p, normalize, scale):
    """scale: M and b multiplied by a power of two on the two-party path, so that the step is a right shift (l > p)"""
    rng = np.random.default_rng(w + normalize)
    d, n, N, lam, l1 = 12, 60, 9, 0.05, 0.002
    A, b = synth_system(oracle, rng, n, d, w, p)
    with np.errstate(over="ignore"):
        A, b = A * np.uint64(scale), b * np.uint64(scale)
    shares = split_shares(rng, A, b, 2, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, normalize, 0, 1)
    beta, trace, gates = _solve(lgc, sysm, shares, l1)
    a, bb = _circuit_input(oracle, A, b, d, w, p, lam, normalize)
    exp, exp_trace, _, _ = lasso_model.lasso(sx(a, w).tolist(), sx(bb, w).tolist(), d, w, p, N, l1)
    assert beta == exp
    assert trace == exp_trace
    assert beta == _plain(gccpu, lgc.Program(sysm, l1=l1), w, p, shares)
    assert len(gates) == N and all(np.diff(gates.astype(np.int64)) > 0)


def test_four_wave_kernel_runs_prox(lgc, oracle):
    """the column-split kernel off: the launches of d = 12 OP_PROX records run on the 4-wave kernel instead"""
    rng = np.random.default_rng(12)
    w, p, d, N, lam, l1 = 64, 56, 12, 6, 0.05, 0.002
    A, b = synth_system(oracle, rng, 60, d, w, p)
    shares = split_shares(rng, A, b, 2, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0)
    lgc.set_split_kernels(False, False)
    try:
        beta, _, _ = _solve(lgc, sysm, shares, l1)
    finally:
        lgc.set_split_kernels(True, True)
    a, bb = _circuit_input(oracle, A, b, d, w, p, lam, 1)
    assert beta == lasso_model.lasso(a.tolist(), bb.tolist(), d, w, p, N, l1)[0]


@pytest.mark.parametrize("d,N", [(300, 3), (600, 2)])
def test_large_systems_quad_and_wide_prox_launches(lgc, oracle, d, N):
    """d = 300: a launch of 300 OP_PROX records runs on the 4-wave kernel; d = 600 on the wide kernel (one wave per record);
    both with Karatsuba products and the hdiff(y) words the OP_PROX records form"""
    rng = np.random.default_rng(d)
    w, p, lam, l1 = 64, 56, 0.01, 0.0002
    A, b = synth_system(oracle, rng, 2 * d, d, w, p)
    shares = split_shares(rng, A, b, 2, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0)
    prog = lgc.Program(sysm, l1=l1)
    recs = np.frombuffer(prog.records().tobytes(), dtype=np.uint32).reshape(-1, 10)
    assert (recs[recs[:, 0] == OP_PROX, 7] != 0).all()          # sb: the records form hdiff(y_i)
    beta, _, _ = _solve(lgc, sysm, shares, l1)
    a, bb = _circuit_input(oracle, A, b, d, w, p, lam, 1)
    exp = lasso_model.lasso(a.tolist(), bb.tolist(), d, w, p, N, l1)[0]
    assert beta == exp
    assert 0 < sum(v == 0 for v in exp) < d


def test_parties_apart(lgc, oracle):
    rng = np.random.default_rng(9)
    w, p, d, N, P, l1 = 64, 56, 7, 6, 3, 0.001
    A, b = synth_system(oracle, rng, 50, d, w, p)
    shares = split_shares(rng, A, b, P, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, 0.01, P, 1, 0, 1)
    G = lgc.Party(sysm, lgc.GARBLER, seed=bytes(range(5, 21)), l1=l1)
    E = lgc.Party(sysm, lgc.EVALUATOR, l1=l1)
    assert G.program_fingerprint() == E.program_fingerprint()
    other = lgc.Party(sysm, lgc.EVALUATOR, l1=2 * l1)
    assert other.program_fingerprint() != E.program_fingerprint()
    other.close()
    for s in range(P):
        E.set_input_labels(s, G.encode_inputs(s, shares[s]))
    for k in range(G.num_launches):
        E.evaluate(k, G.garble(k))
    beta, trace, _ = E.finish(G.decode_bits())
    G.close(); E.close()
    a, bb = _circuit_input(oracle, A, b, d, w, p, 0.01, 1)
    exp, exp_trace, _, _ = lasso_model.lasso(a.tolist(), bb.tolist(), d, w, p, N, l1)
    assert beta.tolist() == exp
    assert trace.tolist() == exp_trace


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


def _file_model(oracle, path, p, w, lam2, N, l1):
    inp = oracle.read_input(path)
    n, d = inp["n"], inp["d"]
    Xq = oracle.quantize(inp["X"], p, n, w)
    yq = oracle.quantize(inp["y"], p, n, w)
    A, b = oracle.aggregate(Xq, yq, n, d, p, w)
    a, bb = _circuit_input(oracle, A, b, d, w, p, lam2, 1)
    return lasso_model.lasso(a.tolist(), bb.tolist(), d, w, p, N, l1)[0]


def test_five_process_readme_run_over_the_table_ring(tmp_path, golden_dir, oracle):
    """bin/linreg <file> 56 <party> lasso 40 0.001 --l1=0.02 --table_ring: [Num. iterations CGD] is N, [Lambda] is lambda2;
    the CSP's tables reach the Evaluator process through the hipIpc table ring"""
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    path, P = _readme(tmp_path, golden_dir)
    exe = os.path.join(HOST, "bin", "linreg")
    procs = [subprocess.Popen([exe, path, "56", str(k), "lasso", "40", "0.001", "--l1=0.02", "--table_ring"], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE) for k in range(1, P + 3)]
    outs = [q.communicate(timeout=300) for q in procs]
    assert all(q.returncode == 0 for q in procs), [e.decode()[-400:] for _, e in outs]
    ev = outs[1][0].decode()
    assert "Algorithm: lasso" in ev and "Number of gates:" in ev and "Time elapsed:" in ev
    got = re.findall("-?[0-9]+\\.[0-9]+", ev.strip().splitlines()[-1])
    exp = _file_model(oracle, path, 56, 64, 0.001, 40, 0.02)
    assert got == ["%.15f" % (v / 2.0 ** 56) for v in exp]
    assert "0.000000000000000" in got and len(set(got)) > 1          # some coordinates set to zero, not all


def test_two_parties_with_different_l1_refuse(tmp_path, golden_dir):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    path, P = _readme(tmp_path, golden_dir)
    exe = os.path.join(HOST, "bin", "linreg")
    procs = [subprocess.Popen([exe, path, "56", str(k), "lasso", "10", "0.001", "--l1=%s" % ("0.03" if k == 1 else "0.02")],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE) for k in range(1, P + 3)]
    outs = [q.communicate(timeout=120) for q in procs]
    assert procs[0].returncode != 0 and procs[1].returncode != 0
    assert b"built different programs" in outs[0][1] and b"built different programs" in outs[1][1]
    assert b"Result:" not in outs[1][0]


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


def test_wrapper_fits_lasso(tmp_path, oracle):
    """MPCLinearRegression with mpc_args ["56", "lasso", "100", "0.0", "--l1=0.05"]: two wrapper instances, four bin/linreg
    processes; the coefficients equal the model's on the combined data set"""
    import multiprocessing as mp
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(11)
    n = 60
    age = rng.integers(20, 70, n).astype(float); sex = rng.integers(0, 2, n)
    height = 1.5 + 0.4 * rng.random(n); weight = 50 + 40 * rng.random(n)
    income = 800 + 35 * age + 400 * sex + 3 * weight + 50 * rng.standard_normal(n)
    csvf = tmp_path / "people.csv"
    with open(csvf, "w") as f:
        f.write("age;sex;height;weight;income\n")
        for i in range(n):
            f.write("%r;%s;%r;%r;%r\n" % (float(age[i]), "mw"[1 - int(sex[i])], float(height[i]), float(weight[i]), float(income[i])))
    base = free_ports(1)[0]
    a_ip, b_ip = "127.0.0.1:%d" % base, "127.0.0.1:%d" % (base + 100)
    args = ["56", "lasso", "100", "0.0", "--l1=0.05"]
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
    exp = _file_model(oracle, str(comb), 56, 64, 0.0, 100, 0.05)
    assert res_b == [float("%.15f" % (v / 2.0 ** 56)) for v in exp]
