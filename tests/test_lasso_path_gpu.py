"""The lasso path (include/linreg_gc_lasso_path.h) on the MI355X: the co-located solver against the CPU checker, the model
(tests/lasso_path_model.py) and L separate GPU lasso solves at both widths and in both modes; the OP_STEPEXP cnt = 2 variant
on every generic record kernel, forced; a d = 300 path whose OP_PROX launches reach the wide kernel; the two roles apart;
bin/linreg's five processes with --l1_ratios over the table ring.  At most six processes hold the GPU at once (the five
parties of the README configuration and this one)."""
import os
import re
import subprocess

import numpy as np
import pytest

import lasso_path_model as lpm
import test_lasso_path_cpu as cpu
from helpers import free_ports, split_shares, synth_system

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "linreg-mpc_amd", "host")
SEED = bytes(range(3, 19))


def _run(lgc, sysm, shares, **kw):
    s = lgc.Solver(sysm, seed=SEED, **kw)
    s.set_shares(shares)
    s.run()
    beta = s.beta().tolist()
    gates, _ = s.iterations()
    s.close()
    return beta, gates


@pytest.mark.parametrize("mode", [lpm.ABSOLUTE, lpm.RATIO])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 28)])
def test_solver_matches_checker_model_and_single_solves(lgc, oracle, gccpu, w, p, mode):
    rng = np.random.default_rng(w + 7 * mode)
    d, n, N, lam = 12, 60, 9, 0.05
    A, b = synth_system(oracle, rng, n, d, w, p)
    shares = split_shares(rng, A, b, 2, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0)
    values = [0.0, 0.001, 0.003, 0.01] if mode == lpm.ABSOLUTE else [0.05, 0.2, 0.5, 1.0625]
    kw = {"l1": values} if mode == lpm.ABSOLUTE else {"l1_ratios": values}
    beta, gates = _run(lgc, sysm, shares, **kw)
    assert len(gates) == N
    prog = lgc.Program(sysm, **kw)
    assert beta == cpu._beta(prog, cpu._plain(gccpu, prog, w, p, shares), w, len(values))
    a, bb = cpu._inputs(oracle, A, b, d, w, p, lam, 1)
    betas, ell, th = lpm.lasso_path(a, bb, d, w, p, N, values, mode)
    assert beta == betas
    # L separate GPU lasso solves, each with the lambda1 the path used for it (ratio mode: theta_l unshifted back to a
    # lambda1 is not public, so the single solves are checked in absolute mode only)
    if mode == lpm.ABSOLUTE:
        for l, v in enumerate(values):
            assert beta[l] == _run(lgc, sysm, shares, l1=v)[0], l
    else:
        assert all(x == 0 for x in beta[-1]) and len(set(map(tuple, beta))) == len(values)


@pytest.mark.parametrize("w", [32, 64])
@pytest.mark.parametrize("kernel", ["split", "quad2", "wide"])
def test_stepexp_ratio_variant_on_generic_kernels(lgc, gccpu, w, kernel):
    """OP_STEPEXP cnt = 2 on the forced kernel, both roles, against the plaintext machine and the integer model"""
    for p in (1, w - 8, w - 1):
        C, cases = cpu.ratio_corpus(w, p, np.random.default_rng([w, p, 2]))
        prog = C.program(lgc, lambda kind: (kernel, kernel))
        mg, me = prog.modes()
        assert mg[0] == lgc.LM[kernel] and me[0] == lgc.LM[kernel]
        s = lgc.RecordSolver(prog, seed=SEED)
        s.set_inputs(np.array(C.inputs, dtype=np.uint64))
        s.run()
        got = [int(v) for v in s.reveal()]
        s.close()
        want = cpu._ratio_expect(C, cases)
        bad = [o for o, v in want.items() if got[o] != v]
        assert not bad, (w, p, kernel, bad[:6])
        plain = cpu.oc.plain_words(gccpu, prog, C)
        assert got[:len(plain)] == plain


def test_d300_path_reaches_the_wide_kernel(lgc, oracle):
    """d = 300, L = 8: launches of 2 400 OP_PROX records (a single solve's 300 run on the 4-wave kernel) run on the wide
    kernel, with Karatsuba products on every y_l"""
    rng = np.random.default_rng(300)
    w, p, d, N, lam = 64, 56, 300, 3, 0.01
    A, b = synth_system(oracle, rng, 2 * d, d, w, p)
    shares = split_shares(rng, A, b, 2, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0)
    ratios = [0.002, 0.005, 0.01, 0.02, 0.05, 0.1, 0.3, 1.0625]
    prog = lgc.Program(sysm, l1_ratios=ratios)
    c = lgc.launch_constants()
    ops = np.frombuffer(prog.records().tobytes(), dtype=np.uint32).reshape(-1, 10)[:, 0]
    prox = [L for L in prog.launches() if (ops[L["first_rec"]:L["first_rec"] + L["nrec"]] == cpu.OP_PROX).all()]
    assert all(L["nrec"] == len(ratios) * d for L in prox)
    assert len(prox) == N and len(ratios) * d >= c["wide_launch"]
    beta, _ = _run(lgc, sysm, shares, l1_ratios=ratios)
    a, bb = cpu._inputs(oracle, A, b, d, w, p, lam, 1)
    exp = lpm.lasso_path(a, bb, d, w, p, N, ratios, lpm.RATIO)[0]
    assert beta == exp
    assert all(v == 0 for v in exp[-1]) and 0 < sum(v == 0 for v in exp[3]) < d


def test_parties_apart(lgc, oracle):
    """garbler and evaluator in one process through host buffers; an evaluator with another ratio list has another
    fingerprint (bin/linreg then refuses to run)"""
    rng = np.random.default_rng(9)
    w, p, d, N, P = 64, 56, 7, 6, 3
    A, b = synth_system(oracle, rng, 50, d, w, p)
    shares = split_shares(rng, A, b, P, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, 0.01, P, 1, 0, 0)
    ratios = [0.1, 0.4, 0.9]
    G = lgc.Party(sysm, lgc.GARBLER, seed=bytes(range(5, 21)), l1_ratios=ratios)
    E = lgc.Party(sysm, lgc.EVALUATOR, l1_ratios=ratios)
    assert G.program_fingerprint() == E.program_fingerprint()
    for other in ([0.1, 0.4, 0.8], [0.1, 0.4], ratios[:]):
        o = lgc.Party(sysm, lgc.EVALUATOR, **({"l1": other} if other == ratios else {"l1_ratios": other}))
        assert o.program_fingerprint() != E.program_fingerprint(), other      # other values, fewer values, the other mode
        o.close()
    for s in range(P):
        E.set_input_labels(s, G.encode_inputs(s, shares[s]))
    for k in range(G.num_launches):
        E.evaluate(k, G.garble(k))
    beta, _, _ = E.finish(G.decode_bits())
    G.close(); E.close()
    a, bb = cpu._inputs(oracle, A, b, d, w, p, 0.01, 1)
    assert beta.shape == (3, d) and beta.tolist() == lpm.lasso_path(a, bb, d, w, p, N, ratios, lpm.RATIO)[0]


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


def test_five_process_ratio_path_over_the_table_ring(tmp_path, golden_dir, oracle):
    """bin/linreg <file> 56 <party> lasso 40 0.001 --l1_ratios=... --table_ring: one 'L1 ratio:' line and one 'Result:' line
    per ratio, equal to the model"""
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    path, P = _readme(tmp_path, golden_dir)
    exe = os.path.join(HOST, "bin", "linreg")
    ratios = [1.0625, 0.5, 0.1]
    arg = "--l1_ratios=" + ",".join(str(r) for r in ratios)
    procs = [subprocess.Popen([exe, path, "56", str(k), "lasso", "40", "0.001", arg, "--table_ring"], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE) for k in range(1, P + 3)]
    outs = [q.communicate(timeout=300) for q in procs]
    assert all(q.returncode == 0 for q in procs), [e.decode()[-400:] for _, e in outs]
    lines = outs[1][0].decode().strip().splitlines()
    heads = [i for i, s in enumerate(lines) if s.startswith("L1 ratio: ")]
    assert [float(lines[i][len("L1 ratio: "):]) for i in heads] == ratios
    assert all(lines[i + 1].startswith("Result: ") for i in heads)
    inp = oracle.read_input(path)
    n, d, w, p = inp["n"], inp["d"], 64, 56
    A, b = oracle.aggregate(oracle.quantize(inp["X"], p, n, w), oracle.quantize(inp["y"], p, n, w), n, d, p, w)
    a, bb = cpu._inputs(oracle, A, b, d, w, p, 0.001, 1)
    exp = lpm.lasso_path(a, bb, d, w, p, 40, ratios, lpm.RATIO)[0]
    for i, e in zip(heads, exp):
        assert re.findall("-?[0-9]+\\.[0-9]+", lines[i + 1]) == ["%.15f" % (v / 2.0 ** p) for v in e]
    assert all(v == 0 for v in exp[0]) and len(set(map(tuple, exp))) == 3
