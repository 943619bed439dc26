"""Standard errors, residual variance and R^2 from the Cholesky solve (include/linreg_gc_inference.h) on the MI355X: the
co-located solver against the CPU checker and the model (tests/inference_model.py) with the kernel of every launch asserted from
the program; the inverse columns inside the Karatsuba shadow (d = 184, W = 64); division launches of d + 1 = 261 records on the
4-wave kernel (d = 260, W = 32); the two roles apart over the table ring with column batches cut at the table cap; bin/linreg
--inference end to end and the wrapper's parsing of it."""
import math
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import inference_model as im
import test_inference_cpu as cpu
import test_lasso_select_cpu as sel
from helpers import free_ports

pytestmark = pytest.mark.gpu

SEED = bytes(range(9, 25))
SE, FIT = im.SE, im.FIT
ROOT = sel.ROOT
HOST = os.path.join(ROOT, "linreg-mpc_amd", "host")
LAM = cpu.LAM


def _solve(lgc, sysm, shares, reveal, rs):
    s = lgc.Solver(sysm, seed=SEED, inference=cpu.SUBSETS[reveal], resid_scale=rs)
    s.set_shares(shares)
    s.run()
    u, s2, r2 = s.std_err_words(), s.sigma2_word(), s.r2_word()
    out = s.beta().tolist() + ([] if u is None else u.tolist()) + ([] if s2 is None else [s2, r2])
    s.close()
    return out


def _plain_solve(lgc, sysm, shares):
    """the plain Cholesky solve of the same (A, b) on the GPU"""
    s = lgc.Solver(sysm, seed=SEED)
    s.set_shares(np.ascontiguousarray(shares[:, :-1]))
    s.run()
    out = s.beta().tolist()
    s.close()
    return out


def _modes_by_size(lgc, prog):
    """the kernel of every launch, as the solver picks it: by record count, the multiply-accumulate kernels for their launches"""
    c = lgc.launch_constants()
    mg, me = lgc.RecordProgram.modes(prog)
    assert mg == me
    r = sel._recs(prog)
    for Lc, m in zip(prog.launches(), mg):
        n = Lc["nrec"]
        if r[Lc["first_rec"], 0] == cpu.OP_MACK:
            assert m == lgc.LM["mack"], (n, m)
            continue
        want = "split" if n <= c["split_max_recs"] else "wide" if n >= c["wide_launch"] else "quad2"
        if Lc["mac_only"] and m == lgc.LM["mac"]:           # (a large batch of plain products: the MAC kernel)
            assert n > c["split_max_recs"], (n, m)
            continue
        assert m == lgc.LM[want], (n, m, want)
    return mg


@pytest.mark.parametrize("d", [5, 33])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_solver_matches_checker_and_model(lgc, gccpu, oracle, w, p, d):
    """normalize = 1, SE + FIT, both roles on one GPU: every revealed word is the CPU checker's and the model's, beta is the
    plain Cholesky solve's run on the GPU here, and the floats of summary(n) follow from the words"""
    rng = np.random.default_rng(zlib.crc32(("gpu inference %d %d" % (w, d)).encode()))
    shares, X, _ = cpu.case(rng, d, w, p, 1)
    n = X.shape[0]
    rs = n / (n - d)
    sysm = lgc.make_system(d, w, p, "cholesky", 0, LAM, 2, 1, 0, 0)
    prog = cpu.program(lgc, sysm, SE | FIT, rs)
    mg = _modes_by_size(lgc, prog)
    r = sel._recs(prog)
    div = [(Lc["nrec"], m) for Lc, m in zip(prog.launches(), mg) if r[Lc["first_rec"], 0] == cpu.OP_DIV]
    assert div[:d] == [(d + 1, lgc.LM["split"])] * d        # a column's division launch: d + 1 records
    got = _solve(lgc, sysm, shares, SE | FIT, rs)
    assert got == cpu.shown(prog, sel.plain(gccpu, prog, w, p, shares), w, SE | FIT)
    m = im.inference(oracle, shares, d, w, p, LAM, rs, 1)
    assert got == im.revealed(m, SE | FIT) and any(got[:d]) and all(v > 0 for v in got[d:])
    assert got[:d] == _plain_solve(lgc, sysm, shares)
    s = lgc.Solver(sysm, seed=SEED, inference=("se", "fit"), resid_scale=rs)
    s.set_shares(shares)
    s.run()
    f = s.summary(n)
    s.close()
    assert f["std_err"].tolist() == [v / 2.0 ** p / math.sqrt(n) for v in m["u"]]
    assert (f["sigma2"], f["r2"]) == (m["s2"] / 2.0 ** p * d, m["r2"] / 2.0 ** p) and 0 < f["r2"] < 1


def test_one_column(lgc, gccpu, oracle):
    """d = 1: the factorisation has no dot product at all; the three reveal subsets"""
    w, p, d = 64, 56, 1
    rng = np.random.default_rng(17)
    shares, X, _ = cpu.case(rng, d, w, p, 1)
    rs = X.shape[0] / (X.shape[0] - d)
    sysm = lgc.make_system(d, w, p, "cholesky", 0, LAM, 2, 1, 0, 0)
    m = im.inference(oracle, shares, d, w, p, LAM, rs, 1)
    for reveal in (SE, FIT, SE | FIT):
        prog = cpu.program(lgc, sysm, reveal, rs)
        r = sel._recs(prog)
        first_div = int(np.nonzero(r[:, 0] == cpu.OP_DIV)[0][0])
        assert not np.isin(r[:first_div, 0], [cpu.OP_MAC, cpu.OP_MAC2, cpu.OP_MACK]).any()
        got = _solve(lgc, sysm, shares, reveal, rs)
        assert got == im.revealed(m, reveal) == cpu.shown(prog, sel.plain(gccpu, prog, w, p, shares), w, reveal)


def _big_case(d, w, p, seed):
    """a well-conditioned system of d columns, two shares, every word in range: on the two-party path, where v_j is the
    variance-inflation factor itself (on the data-provider path it is d times that, past seven integer bits at these d)"""
    rng = np.random.default_rng(seed)
    shares, X, _ = cpu.case(rng, d, w, p, 0, n=2 * d + 60)
    return shares, X.shape[0]


def test_karatsuba_shadow(lgc, gccpu):
    """d = 184, W = 64: the column batches hold OP_MACK records that read the inverse columns through the one shadow (asserted;
    the plain-product fallback was not taken), on the Karatsuba MAC kernel.  Bit-exact against the CPU checker, beta against
    the plain solve on the GPU.  Measured on the MI355X: 1.51 s on the device (16.7 G AND gates), 4.1 s for the whole test"""
    d, w, p = 184, 64, 56
    shares, n = _big_case(d, w, p, 184)
    rs = n / (n - d)
    sysm = lgc.make_system(d, w, p, "cholesky", 0, LAM, 2, 0, 0, 0)
    prog = cpu.program(lgc, sysm, SE | FIT, rs)
    r = sel._recs(prog)
    z_div = r[(r[:, 0] == cpu.OP_DIV) & (r[:, 2] == r[:, 3]) & (r[:, 5] == 0)]
    Z0, Z1 = int(z_div[:, 2].min()) - 1, int(z_div[:, 2].max()) + 1 + d
    mack = r[r[:, 0] == cpu.OP_MACK]
    assert ((mack[:, 4] >= Z0) & (mack[:, 4] < Z1)).sum() > d and (z_div[:, 1] == 2).all()
    mg, me = lgc.RecordProgram.modes(prog)
    assert mg == me and {m for Lc, m in zip(prog.launches(), mg) if r[Lc["first_rec"], 0] == cpu.OP_MACK} == {lgc.LM["mack"]}
    want = cpu.shown(prog, sel.plain(gccpu, prog, w, p, shares), w, SE | FIT)
    got = _solve(lgc, sysm, shares, SE | FIT, rs)
    assert got == want and any(got[:d]) and all(v > 0 for v in got[d:])
    assert got[:d] == _plain_solve(lgc, sysm, shares)


def test_division_launches_on_the_four_wave_kernel(lgc, gccpu):
    """d = 260, W = 32: every division launch of the factorisation has d + 1 = 261 records, past split_max_recs = 256, and runs
    on the 4-wave kernel where the plain solve's d - j records stay on the column-split kernel from column 4 on.  Bit-exact
    against the CPU checker.  Measured on the MI355X: 1.41 s on the device (13.3 G AND gates in 2 315 launches), 3.2 s for the
    whole test with the CPU checker's run of the program -- a few seconds, so d stays at 260"""
    d, w, p = 260, 32, 24
    shares, n = _big_case(d, w, p, 260)
    rs = n / (n - d)
    sysm = lgc.make_system(d, w, p, "cholesky", 0, LAM, 2, 0, 0, 0)
    prog = cpu.program(lgc, sysm, SE | FIT, rs)
    c = lgc.launch_constants()
    assert c["split_max_recs"] < d + 1 < c["wide_launch"]
    r = sel._recs(prog)
    mg, me = lgc.RecordProgram.modes(prog)
    div = [(Lc["nrec"], g, e) for Lc, g, e in zip(prog.launches(), mg, me) if r[Lc["first_rec"], 0] == cpu.OP_DIV]
    assert div[:d] == [(d + 1, lgc.LM["quad2"], lgc.LM["quad2"])] * d
    want = cpu.shown(prog, sel.plain(gccpu, prog, w, p, shares), w, SE | FIT)
    got = _solve(lgc, sysm, shares, SE | FIT, rs)
    assert got == want and any(got[:d]) and all(v > 0 for v in got[d:])


def test_roles_apart_over_the_table_ring_with_cut_batches(lgc, gccpu, oracle):
    """d = 33, W = 64, the two roles as separate parties, the garbler writing into its table ring (three slots, reused) and the
    evaluator reading every launch's tables from it; max_launch_table_bytes = 64 MiB (2^15 gate steps) cuts the larger column
    batches (up to 80 883 steps co-located) into several launches.  Bit-exact; the fingerprint covers the reveal bits and
    q(resid_scale)"""
    d, w, p, reveal = 33, 64, 56, SE | FIT
    rng = np.random.default_rng(33)
    shares, X, _ = cpu.case(rng, d, w, p, 1)
    rs = X.shape[0] / (X.shape[0] - d)
    sysm = lgc.make_system(d, w, p, "cholesky", 0, LAM, 2, 1, 0, 0)
    prog = cpu.program(lgc, sysm, reveal, rs)
    want = im.revealed(im.inference(oracle, shares, d, w, p, LAM, rs, 1), reveal)
    cap = 1 << 26
    assert max(Lc["steps"] for Lc in prog.launches() if Lc["mac_only"]) * 2048 > cap
    kw = dict(inference=("se", "fit"), resid_scale=rs)
    G = lgc.Party(sysm, lgc.GARBLER, seed=bytes(range(5, 21)), max_launch_table_bytes=cap, **kw)
    E = lgc.Party(sysm, lgc.EVALUATOR, max_launch_table_bytes=cap, **kw)
    assert G.num_launches == E.num_launches > prog.info.n_launches               # column batches are cut
    assert max(G.table_bytes(k) for k in range(G.num_launches)) <= cap
    assert G.input_bits == (d * (d + 1) // 2 + d + 1) * w
    assert G.program_fingerprint() == E.program_fingerprint()
    for other in (dict(inference=("se",), resid_scale=rs), dict(inference=("fit",), resid_scale=rs), dict(inference=("se", "fit"), resid_scale=rs * 1.5)):
        o = lgc.Party(sysm, lgc.EVALUATOR, max_launch_table_bytes=cap, **other)
        assert o.program_fingerprint() != E.program_fingerprint()
        o.close()
    for s in range(2):
        E.set_input_labels(s, G.encode_inputs(s, shares[s]))
    G.ring_create(3)
    for k in range(G.num_launches):
        G.garble_ring(k)
        nb = G.table_bytes(k)
        E.evaluate(k, G.test_ring_read(k, nb) if nb else np.zeros(0, dtype=np.uint8))
    beta, _, _ = E.finish(G.decode_bits())
    got = beta.tolist() + E.std_err_words().tolist() + [E.sigma2_word(), E.r2_word()]
    G.close(); E.close()
    assert got == want


# ---- bin/linreg end to end
W, P = 64, 56
ARGS = ["cholesky", "0", "0.001"]


def _readme(tmp_path, golden_dir):
    tok = open(os.path.join(golden_dir, "readme_example.in")).read().split("\n")
    n, d, P_ = map(int, tok[0].split())
    ports = free_ports(P_ + 2)
    for i in range(P_ + 2):
        parts = tok[1 + i].split()
        parts[0] = "127.0.0.1:%d" % ports[i]
        tok[1 + i] = " ".join(parts)
    path = str(tmp_path / "readme.in")
    open(path, "w").write("\n".join(tok))
    return path, n, d, P_


def _run(exe, path, P_, extra):
    """the five processes; the TI seed is pinned as the host tests pin it, so that both runs share their phase-1 randomness"""
    env = dict(os.environ, LINREG_TI_SEED="000102030405060708090a0b0c0d0e0f")
    procs = [subprocess.Popen([exe, path, str(P), str(k)] + ARGS + extra + ["--table_ring"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
             for k in range(1, P_ + 3)]
    try:
        outs = [q.communicate(timeout=240) for q in procs]
    finally:
        for q in procs:
            if q.poll() is None:
                q.kill()
    assert all(q.returncode == 0 for q in procs), [e.decode()[-400:] for _, e in outs]
    return outs[1][0].decode().rstrip("\n").splitlines()


def test_bin_linreg_end_to_end(lgc, oracle, tmp_path, golden_dir):
    """five processes on the README example, cholesky with --inference: the Result line is the run's without --inference, and the
    two lines after it are the model's on the system phase 1 sums to (the oracle's aggregation of the same input, yy = the
    integer sum of y_q^2), in double after the division by sqrt(n); the wrapper's parser reads them"""
    path, n, d, P_ = _readme(tmp_path, golden_dir)
    subprocess.run(["make", "-C", HOST], stdout=subprocess.DEVNULL, check=True, timeout=300)
    exe = os.path.join(HOST, "bin", "linreg_testhooks")
    plain = _run(exe, path, P_, [])
    lines = _run(exe, path, P_, ["--inference"])
    res = [l for l in lines if l.startswith("Result:")]
    assert len(res) == 1 and res == [l for l in plain if l.startswith("Result:")] and plain[-1] == res[0]
    assert lines[-3] == res[0] and lines[-2].startswith("Standard errors:") and lines[-1].startswith("Residual variance:")
    assert "A = " not in "\n".join(lines) and "A = " in "\n".join(plain)           # Y stays hidden, and with it the inputs
    inp = oracle.read_input(os.path.join(golden_dir, "readme_example.in"))
    Xq, yq = oracle.quantize(inp["X"], P, n, W), oracle.quantize(inp["y"], P, n, W)
    A, b = oracle.aggregate(Xq, yq, n, d, P, W)
    yy = sum(int(v) * int(v) for v in yq) & ((1 << W) - 1)
    one = np.concatenate([A, b, np.array([yy], dtype=np.uint64)]).astype(np.uint64)[None, :]
    m = im.inference(oracle, one, d, W, P, 0.001, n / (n - d), 1)
    assert re.findall("-?[0-9]+\\.[0-9]+", res[0]) == ["%.15f" % (v / 2.0 ** P) for v in m["beta"]]
    assert lines[-2] == "Standard errors: " + "".join("%20.15f " % (v / 2.0 ** P / math.sqrt(n)) for v in m["u"])
    assert lines[-1] == "Residual variance: %.15f R^2: %.15f" % (m["s2"] / 2.0 ** P * d, m["r2"] / 2.0 ** P)
    import mpc_linear_regression as mw
    se, s2, r2 = mw.parse_inference_lines(lines)
    assert len(se) == d and all(v > 0 for v in se) and s2 > 0 and 0 < r2 < 1 and mw.parse_result_line(res[0]) == mw.parse_result_line(plain[-1])
    no_se = _run(exe, path, P_, ["--inference", "--no_se"])
    assert no_se[-2] == res[0] and no_se[-1] == lines[-1] and not any(l.startswith("Standard errors:") for l in no_se)
    assert mw.parse_inference_lines(no_se) == (None, s2, r2)


# ---- the wrapper
def _fit_side(own, other, csv_path, spec, args, q):
    """one MPCLinearRegression.fit() in its own process; keeps the MPC input file it wrote"""
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
    q.put((spec, r.result, kept["text"], r.std_errors, r.sigma2, r.r2))


def test_wrapper_fills_the_inference_fields(tmp_path, oracle):
    """two wrapper instances on localhost with --inference in mpc_args: the side that runs the Evaluator parses the Result line
    (no longer the last one) and fills .std_errors, .sigma2 and .r2 -- in studentised units -- with the model's values on the
    combined data set; the peer receives the coefficients as ever"""
    import multiprocessing as mp
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(3)
    n = 60
    age = rng.integers(20, 70, n).astype(float); sex = rng.integers(0, 2, n)
    height = 1.5 + 0.4 * rng.random(n); weight = 50 + 40 * rng.random(n)
    income = 800 + 35 * age + 400 * sex + 900 * height - 3 * weight + 50 * rng.standard_normal(n)
    csvf = tmp_path / "people.csv"
    with open(csvf, "w") as f:
        f.write("age;sex;height;weight;income\n")
        for i in range(n):
            f.write("%r;%s;%r;%r;%r\n" % (float(age[i]), "mw"[1 - int(sex[i])], float(height[i]), float(weight[i]), float(income[i])))
    base = free_ports(1)[0]
    a_ip, b_ip = "127.0.0.1:%d" % base, "127.0.0.1:%d" % (base + 100)
    args = ["56", "cholesky", "0", "0.001", "--inference"]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    pa = ctx.Process(target=_fit_side, args=(a_ip, b_ip, str(csvf), "0 c1", args, q))          # age, sex
    pb = ctx.Process(target=_fit_side, args=(b_ip, a_ip, str(csvf), "2 3 r4", args, q))        # height, weight, income
    pa.start(); pb.start()
    try:
        outs = dict((o[0], o[1:]) for o in (q.get(timeout=120), q.get(timeout=120)))
    finally:
        pa.join(20); pb.join(20)
        for pr in (pa, pb):
            if pr.is_alive():
                pr.kill()
    assert pa.exitcode == 0 and pb.exitcode == 0
    res_a, file_a, se_a, s2_a, r2_a = outs["0 c1"]
    res_b, file_b, se_b, s2_b, r2_b = outs["2 3 r4"]
    d = 4
    assert res_a == res_b and len(res_b) == d and (se_a, s2_a, r2_a) == (None, None, None)
    ta, tb = file_a.split("\n"), file_b.split("\n")
    rows = [ra.split()[:2] + rb.split()[2:] for ra, rb in zip(ta[6:6 + n], tb[6:6 + n])]
    comb = tmp_path / "combined.in"
    comb.write_text("\n".join(ta[:6] + [" ".join(r) for r in rows] + tb[6 + n:]))
    inp = oracle.read_input(str(comb))
    Xq, yq = oracle.quantize(inp["X"], P, n, W), oracle.quantize(inp["y"], P, n, W)
    A, b = oracle.aggregate(Xq, yq, n, d, P, W)
    yy = sum(int(v) * int(v) for v in yq) & ((1 << W) - 1)
    m = im.inference(oracle, np.concatenate([A, b, np.array([yy], dtype=np.uint64)]).astype(np.uint64)[None, :], d, W, P, 0.001, n / (n - d), 1)
    fl = lambda v: float("%.15f" % v)
    assert res_b == [fl(v / 2.0 ** P) for v in m["beta"]]
    assert se_b == [fl(v / 2.0 ** P / math.sqrt(n)) for v in m["u"]]
    assert (s2_b, r2_b) == (fl(m["s2"] / 2.0 ** P * d), fl(m["r2"] / 2.0 ** P))
    # and they are the least-squares quantities of the studentised data, to the accuracy of phase 1's quantisation
    X = np.array([[float(v) for v in r] for r in rows]); y = np.array([float(v) for v in tb[6 + n + 1].split()])
    lam = 0.001 * d
    beta = np.linalg.solve(X.T @ X / n + lam * np.eye(d), X.T @ y / n)
    res = y - X @ beta
    s2 = float(res @ res) / (n - d)
    assert np.allclose(se_b, np.sqrt(s2 * np.diag(np.linalg.inv(X.T @ X + n * lam * np.eye(d)))), rtol=1e-5)
    assert abs(s2_b / s2 - 1) < 1e-5 and abs(r2_b - (1 - float(res @ res) / float(y @ y))) < 1e-6
