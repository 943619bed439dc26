"""In-circuit K-fold cross-validation of the ridge lambda sweep (include/linreg_gc_ridge_cv.h) on the MI355X: a small solve of
the co-located solver against the CPU checker and the model (tests/ridge_cv_model.py), with the kernel of every launch asserted
from the program; Karatsuba products of merged circuits over several systems in one launch, co-located and with the roles
apart and the launch cut at the table cap; beta* against the existing single solve on the GPU; bin/linreg end to end."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import lasso_model as lm
import ridge_cv_model as rcm
import test_lasso_select_cpu as sel
import test_ridge_cv_cpu as cpu
from helpers import free_ports

pytestmark = pytest.mark.gpu

SEED = bytes(range(9, 25))
INDEX, SCORES = rcm.REVEAL_INDEX, rcm.REVEAL_SCORES
ROOT = sel.ROOT
HOST = os.path.join(ROOT, "linreg-mpc_amd", "host")


def _kw(K, lambdas, flags):
    return dict(lambdas=list(lambdas), folds=K, reveal_index=bool(flags & INDEX), reveal_scores=bool(flags & SCORES))


def _solve(lgc, sysm, shares, **kw):
    s = lgc.Solver(sysm, seed=SEED, **kw)
    s.set_shares(shares)
    s.run()
    assert lgc.lib().lgc_solver_num_folds(s._h) == kw["folds"]
    lgc.lib().lgc_solver_num_circuits.restype = lgc.C.c_size_t
    lgc.lib().lgc_solver_num_circuits.argtypes = [lgc.C.c_void_p]
    assert lgc.lib().lgc_solver_num_circuits(s._h) == len(kw["lambdas"])
    if sysm.algorithm == lgc.ALG["cgd"]:
        gates, secs = s.iterations()
        assert len(gates) == sysm.num_iterations and (np.diff(gates.astype(np.int64)) > 0).all() and (np.diff(secs) >= 0).all()
    out = s.beta().tolist(), s.selected_index(), s.scores()
    s.close()
    return out


@pytest.mark.parametrize("alg,N", [("cgd", 4), ("cholesky", 0)])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_small_solve_matches_checker_and_model(lgc, gccpu, oracle, w, p, alg, N):
    """d = 6, K = 3, L = 4 (W = 32 cholesky: L = 5, whose largest merged batch of 270 dual records is the one that leaves the
    column-split kernel), both roles on one GPU.  Every launch of records other than products runs on the column-split kernel
    or, the (K + 1) L d^2 mirror copies, on the wide kernel; the merged dot products of the solvers run on the column-split
    (<= 256 records), the 4-wave and -- W = 64, L = 4: 576 records -- the wide kernel.  Covered in every case: column-split
    and 4-wave; the modes are asserted from the program.  Every revealed word is the CPU checker's and the model's, with the
    reveal flags and without them"""
    d, K, flags = 6, 3, INDEX | SCORES
    L = 5 if (w, alg) == (32, "cholesky") else 4
    lams = [0.05, 0.001, 0.2, 0.01, 0.5][:L]
    rng = np.random.default_rng(zlib.crc32(("gpu ridge cv %d %s" % (w, alg)).encode()))
    shares, per = cpu.case(rng, d, K, w, p)
    sysm = lgc.make_system(d, w, p, alg, N, 0.3, 2, 1, 0, 0)
    prog = lgc.Program(sysm, **_kw(K, lams, flags))
    c = lgc.launch_constants()
    mg, me = lgc.RecordProgram.modes(prog)                  # (the kernel of every launch, as the solver picks it)
    assert mg == me
    for Lc, m in zip(prog.launches(), mg):
        n = Lc["nrec"]
        want = "split" if n <= c["split_max_recs"] else "wide" if n >= c["wide_launch"] else "quad2"
        assert m == lgc.LM[want], (n, m)
    mac_modes = {m for Lc, m in zip(prog.launches(), mg) if Lc["mac_only"]}
    assert {lgc.LM["split"], lgc.LM["quad2"]} <= mac_modes, mac_modes
    beta, idx, cv = _solve(lgc, sysm, shares, **_kw(K, lams, flags))
    assert beta + [idx] + cv.tolist() == sel.shown(prog, cpu.run_plain(gccpu, prog, w, p, shares)[0], w, flags, L)
    best, want, sc, _, _ = rcm.ridge_cv(oracle, per, d, w, p, alg, N, lams, 1)
    assert (beta, idx, cv.tolist()) == (best, want, sc) and any(beta)
    beta0, idx0, cv0 = _solve(lgc, sysm, shares, **_kw(K, lams, 0))
    assert beta0 == best and idx0 == -1 and cv0 is None
    # the existing single solve on the assembled full system at l* (normalize = 0, a zero second share), on the GPU too
    _, train = rcm.systems(per, d, w, 1)
    m = (1 << w) - 1
    one = np.zeros((2, d * (d + 1) // 2 + d), dtype=np.uint64)
    one[0] = [int(v) & m for v in rcm.with_lambda(train[K][0], d, w, lm.to_fixed(lams[idx], p, w)) + list(train[K][1])]
    s = lgc.Solver(lgc.make_system(d, w, p, alg, N, 0.0, 2, 0, 0, 0), seed=SEED)
    s.set_shares(one)
    s.run()
    assert s.beta().tolist() == beta
    s.close()


def _smallest_karatsuba_d(lgc, K, lams, N):
    """the smallest d whose merged program holds OP_MACK records: d^2 must exceed kTargetWaves / circuits = 8192 / 6 products"""
    for d in range(30, 48):
        prog = lgc.Program(lgc.make_system(d, 64, 56, "cgd", N, 0.0, 2, 1, 0, 0), **_kw(K, lams, 0))
        if (sel._recs(prog)[:, 0] == sel.OP_MACK).any():
            return d
    raise AssertionError("no Karatsuba records up to d = 47")


@pytest.mark.parametrize("cut", [False, True])
def test_karatsuba_products_of_merged_circuits_share_a_launch(lgc, gccpu, cut):
    """K = 2, L = 2, cgd with N = 2, W = 64 at the smallest d with OP_MACK records (37): every matrix-vector launch holds the
    Karatsuba records of all (K + 1) L = 6 circuits -- three different systems, two values of lambda each -- and runs on the
    Karatsuba MAC kernel; the scoring tail's batches read beta across the circuits' word strides.  cut: the two roles apart
    with max_launch_table_bytes lowered so that a merged launch is cut into several at the table cap.  Bit-exact against the
    CPU checker"""
    w, p, K, L, N, flags = 64, 56, 2, 2, 2, INDEX | SCORES
    lams = [0.5, 0.01]
    d = _smallest_karatsuba_d(lgc, K, lams, N)
    assert d == 37
    rng = np.random.default_rng(d)
    shares, _ = cpu.case(rng, d, K, w, p, rows=d + 30)
    sysm = lgc.make_system(d, w, p, "cgd", N, 0.0, 2, 1, 0, 0)
    kw = _kw(K, lams, flags)
    prog = lgc.Program(sysm, **kw)
    want = sel.shown(prog, cpu.run_plain(gccpu, prog, w, p, shares)[0], w, flags, L)
    assert any(want[:d]) and len(set(want[d + 1:])) == L

    recs, info = sel._recs(prog), prog.info
    mg, me = lgc.RecordProgram.modes(prog)
    mk = [(recs[Lc["first_rec"]:Lc["first_rec"] + Lc["nrec"]], m, e) for Lc, m, e in zip(prog.launches(), mg, me) if recs[Lc["first_rec"], 0] == sel.OP_MACK]
    assert len(mk) == N
    for r, m, e in mk:
        assert (r[:, 0] == sel.OP_MACK).all() and m == e == lgc.LM["mack"]
        circ = {(int(a) - info.shared_end) // info.word_stride for a in r[:, 3]}        # the circuit whose matrix a record reads
        assert circ == set(range((K + 1) * L)) and {t // L for t in circ} == set(range(K + 1))
        assert int(r[:, 1].sum()) == (K + 1) * L * d * d
    tail = recs[cpu.tail_start(prog):]
    mac = tail[tail[:, 0] == cpu.OP_MAC]
    read = {(int(x) - info.shared_end) // info.word_stride for x in np.concatenate([mac[:, 3], mac[:, 4]])}
    assert {t for t in read if t < (K + 1) * L} == set(range(K * L))           # beta of every fold fit, at its circuit's stride
    if not cut:
        s = lgc.Solver(sysm, seed=SEED, **kw)
        s.set_shares(shares)
        s.run()
        got = s.beta().tolist() + [s.selected_index()] + s.scores().tolist()
        s.close()
        assert got == want
        return
    cap = 1 << 28                                                            # 256 MiB of tables: 2^17 gate steps per launch
    G = lgc.Party(sysm, lgc.GARBLER, seed=bytes(range(5, 21)), max_launch_table_bytes=cap, **kw)
    E = lgc.Party(sysm, lgc.EVALUATOR, max_launch_table_bytes=cap, **kw)
    assert G.num_launches == E.num_launches > info.n_launches + 2               # the merged launches are cut
    assert max(G.table_bytes(k) for k in range(G.num_launches)) <= cap
    assert G.program_fingerprint() == E.program_fingerprint()
    for other in (_kw(3, lams, flags), _kw(K, [0.5, 0.02], flags), _kw(K, lams, INDEX)):
        o = lgc.Party(sysm, lgc.EVALUATOR, max_launch_table_bytes=cap, **other)
        assert o.program_fingerprint() != E.program_fingerprint()
        o.close()
    assert lgc.lib().lgc_party_num_folds(E._h) == K
    for s in range(2):
        E.set_input_labels(s, G.encode_inputs(s, shares[s]))
    buf = lgc.host_alloc(cap)                                               # one page-locked buffer for every launch's tables
    for k in range(G.num_launches):
        lgc._chk(lgc.lib().lgc_party_garble(G._h, k, lgc._vp(buf)))
        lgc._chk(lgc.lib().lgc_party_evaluate(E._h, k, lgc._vp(buf) if G.table_bytes(k) else None))
    beta, _, _ = E.finish(G.decode_bits())
    got = beta.tolist() + [E.selected_index()] + E.scores().tolist()
    assert lgc.lib().lgc_party_selected_index(G._h) == -1                      # the garbler learns nothing
    G.close(); E.close()
    lgc.host_free(buf)
    assert got == want


# ---- bin/linreg end to end
W, P, N, K = 64, 56, 10, 2
GRID = [0.1, 0.001, 0.01]
ARGS = ["cgd", str(N), "0.001", "--lambdas=0.1,0.001,0.01", "--folds=%d" % K, "--reveal_index"]


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
    return path, P_


def _expected(lgc, oracle, golden_dir, tmp):
    """(the fold systems as one (1, K (T + d)) share, beta*, l*) of the README input cut into K contiguous row folds: each fold's
    rows go to a file of their own, the oracle quantises them with that file's row count and sums phase 1 (as
    tests/test_folds_host_gpu.py does for the lasso)"""
    tok = open(os.path.join(golden_dir, "readme_example.in")).read().split("\n")
    n, d, P_ = map(int, tok[0].split())
    rows, ys = tok[2 + P_ + 2:2 + P_ + 2 + n], tok[2 + P_ + 2 + n + 1].split()
    per = []
    for k in range(K):
        r0, r1 = lgc.fold_rows(n, K, k)
        path = str(tmp / ("fold%d.in" % k))
        head = ["%d %d %d" % (r1 - r0, d, P_)] + tok[1:1 + P_ + 2]
        open(path, "w").write("\n".join(head + ["%d %d" % (r1 - r0, d)] + rows[r0:r1] + ["%d" % (r1 - r0), " ".join(ys[r0:r1]), ""]))
        inp = oracle.read_input(path)
        assert (inp["n"], inp["d"]) == (r1 - r0, d)
        A, b = oracle.aggregate(oracle.quantize(inp["X"], P, inp["n"], W), oracle.quantize(inp["y"], P, inp["n"], W), inp["n"], d, P, W)
        per.append(np.concatenate([A, b]).astype(np.uint64)[None, :])
    beta, best, _, _, _ = rcm.ridge_cv(oracle, per, d, W, P, "cgd", N, GRID, 1)
    return np.hstack(per), beta, best, d, P_


def test_bin_linreg_end_to_end(lgc, oracle, tmp_path, golden_dir):
    """five processes, phase 1 once per contiguous row fold, the cross-validated sweep over the table ring: one Result line, the
    model's beta* and l* on the same per-fold phase-1 results; the same fold systems through the co-located solver"""
    system, beta, best, d, P_ = _expected(lgc, oracle, golden_dir, tmp_path)
    path, _ = _readme(tmp_path, golden_dir)
    subprocess.run(["make", "-C", HOST], stdout=subprocess.DEVNULL, check=True, timeout=300)
    exe = os.path.join(HOST, "bin", "linreg")
    procs = [subprocess.Popen([exe, path, str(P), str(k)] + ARGS + ["--table_ring"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
             for k in range(1, P_ + 3)]
    try:
        outs = [q.communicate(timeout=240) for q in procs]
    finally:
        for q in procs:
            if q.poll() is None:
                q.kill()
    assert all(q.returncode == 0 for q in procs), [e.decode()[-400:] for _, e in outs]
    ev = outs[1][0].decode()
    lines = ev.strip().splitlines()
    assert lines[-1].startswith("Result:") and sum(l.startswith("Result:") for l in lines) == 1
    assert re.findall("-?[0-9]+\\.[0-9]+", lines[-1]) == ["%.15f" % (v / 2.0 ** P) for v in beta]
    assert [l for l in lines if l.startswith("Selected index:")] == ["Selected index: %d (lambda: %.17g)" % (best, GRID[best])]
    assert "Folds: %d" % K in lines and "Algorithm: cgd" in ev and "A = " not in ev and "Lambda:" not in ev
    assert len(set(beta)) > 1
    import mpc_linear_regression as m
    assert m.parse_selected_line(lines) == (best, GRID[best]) and len(m.parse_result_line(lines[-1])) == d
    sysm = lgc.make_system(d, W, P, "cgd", N, 0.001, 1, 1, 0, 0)
    s = lgc.Solver(sysm, seed=bytes(range(16)), lambdas=GRID, folds=K, reveal_index=True)
    s.set_shares(system)
    s.run()
    assert (s.beta().tolist(), s.selected_index()) == (beta, best)
    s.close()
