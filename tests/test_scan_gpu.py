"""The association scan (include/linreg_gc_scan.h) on the MI355X: the co-located solver against the CPU checker and the model
(tests/scan_model.py) with the kernel of every launch asserted from the program -- M-record launches on the column-split, the
4-wave and the wide kernel --; the two roles apart over the table ring with an M-record launch cut at the table cap; beta_m
against the plain Cholesky solve of the augmented system, run on the GPU."""
import math
import zlib

import numpy as np
import pytest

import scan_model as sm
import test_inference_gpu as ig
import test_lasso_select_cpu as sel
import test_scan_cpu as cpu

pytestmark = pytest.mark.gpu

SEED = bytes(range(9, 25))
LAM = cpu.LAM


def _solve(lgc, sysm, shares, M, se, rs):
    s = lgc.Solver(sysm, seed=SEED, scan=M, scan_se=bool(se), resid_scale=rs if se else None)
    s.set_shares(shares)
    s.run()
    w = s.scan_std_err_words()
    out = s.beta().tolist() + ([] if w is None else w.tolist())
    s.close()
    return out


@pytest.mark.parametrize("c,M", [(1, 1), (5, 40)])
@pytest.mark.parametrize("w,p", cpu.WIDTHS)
def test_solver_matches_checker_and_model(lgc, gccpu, oracle, w, p, c, M):
    """normalize = 1, with the standard errors, both roles on one GPU: every revealed word is the CPU checker's and the model's;
    without them the coefficients are the same words; the floats of scan_summary(n) follow from the words"""
    rng = np.random.default_rng(zlib.crc32(("gpu scan %d %d %d" % (w, c, M)).encode()))
    shares, _, X, _ = cpu.case(rng, c, M, w, p, 1, nshares=2)
    n, rs = X.shape[0], cpu.resid(X, c)
    sysm = lgc.make_system(c + 1, w, p, "cholesky", 0, LAM, 2, 1, 0, 0)
    prog = cpu.program(lgc, sysm, M, 1, rs)
    ig._modes_by_size(lgc, prog)
    got = _solve(lgc, sysm, shares, M, 1, rs)
    assert got == cpu.shown(prog, sel.plain(gccpu, prog, w, p, shares), w, M, 1)
    m = sm.scan(oracle, shares, c, M, w, p, LAM, rs, 1)
    assert got == sm.revealed(m, 1) and any(got[:M]) and all(v > 0 for v in got[M:])
    assert _solve(lgc, sysm, shares, M, 0, None) == got[:M]
    s = lgc.Solver(sysm, seed=SEED, scan=M, scan_se=True, resid_scale=rs)
    s.set_shares(shares)
    s.run()
    f = s.scan_summary(n)
    st = s.stats()
    s.close()
    assert f["beta"].tolist() == [v / 2.0 ** p for v in m["beta"]]
    assert f["std_err"].tolist() == [v / 2.0 ** p / math.sqrt(n) for v in m["w"]]
    assert st["and_gates"] == prog.info.total_gates and st["launches"] == prog.info.n_launches and st["seconds_total"] > 0


@pytest.mark.parametrize("M,kernel", [(300, "quad2"), (600, "wide")])
def test_m_record_launches_on_every_kernel(lgc, gccpu, oracle, M, kernel):
    """c = 2, W = 32: the launches of M (or a few more) records -- a column's divisions, the candidates' square roots, the
    tail's divisions and products -- run on the 4-wave kernel at M = 300 (past split_max_recs) and on the wide kernel at M = 600
    (wide_launch and more), where (5, 40) above keeps them on the column-split kernel.  Bit-exact against the CPU checker and the
    model"""
    w, p, c = 32, 24, 2
    rng = np.random.default_rng(M)
    shares, _, X, _ = cpu.case(rng, c, M, w, p, 1, nshares=2)
    rs = cpu.resid(X, c)
    sysm = lgc.make_system(c + 1, w, p, "cholesky", 0, LAM, 2, 1, 0, 0)
    prog = cpu.program(lgc, sysm, M, 1, rs)
    k = lgc.launch_constants()
    assert (k["split_max_recs"] < M < k["wide_launch"]) if kernel == "quad2" else M >= k["wide_launch"]
    mg = ig._modes_by_size(lgc, prog)
    r = sel._recs(prog)
    by_op = {}
    for Lc, mode in zip(prog.launches(), mg):
        if M <= Lc["nrec"] <= M + c + 1 and not Lc["mac_only"]:
            by_op.setdefault(int(r[Lc["first_rec"], 0]), set()).add(mode)
    assert by_op[cpu.OP_DIV] == by_op[cpu.OP_SQRT] == by_op[cpu.OP_MUL] == {lgc.LM[kernel]}, by_op
    got = _solve(lgc, sysm, shares, M, 1, rs)
    assert got == cpu.shown(prog, sel.plain(gccpu, prog, w, p, shares), w, M, 1)
    assert got == sm.revealed(sm.scan(oracle, shares, c, M, w, p, LAM, rs, 1), 1)


def test_roles_apart_over_the_table_ring_with_a_cut_launch(lgc, oracle):
    """c = 5, M = 40, W = 64, the two roles as separate parties, the garbler writing into its table ring (three slots, reused)
    and the evaluator reading every launch's tables from it; max_launch_table_bytes = 32 MiB (2^14 gate steps) cuts the M-record
    division launches (40 dividers of 64 bits are far more steps than that) into several.  Bit-exact; the fingerprint covers M,
    the reveal bits and q(resid_scale)"""
    c, M, w, p = 5, 40, 64, 56
    rng = np.random.default_rng(40)
    shares, _, X, _ = cpu.case(rng, c, M, w, p, 1, nshares=2)
    rs = cpu.resid(X, c)
    sysm = lgc.make_system(c + 1, w, p, "cholesky", 0, LAM, 2, 1, 0, 0)
    prog = cpu.program(lgc, sysm, M, 1, rs)
    want = sm.revealed(sm.scan(oracle, shares, c, M, w, p, LAM, rs, 1), 1)
    cap = 1 << 25
    r = sel._recs(prog)
    big = [Lc for Lc in prog.launches() if Lc["nrec"] >= M and r[Lc["first_rec"], 0] == cpu.OP_DIV]
    assert big and min(Lc["steps"] for Lc in big) * 2048 > cap
    kw = dict(scan=M, scan_se=True, resid_scale=rs)
    G = lgc.Party(sysm, lgc.GARBLER, seed=bytes(range(5, 21)), max_launch_table_bytes=cap, **kw)
    E = lgc.Party(sysm, lgc.EVALUATOR, max_launch_table_bytes=cap, **kw)
    assert G.num_launches == E.num_launches > prog.info.n_launches               # M-record launches are cut
    assert max(G.table_bytes(k) for k in range(G.num_launches)) <= cap
    assert G.input_bits == sm.in_words(c, M) * w
    assert G.program_fingerprint() == E.program_fingerprint()
    for other in (dict(scan=M), dict(scan=M + 1, scan_se=True, resid_scale=rs), dict(scan=M, scan_se=True, resid_scale=rs * 1.5)):
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
    got = beta.tolist() + E.scan_std_err_words().tolist()
    n = X.shape[0]
    assert E.scan_summary(n)["std_err"].tolist() == [v / 2.0 ** p / math.sqrt(n) for v in want[M:]]
    G.close(); E.close()
    assert got == want


def test_beta_is_the_plain_gpu_solve_of_the_augmented_system(lgc):
    """three candidates of a (c, M) = (5, 40) scan: beta_m is the last coefficient of the plain Cholesky solve of [C, g_m], both
    run on the GPU"""
    c, M, w, p = 5, 40, 64, 56
    rng = np.random.default_rng(3)
    shares, tot, _, _ = cpu.case(rng, c, M, w, p, 1, nshares=2)
    sysm = lgc.make_system(c + 1, w, p, "cholesky", 0, LAM, 2, 1, 0, 0)
    got = _solve(lgc, sysm, shares, M, 0, None)
    for m in (0, 17, 39):
        s = lgc.Solver(sysm, seed=SEED)
        s.set_shares(cpu.split(rng, sm.augmented_words(tot, c, M, m)[:-1], 2, w))
        s.run()
        assert int(s.beta()[c]) == got[m], m
        s.close()
