"""In-circuit K-fold cross-validation of a lasso path (include/linreg_gc_lasso_cv.h) on the MI355X: a small solve of the
co-located solver -- column-split launches but for its dot products, which run as wide and 4-wave launches -- against the CPU
checker and the model (tests/lasso_cv_model.py); the Karatsuba launch shapes the
lowering adds -- batches that span several matrices under one shadow, cut at the table cap; the two roles apart."""
import zlib

import numpy as np
import pytest

import lasso_cv_model as lcm
import test_lasso_cv_cpu as cpu
import test_lasso_select_cpu as sel

pytestmark = pytest.mark.gpu

SEED = bytes(range(9, 25))
INDEX, SCORES = lcm.REVEAL_INDEX, lcm.REVEAL_SCORES


def _kw(K, values, mode, flags, **kw):
    key = "l1" if mode == lcm.ABSOLUTE else "l1_ratios"
    return dict(kw, folds=K, reveal_index=bool(flags & INDEX), reveal_scores=bool(flags & SCORES), **{key: list(values)})


def _solve(lgc, sysm, shares, **kw):
    s = lgc.Solver(sysm, seed=SEED, **kw)
    s.set_shares(shares)
    s.run()
    assert lgc.lib().lgc_solver_num_folds(s._h) == kw["folds"]
    out = s.beta().tolist(), s.selected_index(), s.scores()
    s.close()
    return out


@pytest.mark.parametrize("mode", [lcm.ABSOLUTE, lcm.RATIO])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_small_solve_matches_checker_and_model(lgc, gccpu, w, p, mode):
    """d = 6, K = 3, L = 4, N = 6, options on, both roles on one GPU.  Every launch of records other than products is a
    column-split launch.  The product launches cannot be at this shape: an iteration's (K + 1) L d = 96 dot products are
    576 one-product records at W = 64 (above the 256 of a column-split launch: a wide launch; 288 dual records at W = 32: a
    4-wave launch) and the scoring's 432 a 4-wave launch; none reaches the MAC kernels.  The modes are asserted from the
    program.  Every revealed word is the CPU checker's and the model's, with the reveal flags and without them"""
    d, K, L, N, lam, flags = 6, 3, 4, 6, 0.05, INDEX | SCORES
    rng = np.random.default_rng(zlib.crc32(("gpu cv %d %d" % (w, mode)).encode()))
    shares, per = cpu.fold_shares(rng, cpu.fold_words(rng, d, K, w, p), 2, w)
    values = sel.VALUES[lcm.RATIO][:L] if mode == lcm.RATIO else [0.001, 0.0002, 0.00002, 0.0005]
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0)
    opts = sel.options(d)
    prog = lgc.Program(sysm, **_kw(K, values, mode, flags, **opts))
    c = lgc.launch_constants()
    mg, me = lgc.RecordProgram.modes(prog)                  # (the kernel of every launch, as the solver picks it)
    assert mg == me
    for Lc, m in zip(prog.launches(), mg):
        n = Lc["nrec"]
        want = "split" if n <= c["split_max_recs"] else "wide" if n >= c["wide_launch"] else "quad2"
        assert m == lgc.LM[want] and (Lc["mac_only"] or want == "split"), (n, m)
    per_it = (K + 1) * L * d * d // (1 if w == 64 else 2)
    assert [Lc["nrec"] for Lc in prog.launches() if Lc["mac_only"]].count(per_it) == N - 1
    assert {lgc.LM["split"], lgc.LM["quad2"]} <= set(mg) and (w == 32 or lgc.LM["wide"] in mg)
    beta, idx, cv = _solve(lgc, sysm, shares, **_kw(K, values, mode, flags, **opts))
    assert beta + [idx] + cv.tolist() == sel.shown(prog, cpu.run_plain(gccpu, prog, w, p, shares)[0], w, flags, L)
    best, want, sc, _ = cpu.model(per, d, w, p, N, values, mode, 1, lam, opts)
    assert (beta, idx, cv.tolist()) == (best, want, sc)
    beta0, idx0, cv0 = _solve(lgc, sysm, shares, **_kw(K, values, mode, 0, **opts))
    assert beta0 == best and idx0 == -1 and cv0 is None


def _mack_launches(prog):
    recs = sel._recs(prog)
    return [recs[Lc["first_rec"]:Lc["first_rec"] + Lc["nrec"]] for Lc in prog.launches() if recs[Lc["first_rec"], 0] == sel.OP_MACK]


def _smallest_karatsuba_d(lgc, K, values, N):
    """the smallest d whose lowered program holds OP_MACK records (d^2 must exceed the 8192 products of kTargetWaves: 91)"""
    for d in range(88, 96):
        prog = lgc.Program(lgc.make_system(d, 64, 56, "lasso", N, 0.01, 2, 1, 0, 0), **_kw(K, values, lcm.RATIO, 0))
        if (sel._recs(prog)[:, 0] == sel.OP_MACK).any():
            return d
    raise AssertionError("no Karatsuba records up to d = 95")


@pytest.mark.parametrize("cut", [False, True])
def test_karatsuba_batches_span_matrices(lgc, gccpu, cut):
    """K = 2, L = 2, N = 2, W = 64 at the smallest d with OP_MACK records: the iteration batch reads the K + 1 training
    matrices and the scoring batch the K validation matrices through ONE shadow offset; cut: the two roles apart with
    max_launch_table_bytes lowered so that a batch is cut into several launches at the table cap.  Bit-exact against the CPU
    checker"""
    w, p, K, L, N, lam, flags = 64, 56, 2, 2, 2, 0.01, INDEX | SCORES
    values = [0.5, 0.05]
    d = _smallest_karatsuba_d(lgc, K, values, N)
    assert d == 91
    rng = np.random.default_rng(d)
    shares, _ = cpu.fold_shares(rng, cpu.fold_words(rng, d, K, w, p, rows=d + 30), 2, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0)
    kw = _kw(K, values, lcm.RATIO, flags)
    prog = lgc.Program(sysm, **kw)
    want = sel.shown(prog, cpu.run_plain(gccpu, prog, w, p, shares)[0], w, flags, L)
    assert any(want[:d]) and len(set(want[d + 1:])) == L

    mk = _mack_launches(prog)
    assert len(mk) == 2 and len({int(r[0, 5]) for r in mk}) == 1          # the iteration batch and the scoring batch, one shadow offset
    a0 = min(int(r[:, 3].min()) for r in mk)
    spans = [len({(int(a) - a0) // (d * d) for a in r[:, 3]}) for r in mk]
    assert spans == [K + 1, K], spans
    assert [int(r[:, 1].sum()) for r in mk] == [(K + 1) * L * d * d, K * L * d * d]
    if not cut:
        beta, idx, cv = _solve(lgc, sysm, shares, **kw)
        assert beta + [idx] + cv.tolist() == want
        return
    cap = 1 << 28                                                            # 256 MiB of tables: 2^17 gate steps per launch
    G = lgc.Party(sysm, lgc.GARBLER, seed=bytes(range(5, 21)), max_launch_table_bytes=cap, **kw)
    E = lgc.Party(sysm, lgc.EVALUATOR, max_launch_table_bytes=cap, **kw)
    assert G.num_launches == E.num_launches > prog.info.n_launches + 2          # both batches are cut
    assert max(G.table_bytes(k) for k in range(G.num_launches)) <= cap
    for s in range(2):
        E.set_input_labels(s, G.encode_inputs(s, shares[s]))
    buf = lgc.host_alloc(cap)                                               # one page-locked buffer for every launch's tables
    for k in range(G.num_launches):
        lgc._chk(lgc.lib().lgc_party_garble(G._h, k, lgc._vp(buf)))
        lgc._chk(lgc.lib().lgc_party_evaluate(E._h, k, lgc._vp(buf) if G.table_bytes(k) else None))
    beta, _, _ = E.finish(G.decode_bits())
    got = beta.tolist() + [E.selected_index()] + E.scores().tolist()
    G.close(); E.close()
    lgc.host_free(buf)
    assert got == want


def test_parties_apart(lgc):
    """garbler and evaluator as Party objects through host buffers, d = 6, K = 2, three shares: beta* and l* are the
    co-located solver's and the model's; the garbler learns no index; the fingerprint follows K and tells a cross-validation
    from a single hold-out"""
    w, p, d, K, N, L, P, lam = 64, 56, 6, 2, 6, 4, 3, 0.01
    rng = np.random.default_rng(29)
    shares, per = cpu.fold_shares(rng, cpu.fold_words(rng, d, K, w, p), P, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, P, 1, 0, 0)
    values = sel.VALUES[lcm.RATIO][:L]
    kw = _kw(K, values, lcm.RATIO, INDEX)
    G = lgc.Party(sysm, lgc.GARBLER, seed=bytes(range(5, 21)), **kw)
    E = lgc.Party(sysm, lgc.EVALUATOR, **kw)
    T = d * (d + 1) // 2
    assert G.input_bits == E.input_bits == K * (T + d) * w
    assert lgc.lib().lgc_party_num_folds(G._h) == lgc.lib().lgc_party_num_folds(E._h) == K
    assert G.program_fingerprint() == E.program_fingerprint()
    for other in (_kw(3, values, lcm.RATIO, INDEX), _kw(K, values, lcm.RATIO, 0),
                  dict(l1_ratios=values, validation=True, reveal_index=True), dict(l1_ratios=values)):
        o = lgc.Party(sysm, lgc.EVALUATOR, **other)
        assert o.program_fingerprint() != E.program_fingerprint()
        assert lgc.lib().lgc_party_num_folds(o._h) == other.get("folds", 0)
        o.close()
    for s in range(P):
        E.set_input_labels(s, G.encode_inputs(s, shares[s]))
    for k in range(G.num_launches):
        E.evaluate(k, G.garble(k))
    assert lgc.lib().lgc_party_selected_index(E._h) == -1      # nothing is decoded before finish()
    beta, _, _ = E.finish(G.decode_bits())
    got = beta.tolist(), E.selected_index(), E.scores()
    assert lgc.lib().lgc_party_selected_index(G._h) == -1      # the garbler learns nothing
    G.close(); E.close()
    assert got == _solve(lgc, sysm, shares, **kw)
    best, want, _, _ = cpu.model(per, d, w, p, N, values, lcm.RATIO, 1, lam, {})
    assert got == (best, want, None)
    s = lgc.Solver(sysm, seed=SEED, l1_ratios=values)
    assert lgc.lib().lgc_solver_num_folds(s._h) == 0
    s.close()
