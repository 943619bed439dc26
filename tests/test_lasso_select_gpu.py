"""In-circuit model selection of a lasso path (include/linreg_gc_lasso_select.h) on the MI355X: the co-located solver on the
column-split kernel against the CPU checker and the model (tests/lasso_select_model.py); the three record variants forced
onto every generic record kernel; a d = 300 and a d = 600 selection whose gated-select launches reach the 4-wave and the wide
kernel; the two roles apart."""
import zlib

import numpy as np
import pytest

import lasso_select_model as lsm
import op_corpus as oc
import test_lasso_select_cpu as cpu

pytestmark = pytest.mark.gpu

SEED = bytes(range(9, 25))
INDEX, SCORES = lsm.REVEAL_INDEX, lsm.REVEAL_SCORES


def _kw(values, mode, flags, **kw):
    key = "l1" if mode == lsm.ABSOLUTE else "l1_ratios"
    return dict(kw, validation=True, reveal_index=bool(flags & INDEX), reveal_scores=bool(flags & SCORES), **{key: list(values)})


def _solve(lgc, sysm, shares, **kw):
    s = lgc.Solver(sysm, seed=SEED, **kw)
    s.set_shares(shares)
    s.run()
    out = s.beta().tolist(), s.selected_index(), s.scores()
    s.close()
    return out


@pytest.mark.parametrize("mode", [lsm.ABSOLUTE, lsm.RATIO])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_small_solve_matches_checker_and_model(lgc, oracle, gccpu, w, p, mode):
    """d = 6, N = 8, L = 5, both roles on one GPU (every launch on the column-split kernel): every revealed word is the CPU
    checker's and the model's"""
    d, N, L, lam, flags = 6, 8, 5, 0.05, INDEX | SCORES
    rng = np.random.default_rng(zlib.crc32(("gpu select %d %d" % (w, mode)).encode()))
    A, b, Av, bv = cpu.two_systems(oracle, rng, d, w, p)
    shares, _, va = cpu.joined_shares(rng, A, b, Av, bv, 2, w)
    values = cpu.VALUES[lsm.RATIO][:L] if mode == lsm.RATIO else [0.01, 0.002, 0.0002, 0.005, 0.0008]
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0)
    opts = cpu.options(d)
    beta, idx, scores = _solve(lgc, sysm, shares, **_kw(values, mode, flags, **opts))
    prog = lgc.Program(sysm, **_kw(values, mode, flags, **opts))
    assert beta + [idx] + scores.tolist() == cpu.shown(prog, cpu.plain(gccpu, prog, w, p, shares), w, flags, L)
    a, bb = cpu.train_inputs(oracle, A, b, d, w, p, lam, 1)
    best, want, sc, _ = lsm.lasso_select(a, bb, va, d, w, p, N, values, mode, 1, opts["penalty_factors"], opts["lower"], opts["upper"])
    assert (beta, idx, scores.tolist()) == (best, want, sc)
    # nothing but beta* without the flags
    beta0, idx0, scores0 = _solve(lgc, sysm, shares, **_kw(values, mode, 0, **opts))
    assert beta0 == best and idx0 == -1 and scores0 is None


def _check(lgc, gccpu, C, g, e, what):
    prog = C.program(lgc, lambda kind: (g, e))
    mg, me = prog.modes()
    assert mg[:3] == [lgc.LM[g]] * 3 and me[:3] == [lgc.LM[e]] * 3, what
    s = lgc.RecordSolver(prog, seed=SEED)
    s.set_inputs(np.array(C.inputs, dtype=np.uint64))
    s.run()
    got = [int(v) for v in s.reveal()]
    s.close()
    plain = oc.plain_words(gccpu, prog, C)
    assert got[:len(plain)] == plain, what
    bad = cpu._mismatches(C, got, lsm.corpus_words(C))
    assert not bad, (what, bad)


@pytest.mark.parametrize("w", [32, 64])
@pytest.mark.parametrize("kernel", ["split", "quad2", "wide"])
def test_variants_on_generic_kernels(lgc, gccpu, w, kernel):
    """the signed minimum, the first-minimum one-hot and the gated select, forced onto each generic kernel, both roles: the
    edge corpus of the CPU test at cnt in {2, 9, 64, 256} (a few dozen records of each variant)"""
    p = w - 8
    C = lsm.select_corpus(w, p, np.random.default_rng([w, p, 5]), cnts=(2, 9, 64, 256))
    _check(lgc, gccpu, C, kernel, kernel, "w=%d p=%d kernel=%s" % (w, p, kernel))


def _launch_kinds(prog):
    recs = cpu._recs(prog)
    return [(Lc["nrec"], set(recs[Lc["first_rec"]:Lc["first_rec"] + Lc["nrec"], 0].tolist()),
             recs[Lc["first_rec"], 4]) for Lc in prog.launches()]


@pytest.mark.parametrize("d,L,wide", [(300, 3, False), (600, 2, True)])
def test_select_launch_reaches_the_4wave_and_wide_kernels(lgc, oracle, gccpu, d, L, wide):
    """N = 2: the launch of d gated-select records is a 4-wave launch at d = 300 and a wide launch at d = 600, where the
    scoring products are Karatsuba records; bit-exact against the CPU checker"""
    w, p, N, lam, flags = 64, 56, 2, 0.01, INDEX | SCORES
    rng = np.random.default_rng(d)
    A, b, Av, bv = cpu.two_systems(oracle, rng, d, w, p, n=2 * d, n_val=d + 50)
    shares, _, _ = cpu.joined_shares(rng, A, b, Av, bv, 2, w)
    values = [0.5, 0.02, 0.1][:L]
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0)
    prog = lgc.Program(sysm, **_kw(values, lsm.RATIO, flags))
    kinds = _launch_kinds(prog)
    sel = [k for k in kinds if k[1] == {cpu.OP_SUM} and k[2] != 0]
    c = lgc.launch_constants()
    assert [k[0] for k in sel] == [d] and (c["split_max_recs"] < d) and ((d >= c["wide_launch"]) == wide)
    mack = sum(k[0] for k in kinds if k[1] == {cpu.OP_MACK})
    assert mack > 0 and kinds[-1][0] == d + 1 + L
    beta, idx, scores = _solve(lgc, sysm, shares, **_kw(values, lsm.RATIO, flags))
    assert beta + [idx] + scores.tolist() == cpu.shown(prog, cpu.plain(gccpu, prog, w, p, shares), w, flags, L)
    assert idx == lsm.argmin_first(scores.tolist()) and any(beta)


def test_parties_apart(lgc, oracle):
    """garbler and evaluator as Party objects through host buffers, d = 6, L = 4: the finished beta* and index are the
    co-located solver's; the fingerprint follows the validation system and the reveal flags"""
    w, p, d, N, L, P, lam = 64, 56, 6, 6, 4, 3, 0.01
    rng = np.random.default_rng(23)
    A, b, Av, bv = cpu.two_systems(oracle, rng, d, w, p)
    shares, _, va = cpu.joined_shares(rng, A, b, Av, bv, P, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, P, 1, 0, 0)
    values = cpu.VALUES[lsm.RATIO][:L]
    kw = _kw(values, lsm.RATIO, INDEX)
    G = lgc.Party(sysm, lgc.GARBLER, seed=bytes(range(5, 21)), **kw)
    E = lgc.Party(sysm, lgc.EVALUATOR, **kw)
    T = d * (d + 1) // 2
    assert G.input_bits == E.input_bits == 2 * (T + d) * w
    assert G.program_fingerprint() == E.program_fingerprint()
    for other in (_kw(values, lsm.RATIO, 0), _kw(values, lsm.RATIO, INDEX | SCORES), dict(l1_ratios=values)):
        o = lgc.Party(sysm, lgc.EVALUATOR, **other)
        assert o.program_fingerprint() != E.program_fingerprint()
        o.close()
    for s in range(P):
        E.set_input_labels(s, G.encode_inputs(s, shares[s]))
    for k in range(G.num_launches):
        E.evaluate(k, G.garble(k))
    assert lgc.lib().lgc_party_selected_index(E._h) == -1      # nothing is decoded before finish()
    with pytest.raises(lgc.LgcError):
        E.selected_index()
    beta, _, _ = E.finish(G.decode_bits())
    got = beta.tolist(), E.selected_index(), E.scores()
    assert lgc.lib().lgc_party_selected_index(G._h) == -1      # the garbler learns nothing
    G.close(); E.close()
    assert got == _solve(lgc, sysm, shares, **kw)
    a, bb = cpu.train_inputs(oracle, A, b, d, w, p, lam, 1)
    best, want, _, _ = lsm.lasso_select(a, bb, va, d, w, p, N, values, lsm.RATIO, 1)
    assert got == (best, want, None)
    # a solver that is no selection has neither an index nor scores
    s = lgc.Solver(sysm, seed=SEED, l1_ratios=values)
    for call in (s.selected_index, s.scores):
        with pytest.raises(lgc.LgcError):
            call()
    s.close()
