"""The one-standard-error rule of the in-circuit K-fold cross-validation (include/linreg_gc_lasso_cv_se.h) on the CPU: the
lowered program, run record by record by the CPU checker and garbled + evaluated by its CPU backends, against the
independent model of tests/lasso_cv_se_model.py; pinned inputs on which the rule does and does not move the choice; a float64
restatement of the curve; the structure of the lowering; the rejections.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lasso_cv_se_data as sed
import lasso_cv_se_model as sem
import test_lasso_select_cpu as sel
from helpers import sx

ROOT = sel.ROOT
INDEX, SCORES, CURVE = sem.REVEAL_INDEX, sem.REVEAL_SCORES, sem.REVEAL_CURVE
ALL = INDEX | SCORES | CURVE
OP_SUM, OP_MUL, OP_MAX, OP_SQRT, OP_IDIVC, OP_EQ = 2, 7, 12, 14, 15, 22      # gc_exec.h
N = 6
GRID = [(d, K, L) for d in (3, 5) for K in (2, 3, 5) for L in (3, 9)]


def mode_of(d, K, L):
    """both modes over the grid, so that neither rides on one shape only"""
    return sem.RATIO if (d + K + L // 3) % 2 else sem.ABSOLUTE


def program(lgc, case, flags, rule="1se", iters=N):
    return lgc.Program(case.system(lgc, iters), **case.request(flags, rule))


def run_plain(gccpu, prog, case):
    info = prog.info
    assert case.shares.shape[1] == case.K * (case.d * (case.d + 1) // 2 + case.d) + case.K
    words = np.zeros(info.n_words, dtype=np.uint64)
    words[info.in_base:info.in_base + case.shares.size] = case.shares.ravel() & np.uint64((1 << case.w) - 1)
    dec = np.zeros(info.n_reveal + 1, dtype=np.uint64)
    steps, gates = gccpu.plain_run(prog.records(), info.n_records, case.w, case.p, words, dec)
    assert steps == info.total_steps and gates == info.total_gates
    return dec


def shown(prog, dec, w):
    """every word the program reveals from rv_beta on"""
    return sx(dec[prog.info.rv_beta:prog.info.n_reveal], w).tolist()


@pytest.mark.parametrize("d,K,L", GRID)
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_program_reveals_the_model(lgc, gccpu, w, p, normalize, d, K, L):
    """every revealed word of the lowered program, run record by record, is the model's: beta+, l+, l*, cv, mean, se; the
    reveal combinations; the arg-min rule with the curve; the values are given out of order (pi is not the identity)"""
    case = sed.Case(w, p, normalize, mode_of(d, K, L), d, K, L)
    m = case.model(N)
    assert m["order"] != list(range(L))
    for flags in (ALL, 0, INDEX, CURVE, INDEX | SCORES):
        prog = program(lgc, case, flags)
        assert shown(prog, run_plain(gccpu, prog, case), w) == sem.revealed(m, flags), flags
    m0 = case.model(N, sem.RULE_MIN)
    assert m0["index"] == m0["min"] == m["min"] and m0["mean"] == m["mean"]
    for flags in (ALL, INDEX):
        prog = program(lgc, case, flags, "min")
        assert shown(prog, run_plain(gccpu, prog, case), w) == sem.revealed(m0, flags, sem.RULE_MIN), flags


@pytest.mark.parametrize("d,K,L", GRID)
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_cpu_garble_evaluate_gives_the_model(lgc, gccpu, w, p, normalize, d, K, L):
    """the same grid garbled and evaluated on the CPU, everything revealed"""
    case = sed.Case(w, p, normalize, mode_of(d, K, L), d, K, L)
    prog = program(lgc, case, ALL)
    dec, gates, _ = gccpu.garble_eval(prog, case.shares)
    assert gates == prog.info.total_gates
    assert shown(prog, dec, w) == sem.revealed(case.model(N), ALL)


@pytest.mark.parametrize("mode", [sem.ABSOLUTE, sem.RATIO])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_penalty_factors_and_bounds(lgc, gccpu, w, p, mode):
    case = sed.Case(w, p, 1, mode, 5, 3, 3, kw=sel.options(5))
    prog = program(lgc, case, ALL)
    m = case.model(N)
    assert shown(prog, run_plain(gccpu, prog, case), w) == sem.revealed(m, ALL)
    dec, _, _ = gccpu.garble_eval(prog, case.shares)
    assert shown(prog, dec, w) == sem.revealed(m, ALL)
    assert m["beta"] != sed.Case(w, p, 1, mode, 5, 3, 3).model(N)["beta"]          # (the options change the model)


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_one_value_scores_nothing(lgc, gccpu, w, p, normalize):
    """L = 1: beta+ = beta_{K,0}, l+ = l* = 0, revealed cv and curve words are the constant 0; no record reads a yy word"""
    case = sed.Case(w, p, normalize, sem.RATIO, 3, 3, 1)
    prog = program(lgc, case, ALL)
    got = shown(prog, run_plain(gccpu, prog, case), w)
    m = case.model(N)
    assert got == sem.revealed(m, ALL) and got[3:] == [0] * 5 and any(got[:3])
    r = sel._recs(prog)
    assert not (r[:, 0] == OP_SQRT).any() and (r[r[:, 0] == sel.OP_REVEAL][3:, 3] == 0).all()


# the pinned cases of both suites (tests/test_lasso_cv_se_gpu.py runs them on the device): on MOVES the rule picks a more
# regularised value than the arg-min, on STAYS the two agree
MOVES = [dict(w=64, p=56, normalize=1, mode=sem.RATIO, d=5, K=3, L=3), dict(w=32, p=24, normalize=1, mode=sem.ABSOLUTE, d=5, K=3, L=3),
         dict(w=64, p=56, normalize=0, mode=sem.RATIO, d=3, K=5, L=9, seed=1), dict(w=32, p=24, normalize=0, mode=sem.RATIO, d=3, K=5, L=9, seed=1)]
STAYS = [dict(w=64, p=56, normalize=0, mode=sem.ABSOLUTE, d=5, K=3, L=3, seed=1), dict(w=32, p=24, normalize=0, mode=sem.ABSOLUTE, d=3, K=5, L=9, seed=1)]


def test_the_rule_moves_the_choice_where_it_should(lgc, gccpu):
    """of the model itself: on MOVES l+ != l*, l+ comes before l* in pi-order (a larger penalty) and its mean lies within
    mean_{l*} + se_{l*} while every value before it in pi-order exceeds that; on STAYS l+ = l*.  The program agrees on each"""
    for kw, moves in [(k, True) for k in MOVES] + [(k, False) for k in STAYS]:
        case = sed.Case(**kw)
        m = case.model(N)
        pi, thr = m["order"], m["mean"][m["min"]] + m["se"][m["min"]]
        assert (m["index"] != m["min"]) == moves, kw
        assert pi.index(m["index"]) <= pi.index(m["min"]) and m["mean"][m["index"]] <= thr
        assert all(m["mean"][l] > thr for l in pi[:pi.index(m["index"])])
        assert m["min"] == min(range(case.L), key=lambda l: (m["cv"][l], l)) and min(m["se"]) >= 0
        q = [int(v * 2.0 ** case.p) for v in case.values]
        assert q[m["index"]] >= q[m["min"]]
        prog = program(lgc, case, ALL)
        assert shown(prog, run_plain(gccpu, prog, case), case.w) == sem.revealed(m, ALL)
        if moves:                                              # the arg-min rule reveals another model on the same inputs
            prog = program(lgc, case, INDEX, "min")
            got = shown(prog, run_plain(gccpu, prog, case), case.w)
            assert got[case.d] == m["min"] and got[:case.d] != m["beta"]


# ---- float64 restatement of the curve
# Largest |integer - float| over the 24 systems of the grid (ratio mode, both input paths, N = 6), as measured on the CPU, in
# units of the decoded values:
#   W = 64, p = 56:  mean 1.388e-17,  se 2.574e-14        (a word's last place: 2^-56 = 1.388e-17)
#   W = 32, p = 24:  mean 4.768e-08,  se 1.541e-04        (a word's last place: 2^-24 = 5.960e-08)
# The mean is one truncating division away from the exact sum; se is a square root of a quantity that carries K truncated
# products and one truncating division, and an error delta under a root of size se grows to delta / (2 se): with se between
# 4e-4 and 1e-2 that is the measured figure.  The tolerance is the measured error plus a margin of two last places for the
# two truncating divisions (mean: by K; se: by K (K - 1) and the root's own truncation).
MEASURED = {64: (1.388e-17, 2.574e-14), 32: (4.768e-08, 1.541e-04)}
MARGIN_ULPS = 2


@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_float_restatement_of_the_curve(lgc, gccpu, w, p):
    """the decoded mean_l and se_l of the PROGRAM against numpy's mean and std(ddof = 1) / sqrt(K) of the decoded per-fold
    errors; cvm and cvsd of cv.glmnet with equal fold weights.  Largest |integer - float| over the 24 systems, as measured
    on the CPU, and the margin added for the truncating divisions (two last places):
      W = 64, p = 56:  mean 1.388e-17, se 2.574e-14, margin 2 x 2^-56 = 2.776e-17
      W = 32, p = 24:  mean 4.768e-08, se 1.541e-04, margin 2 x 2^-24 = 1.192e-07
    The bound is measured + margin.  At W = 32 the bound on se (1.5e-4) is a sizeable fraction of the smallest se on these
    inputs (about 4e-4): an error delta under a root of size se grows to delta / (2 se), so the float check of se is weak
    at that width; the integer model is what pins se there"""
    worst_m = worst_s = 0.0
    for normalize in (0, 1):
        for d, K, L in GRID:
            case = sed.Case(w, p, normalize, sem.RATIO, d, K, L)
            prog = program(lgc, case, CURVE)
            got = shown(prog, run_plain(gccpu, prog, case), w)
            mean, se = (np.array(got[d + h * L:d + (h + 1) * L], dtype=np.float64) / 2.0 ** p for h in (0, 1))
            e = np.array(case.model(N)["errors"], dtype=np.float64) / 2.0 ** p
            worst_m = max(worst_m, float(np.abs(mean - e.mean(axis=0)).max()))
            worst_s = max(worst_s, float(np.abs(se - e.std(axis=0, ddof=1) / np.sqrt(K)).max()))
    print("W = %d: largest |integer - float|: mean %.3e, se %.3e" % (w, worst_m, worst_s))
    margin = MARGIN_ULPS * 2.0 ** -p
    assert worst_m <= MEASURED[w][0] + margin and worst_s <= MEASURED[w][1] + margin


# ---- structure of the lowering
def _ops(prog):
    r = sel._recs(prog)
    return {int(op): int((r[:, 0] == op).sum()) for op in set(r[:, 0].tolist())}


def test_structure_of_the_lowering(lgc):
    """d = 5, K = 3, L = 4 on the data-provider path.  The arg-min rule without the curve through the new call has the records
    of lgc_program_build_lasso_cv, op for op and launch for launch: only the K input words per share are added.  The rule adds
    K L multiplies, L square roots, 2 L constant divisions (K more for the Y_k in the prefix), L two-word minima, one first-match
    record and three gated selects; the curve alone adds the first three and no compare"""
    d, K, L = 5, 3, 4
    sysm = lgc.make_system(d, 64, 56, "lasso", 3, 0.01, 2, 1, 0, 0)
    kw = dict(l1_ratios=[0.1, 1.0, 0.5, 0.3], folds=K, reveal_index=True)
    base, off, on, curve = (lgc.Program(sysm, **kw), lgc.Program(sysm, rule="min", **kw), lgc.Program(sysm, rule="1se", **kw),
                            lgc.Program(sysm, rule="min", reveal_curve=True, **kw))
    T = d * (d + 1) // 2
    assert off.info.n_words == base.info.n_words + 3 * K             # two shares and their sums
    assert _ops(off) == _ops(base) and off.info.n_launches == base.info.n_launches and off.info.total_gates == base.info.total_gates
    assert off.info.n_reveal == base.info.n_reveal == d + 1 and on.info.n_reveal == d + 2 and curve.info.n_reveal == d + 1 + 2 * L
    a, b, c = _ops(base), _ops(on), _ops(curve)
    diff = lambda x, op: x.get(op, 0) - a.get(op, 0)
    assert (diff(b, OP_MUL), diff(b, OP_SQRT), diff(b, OP_IDIVC)) == (K * L, L, 2 * L + K) == (diff(c, OP_MUL), diff(c, OP_SQRT), diff(c, OP_IDIVC))
    assert diff(b, OP_MAX) == L and diff(b, OP_EQ) == 1 and diff(c, OP_MAX) == 0 and diff(c, OP_EQ) == 0
    assert diff(b, OP_SUM) == K + 2 * L + 3 and diff(c, OP_SUM) == K + 2 * L
    # the K sums Y_k and their divisions are words and launches of the prefix
    r = sel._recs(on)
    in_base, IN = on.info.in_base, K * (T + d) + K
    ysum = r[(r[:, 0] == OP_SUM) & (r[:, 3] >= in_base + K * (T + d)) & (r[:, 3] < in_base + IN)]
    assert len(ysum) == K and (ysum[:, 1] == 2).all() and (ysum[:, 6] == IN).all() and (ysum[:, 2] < on.info.shared_end).all()
    # one value: the full system alone is fitted and no yy word is read
    one = lgc.Program(sysm, l1_ratios=[0.3], folds=K, rule="1se", reveal_index=True, reveal_curve=True)
    assert one.info.n_reveal == d + 4 and _ops(one).get(OP_SQRT, 0) == 0


def test_programs_differ_with_the_rule_the_curve_and_the_order(lgc):
    """the record bytes of rule on / off, curve on / off and of two orders of the same values differ pairwise"""
    sysm = lgc.make_system(4, 64, 56, "lasso", 3, 0.01, 2, 1, 0, 0)
    progs = [lgc.Program(sysm, l1_ratios=v, folds=3, rule=r, reveal_curve=c)
             for v, r, c in (([0.1, 1.0, 0.5], "1se", False), ([0.1, 1.0, 0.5], "min", False), ([0.1, 1.0, 0.5], "1se", True),
                             ([0.1, 1.0, 0.5], "min", True), ([1.0, 0.5, 0.1], "1se", False))]
    assert len({pr.records().tobytes() for pr in progs}) == len(progs)


def test_ties_in_the_order_go_to_the_smaller_index():
    assert sem.order([0.5, 1.0, 0.5, 1.0], 64, 56) == [1, 3, 0, 2]


# ---- rejections and the interface
def test_rejections(lgc):
    d = 4
    sysm = lgc.make_system(d, 64, 56, "lasso", 5, 0.01, 2, 1, 0, 0)
    Lb = lgc.lib()
    vals = (C.c_double * 2)(0.1, 0.2)
    o = lgc.LassoOpts(2, C.cast(vals, C.c_void_p), 0, None, None, None)
    out = C.c_void_p()
    for rule in (2, -1, 7):
        assert Lb.lgc_program_build_lasso_cv_se(C.byref(out), C.byref(sysm), C.byref(o), 3, 0, rule) == -1
        assert b"unknown cross-validation rule" in Lb.lgc_last_error()
    for flags in (8, 16 | 1, -1):
        assert Lb.lgc_program_build_lasso_cv_se(C.byref(out), C.byref(sysm), C.byref(o), 3, flags, 1) == -1
        assert b"unknown reveal flags" in Lb.lgc_last_error() and b"LGC_SELECT_REVEAL_CURVE (4)" in Lb.lgc_last_error()
    # the older call keeps refusing the new bit
    assert Lb.lgc_program_build_lasso_cv(C.byref(out), C.byref(sysm), C.byref(o), 3, 4) == -1
    assert b"unknown reveal flags" in Lb.lgc_last_error() and b"CURVE" not in Lb.lgc_last_error()
    assert Lb.lgc_program_build_lasso_cv_se(C.byref(out), C.byref(sysm), None, 3, 0, 1) == -1 and b"null opts" in Lb.lgc_last_error()
    for K in (1, 17):
        assert Lb.lgc_program_build_lasso_cv_se(C.byref(out), C.byref(sysm), C.byref(o), K, 0, 1) == -1 and b"2..16 folds" in Lb.lgc_last_error()
    assert Lb.lgc_program_build_lasso_cv_se(C.byref(out), C.byref(sysm), C.byref(o), 16, 7, 1) == 0
    Lb.lgc_program_destroy(out)
    assert Lb.lgc_solver_min_index(None) == -1 and Lb.lgc_party_min_index(None) == -1
    for kw, want in ((dict(rule="1se"), "belong to folds=K"), (dict(reveal_curve=True), "belong to folds=K"),
                     (dict(folds=3, rule="2se"), "unknown rule"), (dict(validation=True, rule="1se"), "belong to folds=K")):
        with pytest.raises(lgc.LgcError) as e:
            lgc.Program(sysm, l1=[0.1, 0.2], **kw)
        assert want in str(e.value), str(e.value)
    tr = lgc.make_system(d, 64, 56, "lasso", 5, 0.01, 2, 1, 0, 1)
    with pytest.raises(lgc.LgcError) as e:                       # (refused before a GPU is looked for)
        lgc.Solver(tr, l1=[0.1, 0.2], folds=2, rule="1se")
    assert "trace" in str(e.value)
    with pytest.raises(lgc.LgcError) as e:
        lgc.Party(sysm, lgc.GARBLER, seed=bytes(16), l1_ratios=[0.3], folds=17, reveal_curve=True)
    assert "2..16 folds" in str(e.value)


@pytest.mark.parametrize("normalize", [0, 1])
def test_reveal_inputs_gives_the_folds_and_their_sums(lgc, gccpu, normalize):
    """reveal_inputs = 1: K (T + d) + K words laid out as a share is, the folds and then Y_k as the model assembles them"""
    import lasso_cv_model as lcm
    case = sed.Case(64, 56, normalize, sem.RATIO, 4, 3, 3)
    sysm = lgc.make_system(4, 64, 56, "lasso", 2, case.lam, 2, normalize, 1, 0)
    prog = lgc.Program(sysm, **case.request(INDEX))
    dec = run_plain(gccpu, prog, case)
    n = case.shares.shape[1]
    want = [v for M, b in lcm.fold_systems(case.per, 4, 64, normalize) for v in lcm.packed(M, 4) + list(b)] + sem.fold_sums(case.yy, 4, 64, normalize)
    assert sx(dec[prog.info.rv_inputs:prog.info.rv_inputs + n], 64).tolist() == want and prog.info.rv_beta == prog.info.rv_inputs + n
    # no curve formed (the arg-min without the curve bit; one value): the K slots are revealed as the constant zero
    one = sed.Case(64, 56, normalize, sem.RATIO, 4, 3, 1)
    for c, req in ((case, case.request(INDEX, "min")), (one, one.request(INDEX))):
        prog = lgc.Program(sysm, **req)
        c.shares[:] = np.hstack([case.shares[:, :n - 3], case.yy])         # (the same folds under either request)
        dec = np.full(prog.info.n_reveal + 1, 0x5a5a, dtype=np.uint64)          # decode words that do not start at zero
        words = np.zeros(prog.info.n_words, dtype=np.uint64)
        words[prog.info.in_base:prog.info.in_base + c.shares.size] = c.shares.ravel()
        gccpu.plain_run(prog.records(), prog.info.n_records, 64, 56, words, dec)
        assert sx(dec[prog.info.rv_inputs:prog.info.rv_inputs + n], 64).tolist() == want[:n - 3] + [0, 0, 0]
        r = sel._recs(prog)
        assert (r[:, 0] == sel.OP_REVEAL).sum() == prog.info.n_reveal


def test_headers_are_exported_and_documented(lgc):
    names = {}
    for hdr in ("linreg_gc_lasso_cv_se.h", "linreg_gc_folds_yy.h"):
        text = open(os.path.join(ROOT, "include", hdr)).read()
        names[hdr] = set(re.findall(r"^[a-z][^\n(]*?\b(lgc_[a-z_0-9]+)\s*\(", text, flags=re.M))
    assert names["linreg_gc_lasso_cv_se.h"] == {"lgc_program_build_lasso_cv_se", "lgc_solver_create_lasso_cv_se", "lgc_party_create_lasso_cv_se",
                                                "lgc_solver_min_index", "lgc_party_min_index"}
    assert names["linreg_gc_folds_yy.h"] == {"lgc_p1_local_folds_yy"}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for hdr, ns in names.items():
        assert hdr in doc, hdr
        for nme in ns:
            assert hasattr(lgc.lib(), nme), nme
            assert nme in doc, nme
    assert "### 1.13" in doc and "LGC_SELECT_REVEAL_CURVE" in doc and "LGC_CV_RULE_ONE_SE" in doc
    hdr = open(os.path.join(ROOT, "include", "linreg_gc_lasso_cv_se.h")).read()
    for word in ("K (T + d) + K", "leaks", "per-fold error is never revealed", "ties to the smaller l"):
        assert word in hdr, word
    assert "lasso_one_se" in design and "one-standard-error" in design
    assert "--one_se" in open(os.path.join(ROOT, "README.md")).read()
