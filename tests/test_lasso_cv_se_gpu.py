"""The one-standard-error rule of the in-circuit K-fold cross-validation (include/linreg_gc_lasso_cv_se.h) on the MI355X:
every revealed word -- beta+, l+, l*, cv, mean, se -- of the co-located solver and of the two roles apart against the model
(tests/lasso_cv_se_model.py) and the CPU checker, on the cases tests/test_lasso_cv_se_cpu.py pins (the rule moves the choice
on MOVES); one d = 40 solve at W = 64 whose new launches run beside product batches on the MAC kernel."""
import numpy as np
import pytest

import lasso_cv_se_data as sed
import lasso_cv_se_model as sem
import test_lasso_cv_se_cpu as cpu
import test_lasso_select_cpu as sel

pytestmark = pytest.mark.gpu

SEED = bytes(range(9, 25))
ALL, N = cpu.ALL, cpu.N


def _solve(lgc, case, flags, rule="1se", iters=N):
    s = lgc.Solver(case.system(lgc, iters), seed=SEED, **case.request(flags, rule))
    s.set_shares(case.shares)
    s.run()
    assert lgc.lib().lgc_solver_num_folds(s._h) == case.K
    out = s.beta().tolist(), s.selected_index(), s.min_index(), s.scores(), s.cv_curve()
    s.close()
    return out


def _words(beta, idx, lmin, cv, curve, rule=sem.RULE_ONE_SE):
    return (beta + ([idx, lmin] if rule == sem.RULE_ONE_SE else [lmin]) + cv.tolist() + curve[0].tolist() + curve[1].tolist())


@pytest.mark.parametrize("kw", cpu.MOVES + cpu.STAYS, ids=lambda k: "w%d d%d K%d L%d" % (k["w"], k["d"], k["K"], k["L"]))
def test_solve_reveals_the_model(lgc, gccpu, kw):
    """both roles on one GPU, both widths, d = 5, K = 3, L = 3 and d = 3, K = 5, L = 9 (the two-level minimum tree)"""
    case = sed.Case(**kw)
    m = case.model(N)
    assert (m["index"] != m["min"]) == (kw in cpu.MOVES)
    got = _solve(lgc, case, ALL)
    assert _words(*got) == sem.revealed(m, ALL)
    assert (got[1], got[2]) == (m["index"], m["min"])
    prog = cpu.program(lgc, case, ALL)
    assert _words(*got) == cpu.shown(prog, cpu.run_plain(gccpu, prog, case), case.w)
    if kw in cpu.MOVES[:2]:                                   # nothing but beta+; the arg-min rule with the curve
        beta, idx, lmin, cv, curve = _solve(lgc, case, 0)
        assert beta == m["beta"] and (idx, lmin, cv, curve) == (-1, -1, None, None)
        got0 = _solve(lgc, case, ALL, "min")
        m0 = case.model(N, sem.RULE_MIN)
        assert _words(*got0, rule=sem.RULE_MIN) == sem.revealed(m0, ALL, sem.RULE_MIN) and got0[1] == got0[2] == m["min"]
        assert got0[0] != beta


def test_parties_apart(lgc):
    """garbler and evaluator as Party objects through host buffers on a MOVES case with three shares: every revealed word is
    the model's; the garbler learns no index; the fingerprint follows the rule, the curve bit and the order pi"""
    case = sed.Case(nshares=3, **cpu.MOVES[0])
    m = case.model(N)
    assert m["index"] != m["min"]
    kw = case.request(ALL)
    sysm = case.system(lgc, N)
    G = lgc.Party(sysm, lgc.GARBLER, seed=bytes(range(5, 21)), **kw)
    E = lgc.Party(sysm, lgc.EVALUATOR, **kw)
    T = case.d * (case.d + 1) // 2
    assert G.input_bits == E.input_bits == (case.K * (T + case.d) + case.K) * case.w
    assert G.program_fingerprint() == E.program_fingerprint()
    swapped = dict(kw, l1_ratios=[kw["l1_ratios"][i] for i in (2, 1, 0)])
    for other in (dict(kw, rule="min"), dict(kw, reveal_curve=False), swapped, {k: v for k, v in kw.items() if k not in ("rule", "reveal_curve")}):
        o = lgc.Party(sysm, lgc.EVALUATOR, **other)
        assert o.program_fingerprint() != E.program_fingerprint()
        o.close()
    for s in range(3):
        E.set_input_labels(s, G.encode_inputs(s, case.shares[s]))
    for k in range(G.num_launches):
        E.evaluate(k, G.garble(k))
    assert lgc.lib().lgc_party_min_index(E._h) == -1            # nothing is decoded before finish()
    beta, _, _ = E.finish(G.decode_bits())
    got = _words(beta.tolist(), E.selected_index(), E.min_index(), E.scores(), E.cv_curve())
    assert lgc.lib().lgc_party_min_index(G._h) == -1 and lgc.lib().lgc_party_selected_index(G._h) == -1   # the garbler learns nothing
    G.close(); E.close()
    assert got == sem.revealed(m, ALL)


def test_beside_mac_kernel_batches(lgc, gccpu):
    """d = 40, K = 2, L = 3, N = 3 at W = 64: an iteration's (K + 1) L d d = 14400 products exceed kara_min (8192), so the
    batch is shaped as the Karatsuba batches are -- one product launch of 14400 records on the MAC kernel (d d = 1600 stays
    under the threshold for a shadow, so the records are OP_MAC) -- and the rule's short launches follow the scoring
    batches.  Bit-exact against the CPU checker, whose revealed words the model confirms"""
    case = sed.Case(64, 56, 1, sem.RATIO, 40, 2, 3, rows=60)
    prog = cpu.program(lgc, case, ALL, iters=3)
    r = sel._recs(prog)
    mac = [Lc["nrec"] for Lc in prog.launches() if Lc["mac_only"]]
    assert mac[:2] == [14400, 14400] and len(mac) == 4 and (r[:, 0] == cpu.OP_SQRT).sum() == 3
    want = cpu.shown(prog, cpu.run_plain(gccpu, prog, case), 64)
    assert want == sem.revealed(case.model(3), ALL)
    assert _words(*_solve(lgc, case, ALL, iters=3)) == want
