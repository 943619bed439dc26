"""What the Python binding makes of a program request, without the library and without a GPU.

tests/golden/binding_calls.json (tests/golden/gen_binding_calls.py) holds, for every case on each of Program, Solver and
Party, the one creation call with its arguments by value and the attributes the object then shows, or the text of the
refusal -- recorded from the binding as it was before its three constructors were folded into one request.  Here the cases
are replayed on the binding of the tree against the same recording stub.  The second test pins where every revealed word
goes, against the layouts written in the headers."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_binding_calls", os.path.join(HERE, "golden", "gen_binding_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def binding():
    """the module alone: nothing here loads liblinreg_gc.so"""
    import linreg_gc
    return linreg_gc


def test_every_request_makes_the_recorded_call_or_refusal(gen, binding, golden_dir):
    want = json.load(open(os.path.join(golden_dir, "binding_calls.json")))["cases"]
    got = gen.record(binding)
    assert sorted(got) == sorted(want)
    for name, fronts, _, _, _ in gen.cases():
        assert sorted(got[name]) == sorted(want[name]) == sorted(fronts)
        for front in fronts:
            g, w = got[name][front], want[name][front]
            assert json.loads(json.dumps(g)) == w, (name, front)      # (the call with every argument, the attributes; or the text)


def test_cases_cover_every_kind_front_and_refusal(gen, binding, golden_dir):
    """the fixture reaches each of the twelve kinds on every front that has it, the variants the kinds have, and every
    `raise LgcError` of the request's helpers and of the fronts"""
    want = json.load(open(os.path.join(golden_dir, "binding_calls.json")))["cases"]
    calls = {r["call"][0] for v in want.values() for r in v.values() if "call" in r}
    kinds = ("", "_targets", "_sweep_at", "_lasso", "_lasso_path", "_lasso_opts", "_lasso_select", "_lasso_cv", "_lasso_cv_se",
             "_ridge_cv", "_inference", "_scan")
    assert calls == {p + k for p in gen.CREATION for k in kinds} - {"lgc_party_create_sweep_at"}
    tails = [r["call"][1] for v in want.values() for r in v.values() if "call" in r]
    opts = [a for t in tails for a in t if isinstance(a, dict) and "l1_mode" in a]
    assert {o["l1_mode"] for o in opts} == {0, 1} and {o["l1_count"] for o in opts} >= {1, 2, 3}
    assert all(any(o[k] is not None for o in opts) for k in ("lower", "upper", "penalty_factors"))
    assert any(o["lower"] == [0.0] * 4 and o["upper"] is None for o in opts)                                  # positive=True
    attrs = [r["attrs"] for v in want.values() for r in v.values() if "attrs" in r]
    assert {a["select"] for a in attrs} >= {None, 0, 1, 2, 3, 4, 7} and {a["rule"] for a in attrs} == {None, 0, 1}
    assert {tuple(a["infer"])[0] for a in attrs if a["infer"]} == {1, 2, 3} and {a["scan"][1] for a in attrs if a["scan"]} == {0, 1}
    assert want["sweep first"]["Solver"]["call"][1][-1] == 5 and want["sweep first"]["Solver"]["attrs"]["count"] == 3
    assert want["select scalar"]["Program"]["attrs"]["path"] is None and want["select scalar"]["Solver"]["attrs"]["path"] == 1
    # every refusal the binding can raise: the text of each `raise LgcError(-1, "...")`, up to its first % conversion
    src = open(binding.__file__).read()
    raised = re.findall(r'raise LgcError\(-1, "((?:[^"\\]|\\.)*)"', src) + re.findall(r'no_sweep="([^"]*)"', src)
    assert len(raised) >= 25
    texts = [r["error"] for v in want.values() for r in v.values() if "error" in r]
    later = ("not a model selection", "no curve", "not an inference program", "not a scan", "the scan words follow",
             "the inference words follow")                                       # (of the accessors: the next test)
    for msg in raised:
        head = re.split(r"%[sdr]", msg.replace('\\"', '"'))[0]
        if not head.startswith(later):
            assert any(head in t for t in texts), msg


# ---- where the revealed words go.  d = 4, L = 3 values, K = 2 folds, M = 2 candidates; lgc_party_finish is a stub that fills
# the buffer it is given with 100, 101, 102, ..: the expected slices are the headers' layouts, written out
D, L3 = 4, [0.5, 0.25, 0.125]
T = D * (D + 1) // 2
CV = dict(l1_ratios=L3, folds=2)
LAYOUT = [
    # keywords; words per share; size of the buffer; beta; then the accessors
    # include/linreg_gc.h, _targets.h, _lasso_path.h: beta alone, in its shape
    (dict(), T + D, 4, [100, 101, 102, 103], {}),
    (dict(targets=2), T + 2 * D, 8, [[100, 101, 102, 103], [104, 105, 106, 107]], {}),
    (dict(l1=[0.1, 0.01, 0.001]), T + D, 12, [[100, 101, 102, 103], [104, 105, 106, 107], [108, 109, 110, 111]], {}),
    # include/linreg_gc_lasso_select.h: beta* (d), [l*], [score_0 .. score_{L-1}]; the buffer has room for d + 2 + 3 L
    (dict(l1_ratios=L3, validation=True), 2 * (T + D), 15, [100, 101, 102, 103], dict(scores=None, index=None, min_index=None)),
    (dict(l1_ratios=L3, validation=True, reveal_index=True, reveal_scores=True), 2 * (T + D), 15, [100, 101, 102, 103],
     dict(scores=[105, 106, 107], index=104, min_index=104)),
    (dict(l1_ratios=L3, validation=True, reveal_scores=True), 2 * (T + D), 15, [100, 101, 102, 103], dict(scores=[104, 105, 106])),
    (dict(l1=0.1, validation=True, reveal_index=True, reveal_scores=True), 2 * (T + D), 9, [100, 101, 102, 103],
     dict(scores=[105], index=104)),
    # include/linreg_gc_lasso_cv.h: the same layout, K (T + d) words per share
    (dict(CV, reveal_index=True, reveal_scores=True), 2 * (T + D), 15, [100, 101, 102, 103],
     dict(scores=[105, 106, 107], index=104, min_index=104, cv_curve=None)),
    # include/linreg_gc_ridge_cv.h: as linreg_gc_lasso_cv.h, L the number of lambdas
    (dict(lambdas=[0.1, 0.01], folds=3, reveal_index=True, reveal_scores=True), 3 * (T + D), 12, [100, 101, 102, 103],
     dict(scores=[105, 106], index=104)),
    # include/linreg_gc_lasso_cv_se.h: beta+ (d); l+, then l* (LGC_CV_RULE_MIN: l* alone); cv (L); mean (L), se (L); K words yy
    (dict(CV, rule="1se", reveal_index=True, reveal_scores=True, reveal_curve=True), 2 * (T + D) + 2, 15, [100, 101, 102, 103],
     dict(index=104, min_index=105, scores=[106, 107, 108], cv_curve=([109, 110, 111], [112, 113, 114]))),
    (dict(CV, rule="min", reveal_index=True, reveal_curve=True), 2 * (T + D) + 2, 15, [100, 101, 102, 103],
     dict(index=104, min_index=104, scores=None, cv_curve=([105, 106, 107], [108, 109, 110]))),
    (dict(CV, rule="1se", reveal_index=True), 2 * (T + D) + 2, 15, [100, 101, 102, 103],
     dict(index=104, min_index=105, scores=None, cv_curve=None)),
    (dict(CV, reveal_curve=True), 2 * (T + D) + 2, 15, [100, 101, 102, 103],
     dict(index=None, scores=None, cv_curve=([104, 105, 106], [107, 108, 109]))),
    (dict(CV, rule="1se", reveal_scores=True, reveal_curve=True), 2 * (T + D) + 2, 15, [100, 101, 102, 103],
     dict(scores=[104, 105, 106], cv_curve=([107, 108, 109], [110, 111, 112]))),
    # include/linreg_gc_inference.h: beta (d), [u (d)], [s2, r2]; every share [A, b, yy]; room for 2 d + 2
    (dict(inference=("se", "fit"), resid_scale=1.25), T + D + 1, 10, [100, 101, 102, 103],
     dict(std_err_words=[104, 105, 106, 107], sigma2_word=108, r2_word=109)),
    (dict(inference="se", resid_scale=1.25), T + D + 1, 10, [100, 101, 102, 103],
     dict(std_err_words=[104, 105, 106, 107], sigma2_word=None, r2_word=None)),
    (dict(inference="fit", resid_scale=1.25), T + D + 1, 10, [100, 101, 102, 103],
     dict(std_err_words=None, sigma2_word=104, r2_word=105)),
    # include/linreg_gc_scan.h: beta_0 .. beta_{M-1}, [w_0 .. w_{M-1}]; c = d - 1 = 3: T_c + c + 1 + M (c + 2) words per share
    (dict(scan=2, scan_se=True, resid_scale=1.5), 6 + 3 + 1 + 2 * 5, 4, [100, 101], dict(scan_std_err_words=[102, 103])),
    (dict(scan=2), 6 + 3 + 1 + 2 * 5, 2, [100, 101], dict(scan_std_err_words=None)),
]


def _plain(v):
    if isinstance(v, tuple):
        return tuple(_plain(x) for x in v)
    return v.tolist() if isinstance(v, np.ndarray) else v


@pytest.mark.parametrize("case", range(len(LAYOUT)))
def test_revealed_words_go_where_the_headers_say(gen, binding, monkeypatch, case):
    kw, in_words, size, beta, rest = LAYOUT[case]
    lg = binding
    seen = {}

    class Finishing(gen.Stub):
        def lgc_party_finish(self, h, dec, out, trace, inputs):
            seen.update(out=out.size, inputs=inputs.size)
            out.reshape(-1)[:] = 100 + np.arange(out.size)
            return 0
    monkeypatch.setattr(lg, "_lib", Finishing())
    monkeypatch.setattr(lg, "_vp", lambda a: a)                      # (the stub takes the arrays themselves)
    alg = "lasso" if "l1" in kw or "l1_ratios" in kw else "cholesky"
    sysm = lg.make_system(D, 64, 56, alg, 2 if alg == "lasso" else 0, 0.015625, 2, 1, 0, 0)
    party = lg.Party(sysm, lg.EVALUATOR, **kw)
    for name in rest:
        if name not in ("index", "min_index"):
            with pytest.raises(lg.LgcError, match=r"follows? finish\(\)"):
                getattr(party, name)()
    got, trace, inputs = party.finish(np.zeros(1, dtype=np.uint64))
    assert seen == dict(out=size, inputs=in_words) and inputs.shape == (in_words,)
    assert got.dtype == np.int64 and got.tolist() == beta
    for name, want in rest.items():
        if name in ("index", "min_index"):                           # (the accessors ask the library; the words are split all the same)
            assert getattr(party._req.split(100 + np.arange(size)), name) == want, name
        else:
            assert _plain(getattr(party, name)()) == want, name
    if "scan" in kw:
        s = party.scan_summary(4)
        assert s["beta"].tolist() == [100 / 2.0 ** 56, 101 / 2.0 ** 56]
        assert (s["std_err"] is None) if not kw.get("scan_se") else s["std_err"].tolist() == [102 / 2.0 ** 56 / 2, 103 / 2.0 ** 56 / 2]
    if "inference" in kw:
        s = party.summary(4)
        assert (s["std_err"] is None) == (rest["std_err_words"] is None) and (s["r2"] is None) == (rest["r2_word"] is None)
        if rest["r2_word"] is not None:
            assert s["r2"] == rest["r2_word"] / 2.0 ** 56 and s["sigma2"] == rest["sigma2_word"] / 2.0 ** 56 * D    # normalize = 1
    # what the program does not reveal is refused by name, as before
    if "validation" not in kw and "folds" not in kw:
        with pytest.raises(lg.LgcError, match=r"scores follows finish\(\) of a model selection"):
            party.scores()
    if "inference" not in kw:
        with pytest.raises(lg.LgcError, match="the inference words follow"):
            party.sigma2_word()
    if "scan" not in kw:
        with pytest.raises(lg.LgcError, match="the scan words follow"):
            party.scan_summary(4)
