#!/usr/bin/env python3
"""Pins what the Python binding makes of a program request: the C call and its arguments, or the refusal.

    python tests/golden/gen_binding_calls.py [DIR]      # rewrites tests/golden/binding_calls.json

DIR: a directory whose linreg_gc.py is recorded instead of the tree's (it goes first on sys.path).  The fixture is a record of
the binding BEFORE a change to it, never of the code under test: to regenerate it for a change of the binding, take the
parent commit's file (`git show HEAD~:linreg-mpc_amd/python/linreg_gc.py > DIR/linreg_gc.py`) and pass DIR.

In the manner of gen_program_digests.py, without the library: linreg_gc._lib is replaced by a stub whose every function
records (name, arguments by value) and returns 0, so each of Program, Solver and Party runs its Python-side checks and makes
its one creation call into the stub.  Per case and front the fixture holds {"call": [name, arguments], "attrs": {..}} or
{"error": the LgcError's text}.  tests/test_binding_requests_cpu.py replays the cases and compares."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "binding_calls.json")
FRONTS = ("Program", "Solver", "Party")
ATTRS = ("path", "folds", "select", "rule", "infer", "scan", "targets", "count")
CREATION = ("lgc_program_build", "lgc_solver_create", "lgc_party_create")
UNSET = "<unset>"
INF = float("inf")
L2, L3 = [0.1, 0.01], [0.5, 0.25, 0.125]
D4 = dict(lower=[-1.0, -INF, 0.0, -0.5], upper=[1.0, INF, 2.0, 0.5], penalty_factors=[1.0, 0.0, 2.0, 0.5])


class Stub:
    """stands in for the loaded library: every attribute is a function that records (name, normalised arguments), returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            # (by value, at once: the arrays behind the pointers are alive now; of the other calls the name is enough)
            self.calls.append((name, normalise(args) if name.startswith(CREATION) else None))
            return 0
        fn.__name__ = name
        return fn


def _doubles(addr, n):
    return None if not addr else [float(v) for v in (C.c_double * n).from_address(addr)]


def _struct(s, d):
    f = {k: getattr(s, k) for k, _ in s._fields_}
    if "l1_count" in f:                                   # struct lgc_lasso_opts: its arrays read out
        f["l1"] = _doubles(f["l1"], f["l1_count"])
        for k in ("penalty_factors", "lower", "upper"):
            f[k] = _doubles(f[k], d)
    return f


def normalise(args):
    """arguments by value: scalars as they are, byref structs through their fields (the handle a call returns through as
    "out"), a pointer to doubles as the list of the count before it, bytes (the seed) as hex"""
    out, d = [], None
    for a in args:
        if type(a).__name__ == "CArgObject":              # C.byref(..)
            a = a._obj
            if isinstance(a, C.c_void_p):
                out.append("out")
            else:
                f = _struct(a, d)
                d = f.get("d", d)                         # (the system comes before the options in every call)
                out.append(f)
        elif isinstance(a, C.c_void_p):
            out.append(_doubles(a.value, out[-1]))
        elif isinstance(a, (bytes, bytearray)):
            out.append(bytes(a).hex())
        elif isinstance(a, (bool, np.bool_)):
            out.append(int(a))
        elif isinstance(a, (int, np.integer)):
            out.append(int(a))
        elif isinstance(a, (float, np.floating)):
            out.append(float(a))
        else:
            assert a is None, a
            out.append(None)
    return out


def _jsonable(v):
    return [_jsonable(x) for x in v] if isinstance(v, (tuple, list)) else v


def cases():
    """(name, fronts, d, algorithm, keywords).  d = 4 (a scan: c = 2 covariates, d = 3, M = 2)"""
    ALL, PS = FRONTS, ("Program", "Solver")
    sel = dict(l1_ratios=L3, validation=True)
    cv = dict(l1_ratios=L3, folds=2)
    rcv = dict(lambdas=L2, folds=3)
    inf = dict(inference=("se", "fit"), resid_scale=1.25)
    out = [
        # ---- the twelve kinds and their variants
        ("plain", ALL, "cgd", {}),
        ("targets", ALL, "cholesky", dict(targets=2)),
        ("sweep", ALL, "cgd", dict(lambdas=L2)),                            # (a party refuses a plain sweep)
        ("sweep first", PS, "cgd", dict(lambdas=L3, first=5)),
        ("lasso scalar", ALL, "lasso", dict(l1=0.003)),
        ("lasso one element", ALL, "lasso", dict(l1=[0.003])),
        ("lasso path absolute", ALL, "lasso", dict(l1=L2)),
        ("lasso path ratio", ALL, "lasso", dict(l1_ratios=L3)),
        ("lasso path ratio scalar", ALL, "lasso", dict(l1_ratios=0.5)),
        ("opts positive scalar", ALL, "lasso", dict(l1=0.003, positive=True)),
        ("opts lower upper path", ALL, "lasso", dict(l1=L2, lower=D4["lower"], upper=D4["upper"])),
        ("opts penalty ratio", ALL, "lasso", dict(l1_ratios=L3, penalty_factors=D4["penalty_factors"])),
        ("opts positive upper", ALL, "lasso", dict(l1=[0.003], positive=True, upper=D4["upper"])),
        ("select", ALL, "lasso", dict(sel)),
        ("select index", ALL, "lasso", dict(sel, reveal_index=True)),
        ("select scores", ALL, "lasso", dict(sel, reveal_scores=True)),
        ("select both absolute", ALL, "lasso", dict(l1=L2, validation=True, reveal_index=True, reveal_scores=True)),
        ("select scalar", ALL, "lasso", dict(l1=0.003, validation=True, reveal_index=True)),
        ("select opts", ALL, "lasso", dict(sel, positive=True, penalty_factors=D4["penalty_factors"])),
        ("cv", ALL, "lasso", dict(cv)),
        ("cv index scores", ALL, "lasso", dict(cv, reveal_index=True, reveal_scores=True)),
        ("cv scalar", ALL, "lasso", dict(l1=0.003, folds=2)),
        ("cv one element bounds", ALL, "lasso", dict(l1=[0.003], folds=3, lower=D4["lower"])),
        ("cv se min", ALL, "lasso", dict(cv, rule="min")),
        ("cv se 1se index", ALL, "lasso", dict(cv, rule="1se", reveal_index=True)),
        ("cv se curve alone", ALL, "lasso", dict(cv, reveal_curve=True)),
        ("cv se 1se all", ALL, "lasso", dict(cv, rule="1se", reveal_index=True, reveal_scores=True, reveal_curve=True)),
        ("cv se scalar", ALL, "lasso", dict(l1=0.003, folds=2, rule="1se")),
        ("cv se opts", ALL, "lasso", dict(l1=L2, folds=2, rule="min", reveal_curve=True, positive=True)),
        ("ridge cv", ALL, "cgd", dict(rcv)),
        ("ridge cv index", ALL, "cholesky", dict(rcv, reveal_index=True)),
        ("ridge cv scores", ALL, "ldlt", dict(rcv, reveal_scores=True)),
        ("ridge cv both scalar", ALL, "cgd", dict(lambdas=0.1, folds=2, reveal_index=True, reveal_scores=True)),
        ("inference tuple", ALL, "cholesky", dict(inf)),
        ("inference se string", ALL, "cholesky", dict(inference="se", resid_scale=1.5)),
        ("inference fit string", ALL, "cholesky", dict(inference="fit", resid_scale=1.0625)),
        ("inference fit list", ALL, "cholesky", dict(inference=["fit"], resid_scale=2.0)),
        ("scan", ALL, "cholesky", dict(scan=2)),
        ("scan se", ALL, "cholesky", dict(scan=2, scan_se=True, resid_scale=1.5)),
        ("scan none", ALL, "cholesky", dict(scan=0)),
        # ---- every refusal of the helpers
        ("no: sweep with targets", ALL, "cgd", dict(lambdas=L2, targets=2)),
        ("no: l1 with sweep", ALL, "lasso", dict(l1=0.1, lambdas=L2)),
        ("no: ratios with targets", ALL, "lasso", dict(l1_ratios=L3, targets=2)),
        ("no: l1 and ratios", ALL, "lasso", dict(l1=0.1, l1_ratios=L3)),
        ("no: validation and folds", ALL, "lasso", dict(l1=L2, validation=True, folds=2)),
        ("no: index without selection", ALL, "lasso", dict(l1=L2, reveal_index=True)),
        ("no: scores without selection", ALL, "cgd", dict(reveal_scores=True)),
        ("no: validation without path", ALL, "lasso", dict(validation=True)),
        ("no: folds without path", ALL, "lasso", dict(folds=2)),
        ("no: ridge cv validation", ALL, "cgd", dict(rcv, validation=True)),
        ("no: ridge cv lasso", ALL, "lasso", dict(rcv)),
        ("no: ridge cv first", PS, "cgd", dict(rcv, first=1)),
        ("no: ridge cv rule", ALL, "cgd", dict(rcv, rule="min")),
        ("no: ridge cv curve", ALL, "cgd", dict(rcv, reveal_curve=True)),
        ("no: resid_scale alone", ALL, "cholesky", dict(resid_scale=1.25)),
        ("no: inference with others", ALL, "cholesky", dict(inf, targets=2, l1=0.1, positive=True)),
        ("no: inference with first", PS, "cholesky", dict(inf, first=1)),
        ("no: inference unknown", ALL, "cholesky", dict(inference=("se", "r2"), resid_scale=1.25)),
        ("no: inference without resid_scale", ALL, "cholesky", dict(inference="se")),
        ("no: scan_se alone", ALL, "cholesky", dict(scan_se=True)),
        ("no: scan with others", ALL, "cholesky", dict(scan=2, folds=2, reveal_curve=True, lambdas=L2)),
        ("no: scan with first", PS, "cholesky", dict(scan=2, first=2)),
        ("no: scan_se without resid_scale", ALL, "cholesky", dict(scan=2, scan_se=True)),
        ("no: scan resid_scale without se", ALL, "cholesky", dict(scan=2, resid_scale=1.5)),
        ("no: scan negative", ALL, "cholesky", dict(scan=-1)),
        ("no: rule without folds", ALL, "lasso", dict(l1=L2, rule="min")),
        ("no: curve without folds", ALL, "lasso", dict(l1=L2, validation=True, reveal_curve=True)),
        ("no: rule unknown", ALL, "lasso", dict(cv, rule="2se")),
        ("no: positive and lower", ALL, "lasso", dict(l1=0.1, positive=True, lower=D4["lower"])),
        ("no: options without l1", ALL, "cgd", dict(upper=D4["upper"])),
        ("no: lower short", ALL, "lasso", dict(l1=0.1, lower=[0.0] * 3)),
        ("no: upper long", ALL, "lasso", dict(l1=L2, upper=[1.0] * 5)),
        ("no: penalty_factors short", ALL, "lasso", dict(cv, penalty_factors=[1.0])),
        # ---- two things wrong at once: which refusal wins
        ("first of two: scan over inference", ALL, "cholesky", dict(inf, scan=2)),
        ("first of two: scan_se alone over resid_scale alone", ALL, "cholesky", dict(scan_se=True, resid_scale=1.5)),
        ("first of two: scan resid_scale over negative", ALL, "cholesky", dict(scan=-1, scan_se=True)),
        ("first of two: inference others over unknown", ALL, "cholesky", dict(inference="r2", targets=2)),
        ("first of two: inference unknown over resid_scale", ALL, "cholesky", dict(inference="r2")),
        ("first of two: sweep targets over lasso mix", ALL, "lasso", dict(lambdas=L2, targets=2, l1=0.1)),
        ("first of two: l1 and ratios over lasso mix", ALL, "lasso", dict(l1=0.1, l1_ratios=L3, lambdas=L2)),
        ("first of two: lasso mix over ridge cv", ALL, "lasso", dict(rcv, l1=L2)),
        ("first of two: ridge cv lasso over first", PS, "lasso", dict(rcv, first=1)),
        ("first of two: ridge cv first over rule", PS, "cgd", dict(rcv, first=1, rule="min")),
        ("first of two: sweep targets over party", ALL, "cgd", dict(lambdas=L2, targets=2, reveal_index=True)),
        ("first of two: party over reveal flags", ALL, "cgd", dict(lambdas=L2, reveal_index=True)),
        ("first of two: party over options", ALL, "cgd", dict(lambdas=L2, positive=True, lower=D4["lower"])),
        ("first of two: reveal flags over options", ALL, "cgd", dict(reveal_index=True, positive=True)),
        ("first of two: selection without path over options", ALL, "lasso", dict(folds=2, positive=True, lower=D4["lower"])),
        ("first of two: positive and lower over no l1", ALL, "cgd", dict(positive=True, lower=D4["lower"])),
        ("first of two: options over rule", ALL, "lasso", dict(l1=0.1, upper=[1.0], rule="min")),
        ("first of two: rule without folds over unknown", ALL, "lasso", dict(l1=L2, rule="2se")),
    ]
    return [(name, fronts, 3 if "scan" in kw else 4, alg, kw) for name, fronts, alg, kw in out]


def make(lgc, front, d, alg, kw):
    """the object of one case on one front.  Solver: a seed and a device of its own; Party: the garbler with a seed and a table
    cap, except that every other case is the evaluator without either"""
    sysm = lgc.make_system(d, 64, 56, alg, 2 if alg in ("cgd", "lasso") else 0, 0.015625, 2, 1, 0, 0)
    if front == "Program":
        return lgc.Program(sysm, **kw)
    if front == "Solver":
        return lgc.Solver(sysm, seed=bytes(range(16)), device=3, **kw)
    if len(kw) % 2:
        return lgc.Party(sysm, lgc.EVALUATOR, **kw)
    return lgc.Party(sysm, lgc.GARBLER, seed=bytes(range(16, 32)), device=1, max_launch_table_bytes=1 << 25, **kw)


def record(lgc):
    """{case: {front: {"call": [name, arguments], "attrs": {..}} or {"error": text}}} of lgc with a stub for its library"""
    res = {}
    saved, stub = lgc._lib, Stub()
    lgc._lib = stub
    try:
        for name, fronts, d, alg, kw in cases():
            assert name not in res, name
            res[name] = {}
            for front in fronts:
                del stub.calls[:]
                try:
                    obj = make(lgc, front, d, alg, kw)
                except lgc.LgcError as e:
                    assert not stub.calls, (name, front, stub.calls)
                    res[name][front] = {"error": str(e)}
                    continue
                made = [c for c in stub.calls if c[0].startswith(CREATION)]
                assert len(made) == 1, (name, front, stub.calls)
                res[name][front] = {"call": [made[0][0], made[0][1]],
                                    "attrs": {a: _jsonable(getattr(obj, a, UNSET)) for a in ATTRS}}
    finally:
        lgc._lib = saved
    return res


def main():
    root = os.path.dirname(os.path.dirname(HERE))
    sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "linreg-mpc_amd", "python"))
    import linreg_gc as lgc
    with open(OUT, "w") as f:
        json.dump({"cases": record(lgc)}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, "from", lgc.__file__)


if __name__ == "__main__":
    main()
