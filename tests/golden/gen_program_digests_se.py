#!/usr/bin/env python3
"""Pins the programs and the new rejections of include/linreg_gc_lasso_cv_se.h.

    python tests/golden/gen_program_digests_se.py     # rewrites tests/golden/program_digests_se.json

In the manner of gen_program_digests.py, whose digest and system helpers it uses: sha256 digests of the records, the launch
list and every lgc_program_info field of K = 2, 3, 5 with the rule on / off and the curve on / off at both widths on both
input paths; and the (code, message) of one invalid request per new check through Program, Solver and Party creation.
tests/test_program_digests_se.py rebuilds both and compares."""
import ctypes as C
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "program_digests_se.json")


def _base():
    spec = importlib.util.spec_from_file_location("gen_program_digests", os.path.join(HERE, "gen_program_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# K -> (d, the values, out of order, and their mode): K = 5 takes nine values (the two-level minimum tree), K = 3 options
SHAPES = {2: (17, dict(l1_ratios=[0.1, 1.0, 0.5])), 3: (6, dict(l1=[0.05, 0.2, 0.1])), 5: (5, dict(l1=[0.4 * 0.7 ** ((3 * k) % 9) for k in range(9)]))}


def programs(lgc):
    g = _base()
    out = []
    for w in (32, 64):
        for nz in (0, 1):
            for K, (d, vals) in sorted(SHAPES.items()):
                opts = g.lasso_options(d) if K == 3 else {}
                for rule in ("min", "1se"):
                    for curve in (False, True):
                        name = "w%d norm%d cv%d d%d rule %s curve%d" % (w, nz, K, d, rule, curve)
                        out.append((name, lambda lgc, w=w, nz=nz, K=K, d=d, vals=vals, opts=opts, rule=rule, curve=curve:
                                    lgc.Program(g._sys(lgc, d, w, "lasso", 3, nz, 1), folds=K, rule=rule, reveal_curve=curve,
                                                reveal_index=True, reveal_scores=curve, **vals, **opts)))
            out.append(("w%d norm%d cv4 d5 L1 rule 1se curve1" % (w, nz), lambda lgc, w=w, nz=nz:
                        lgc.Program(g._sys(lgc, 5, w, "lasso", 3, nz, 1), folds=4, rule="1se", reveal_curve=True, reveal_index=True, l1=[g.L1])))
    return out


def build_digests(lgc):
    g = _base()
    res = {}
    for name, fn in programs(lgc):
        prog = fn(lgc)
        res[name] = g.digest(prog)
        prog.close()
    return res


def rejections():
    """(name, system fields, folds, reveal flags, rule)"""
    la = dict(d=5, w=64, alg="lasso", iters=2, normalize=1)
    return [("rule 2", la, 3, 0, 2), ("rule -1", la, 3, 0, -1), ("reveal flags 8", la, 3, 8, 1), ("rule before the flags", la, 3, 8, 2),
            ("folds before the rule", la, 1, 0, 2), ("folds 17", la, 17, 7, 1), ("trace", dict(la, trace=1), 3, 4, 1),
            ("too large for 31-bit word ids", dict(la, d=4096, nshares=16), 16, 4, 1)]


def build_rejections(lgc):
    g = _base()
    L = lgc.lib()
    res = {}
    vals = (C.c_double * 2)(0.1, 0.05)
    o = lgc.LassoOpts(2, C.cast(vals, C.c_void_p), 0, None, None, None)
    seed = bytes(range(16))
    for name, spec, folds, flags, rule in rejections():
        sysm = g._raw_system(lgc, spec)
        for kind in ("program", "solver", "party"):
            h = C.c_void_p()
            if kind == "program": rc = L.lgc_program_build_lasso_cv_se(C.byref(h), C.byref(sysm), C.byref(o), folds, flags, rule)
            elif kind == "solver": rc = L.lgc_solver_create_lasso_cv_se(C.byref(h), 0, C.byref(sysm), seed, C.byref(o), folds, flags, rule)
            else: rc = L.lgc_party_create_lasso_cv_se(C.byref(h), 0, C.byref(sysm), 1, seed, 0, C.byref(o), folds, flags, rule)
            assert rc != 0 and not h.value, (kind, name, rc)
            res["%s: cv_se %s" % (kind, name)] = [int(rc), L.lgc_last_error().decode()]
    for kind, call in (("program", lambda h, s: L.lgc_program_build_lasso_cv_se(C.byref(h), C.byref(s), None, 3, 0, 1)),
                       ("solver", lambda h, s: L.lgc_solver_create_lasso_cv_se(C.byref(h), 0, C.byref(s), seed, None, 3, 0, 1)),
                       ("party", lambda h, s: L.lgc_party_create_lasso_cv_se(C.byref(h), 0, C.byref(s), 1, seed, 0, None, 3, 0, 1))):
        h = C.c_void_p()
        rc = call(h, g._raw_system(lgc, rejections()[0][1]))
        assert rc != 0 and not h.value
        res["%s: cv_se null opts" % kind] = [int(rc), L.lgc_last_error().decode()]
    return res


def main():
    root = os.path.dirname(os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(root, "linreg-mpc_amd", "python"))
    import linreg_gc as lgc
    progs, rej = build_digests(lgc), build_rejections(lgc)
    with open(OUT, "w") as f:
        json.dump({"programs": progs, "rejections": rej}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d programs, %d rejections -> %s" % (len(progs), len(rej), OUT))


if __name__ == "__main__":
    main()
