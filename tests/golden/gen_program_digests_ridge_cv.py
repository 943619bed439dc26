#!/usr/bin/env python3
"""Pins the programs of include/linreg_gc_ridge_cv.h.

    python tests/golden/gen_program_digests_ridge_cv.py     # rewrites tests/golden/program_digests_ridge_cv.json

In the manner of gen_program_digests_se.py, with the digest and system helpers of gen_program_digests.py: sha256 digests of
the records, the launch list and every lgc_program_info field of the cross-validated ridge sweep at both widths on both input
paths, K = 2 and 3, cgd and cholesky, with the reveal flags and without, and one value (nothing scored).
tests/test_program_digests_ridge_cv.py rebuilds them and compares."""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "program_digests_ridge_cv.json")


def _base():
    spec = importlib.util.spec_from_file_location("gen_program_digests", os.path.join(HERE, "gen_program_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# K -> (d, the values of lambda, out of order)
SHAPES = {2: (7, [0.01, 0.5, 0.1]), 3: (6, [0.2, 0.001, 0.05, 0.01])}


def programs(lgc):
    g = _base()
    out = []
    for w in (32, 64):
        for nz in (0, 1):
            for K, (d, lams) in sorted(SHAPES.items()):
                for alg, iters in (("cgd", 3), ("cholesky", 0)):
                    for flags in (0, 3):
                        name = "w%d norm%d ridge cv%d d%d %s reveal%d" % (w, nz, K, d, alg, flags)
                        out.append((name, lambda lgc, w=w, nz=nz, K=K, d=d, lams=lams, alg=alg, iters=iters, flags=flags:
                                    lgc.Program(g._sys(lgc, d, w, alg, iters, nz), lambdas=lams, folds=K, reveal_index=bool(flags & 1),
                                                reveal_scores=bool(flags & 2))))
            out.append(("w%d norm%d ridge cv4 d5 L1 ldlt reveal3" % (w, nz), lambda lgc, w=w, nz=nz:
                        lgc.Program(g._sys(lgc, 5, w, "ldlt", 0, nz), lambdas=[0.03], folds=4, reveal_index=True, reveal_scores=True)))
    return out


def build_digests(lgc):
    g = _base()
    res = {}
    for name, fn in programs(lgc):
        prog = fn(lgc)
        res[name] = g.digest(prog)
        prog.close()
    return res


def main():
    root = os.path.dirname(os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(root, "linreg-mpc_amd", "python"))
    import linreg_gc as lgc
    with open(OUT, "w") as f:
        json.dump({"programs": build_digests(lgc)}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
