#!/usr/bin/env python3
"""Pins the programs of include/linreg_gc_inference.h.

    python tests/golden/gen_program_digests_inference.py     # rewrites tests/golden/program_digests_inference.json

In the manner of gen_program_digests_ridge_cv.py, with the digest and system helpers of gen_program_digests.py: sha256 digests
of the records, the launch list and every lgc_program_info field of the Cholesky solve with inference at both widths on both
input paths, the three reveal subsets and d = 1, 5, 65 and 184 (184: Karatsuba products in the factorisation at width 64).
tests/test_program_digests_inference.py rebuilds them and compares."""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "program_digests_inference.json")
SUBSETS = {1: ("se",), 2: ("fit",), 3: ("se", "fit")}
DIMS = (1, 5, 65, 184)
RESID_SCALE = 1.0625                              # (a dyadic value: the same word on every host)


def _base():
    spec = importlib.util.spec_from_file_location("gen_program_digests", os.path.join(HERE, "gen_program_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def programs(lgc):
    g = _base()
    out = []
    for w in (32, 64):
        for nz in (0, 1):
            for d in DIMS:
                for bits, names in sorted(SUBSETS.items()):
                    out.append(("w%d norm%d inference d%d reveal%d" % (w, nz, d, bits), lambda lgc, w=w, nz=nz, d=d, names=names:
                                lgc.Program(g._sys(lgc, d, w, "cholesky", 0, nz), inference=names, resid_scale=RESID_SCALE)))
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
