#!/usr/bin/env python3
"""Pins the programs of include/linreg_gc_scan.h.

    python tests/golden/gen_program_digests_scan.py     # rewrites tests/golden/program_digests_scan.json

In the manner of gen_program_digests_inference.py, with the digest and system helpers of gen_program_digests.py: sha256 digests
of the records, the launch list and every lgc_program_info field of the association scan at both widths on both input paths,
with and without LGC_SCAN_SE, c = 1, 2, 5 covariates and M = 1, 3, 40 candidates.  tests/test_program_digests_scan.py rebuilds
them and compares."""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "program_digests_scan.json")
COVARIATES = (1, 2, 5)
CANDIDATES = (1, 3, 40)
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
            for c in COVARIATES:
                for M in CANDIDATES:
                    for se in (0, 1):
                        out.append(("w%d norm%d scan c%d M%d se%d" % (w, nz, c, M, se), lambda lgc, w=w, nz=nz, c=c, M=M, se=se:
                                    lgc.Program(g._sys(lgc, c + 1, w, "cholesky", 0, nz), scan=M, scan_se=bool(se),
                                                resid_scale=RESID_SCALE if se else None)))
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
