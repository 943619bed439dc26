"""Device seconds of the lasso solver against CGD on the same system, alternated A B A B in one process, one JSON line:
   python tests/tools/gpu_lasso.py --d 500 --iters 15 [--rounds 2] [--l1 0.001] [--width 64 --precision 56]
A is lasso with N = --iters (N - 1 matrix-vector products), B is CGD with --iters iterations.  Times are
stats()["seconds_total"] (input labels + garble + evaluate + decode) of each run; "lasso_over_cgd" is the ratio of the medians."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "linreg-mpc_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import linreg_gc as lgc  # noqa: E402
import orc  # noqa: E402
from helpers import split_shares, synth_system  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=500)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--l1", type=float, default=0.001)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--precision", type=int, default=56)
    a = ap.parse_args()
    d, w, p = a.d, a.width, a.precision
    oracle = orc.load()
    rng = np.random.default_rng(d)
    A, b = synth_system(oracle, rng, 3 * d, d, w, p)
    shares = split_shares(rng, A, b, 2, w)
    runs = {"lasso": [], "cgd": []}
    info = {}
    for _ in range(a.rounds):
        for alg in ("lasso", "cgd"):
            sysm = lgc.make_system(d, w, p, alg, a.iters, 1e-3, 2, 1, 0, 0)
            s = lgc.Solver(sysm, seed=bytes(range(16)), l1=a.l1 if alg == "lasso" else None)
            s.set_shares(shares)
            s.run()
            st = s.stats()
            if alg == "lasso":
                info["lasso_zeros"] = int((s.beta() == 0).sum())
            s.close()
            runs[alg].append(st["seconds_total"])
            info[alg] = {"and_gates": st["and_gates"], "launches": st["launches"]}
    out = {"d": d, "width": w, "iters": a.iters, "l1": a.l1, "seconds": runs,
           "lasso_over_cgd": statistics.median(runs["lasso"]) / statistics.median(runs["cgd"])}
    out.update(info)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
