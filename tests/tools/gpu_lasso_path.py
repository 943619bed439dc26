"""Device seconds of a lasso path against L single lasso solves on the same system, alternated A B A B in one process, one
JSON line per dimension:
   python tests/tools/gpu_lasso_path.py [--d 100 500] [--L 8] [--iters 15] [--rounds 2] [--width 64 --precision 56]
A is one absolute path of L values of lambda1 (lgc_solver_create_lasso_path); B is L solves with lgc_solver_create_lasso, one
per value, and its time is their sum.  Times are stats()["seconds_total"] (input labels + garble + evaluate + decode) of
each run; "path_over_singles" is the ratio of the medians.  Both give the same L betas, bit for bit (checked)."""
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


def _solve(sysm, shares, l1):
    s = lgc.Solver(sysm, seed=bytes(range(16)), l1=l1)
    s.set_shares(shares)
    s.run()
    st, beta = s.stats(), s.beta()
    s.close()
    return st, beta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, nargs="+", default=[100, 500])
    ap.add_argument("--L", type=int, default=8)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--precision", type=int, default=56)
    a = ap.parse_args()
    w, p = a.width, a.precision
    oracle = orc.load()
    values = [0.0005 * 1.6 ** l for l in range(a.L)]
    for d in a.d:
        rng = np.random.default_rng(d)
        A, b = synth_system(oracle, rng, 3 * d, d, w, p)
        shares = split_shares(rng, A, b, 2, w)
        sysm = lgc.make_system(d, w, p, "lasso", a.iters, 1e-3, 2, 1, 0, 0)
        runs = {"path": [], "singles": []}
        info = {}
        for _ in range(a.rounds):
            st, beta_path = _solve(sysm, shares, values)
            runs["path"].append(st["seconds_total"])
            info["path"] = {"and_gates": st["and_gates"], "launches": st["launches"]}
            t, gates, launches, betas = 0.0, 0, 0, []
            for v in values:
                st, beta = _solve(sysm, shares, v)
                t += st["seconds_total"]; gates += st["and_gates"]; launches += st["launches"]
                betas.append(beta)
            runs["singles"].append(t)
            info["singles"] = {"and_gates": gates, "launches": launches}
            assert (np.array(betas) == beta_path).all(), "the path and the single solves disagree"
        out = {"d": d, "L": a.L, "width": w, "iters": a.iters, "l1": values, "seconds": runs,
               "path_over_singles": statistics.median(runs["path"]) / statistics.median(runs["singles"])}
        out.update(info)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
