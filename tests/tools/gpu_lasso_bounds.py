"""Device seconds of a lasso solve with every coordinate bounded against the same solve with no bound, alternated A B A B in one
process, one JSON line per dimension:
   python tests/tools/gpu_lasso_bounds.py [--d 100 500] [--iters 15] [--rounds 2] [--width 64 --precision 56]
A is lgc_solver_create_lasso_opts with lower = -0.5 and upper = 0.5 on every coordinate (every OP_PROX record carries the
clamp); B is lgc_solver_create_lasso with the same lambda1.  Times are stats()["seconds_total"] (input labels + garble +
evaluate + decode) of each run; "bounded_over_plain" is the ratio of the medians."""
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


def _solve(sysm, shares, **kw):
    s = lgc.Solver(sysm, seed=bytes(range(16)), **kw)
    s.set_shares(shares)
    s.run()
    st, beta = s.stats(), s.beta()
    s.close()
    return st, beta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, nargs="+", default=[100, 500])
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--precision", type=int, default=56)
    a = ap.parse_args()
    w, p, l1 = a.width, a.precision, 0.001
    oracle = orc.load()
    for d in a.d:
        rng = np.random.default_rng(d)
        A, b = synth_system(oracle, rng, 3 * d, d, w, p)
        shares = split_shares(rng, A, b, 2, w)
        sysm = lgc.make_system(d, w, p, "lasso", a.iters, 1e-3, 2, 1, 0, 0)
        runs = {"bounded": [], "plain": []}
        info = {}
        for _ in range(a.rounds):
            for name, kw in (("bounded", dict(lower=[-0.5] * d, upper=[0.5] * d)), ("plain", {})):
                st, beta = _solve(sysm, shares, l1=l1, **kw)
                runs[name].append(st["seconds_total"])
                info[name] = {"and_gates": st["and_gates"], "launches": st["launches"]}
            assert info["bounded"]["launches"] == info["plain"]["launches"]
        out = {"d": d, "width": w, "iters": a.iters, "l1": l1, "seconds": runs,
               "bounded_over_plain": statistics.median(runs["bounded"]) / statistics.median(runs["plain"])}
        out.update(info)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
