"""Device seconds of a lasso path with in-circuit model selection (B, lgc_solver_create_lasso_select) against the plain path
that reveals every model (A, lgc_solver_create_lasso_path) on the same training system, in one process: A B A B, then A A for
the run-to-run spread.  One JSON line per dimension:
   python tests/tools/gpu_lasso_select.py [--d 100 500] [--L 8] [--iters 15] [--width 64 --precision 56] [--profile]
Times are stats()["seconds_total"] (input labels + garble + evaluate + decode).  "time_ratio" is median B / median A,
"gate_ratio" the AND gates of the two lowered programs, "aa_spread" |A - A| / A of the last two runs.  --profile runs B once
more with the two roles serialised and sums the per-launch seconds of everything after the last iteration ("selection_s":
setup, scoring products, merges, minimum tree, one-hot, gated select, reveal) and of the input launches before the first
product ("inputs_s").  beta* is checked to be row l* of A's betas."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "linreg-mpc_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import linreg_gc as lgc  # noqa: E402
from helpers import split_shares  # noqa: E402


def _words(M, v, d, p):
    A = np.array([int(M[i][j] * 2.0 ** p) for i in range(d) for j in range(i + 1)], dtype=np.int64).astype(np.uint64)
    return A, np.array([int(x * 2.0 ** p) for x in v], dtype=np.int64).astype(np.uint64)


def _run(sysm, shares, profile=False, **kw):
    s = lgc.Solver(sysm, seed=bytes(range(16)), **kw)
    s.set_shares(shares)
    s.run(profile=profile)
    st, beta = s.stats(), s.beta()
    out = dict(st=st, beta=beta, index=s.selected_index() if kw.get("validation") else None)
    if profile:
        g, e = s.profile(st["launches"])
        out["launch_s"] = g + e
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, nargs="+", default=[100, 500])
    ap.add_argument("--L", type=int, default=8)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--precision", type=int, default=56)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    w, p = a.width, a.precision
    ratios = [0.9 * 0.6 ** l for l in range(a.L)]
    for d in a.d:
        rng = np.random.default_rng(d)
        beta = rng.random(d) * (rng.random(d) < 0.3)
        halves = []
        for rows in (3 * d, 2 * d):
            X = rng.standard_normal((rows, d)); X /= np.abs(X).max(axis=0)
            y = X @ beta + 0.1 * rng.standard_normal(rows)
            halves.append(split_shares(rng, *_words(X.T @ X / (rows * d), X.T @ y / (rows * d), d, p), 2, w))
        train, both = halves[0], np.ascontiguousarray(np.hstack(halves))
        sysm = lgc.make_system(d, w, p, "lasso", a.iters, 1e-3, 2, 1, 0, 0)
        sel = dict(l1_ratios=ratios, validation=True, reveal_index=True)
        t = {"A": [], "B": []}
        for _ in range(2):
            ra = _run(sysm, train, l1_ratios=ratios)
            t["A"].append(ra["st"]["seconds_total"])
            rb = _run(sysm, both, **sel)
            t["B"].append(rb["st"]["seconds_total"])
            assert 0 <= rb["index"] < a.L and (ra["beta"][rb["index"]] == rb["beta"]).all(), "beta* is not row l* of the path"
        aa = [_run(sysm, train, l1_ratios=ratios)["st"]["seconds_total"] for _ in range(2)]
        out = {"d": d, "L": a.L, "width": w, "iters": a.iters, "ratios": ratios, "seconds": t, "aa_seconds": aa,
               "selected": rb["index"],
               "time_ratio": statistics.median(t["B"]) / statistics.median(t["A"]),
               "aa_spread": abs(aa[0] - aa[1]) / min(aa),
               "and_gates": {"A": ra["st"]["and_gates"], "B": rb["st"]["and_gates"]},
               "gate_ratio": rb["st"]["and_gates"] / ra["st"]["and_gates"],
               "launches": {"A": ra["st"]["launches"], "B": rb["st"]["launches"]}}
        if a.profile:
            prog = lgc.Program(sysm, **sel)
            ops = np.frombuffer(prog.records().tobytes(), dtype=np.uint32).reshape(-1, 10)[:, 0]
            first = [Lc["first_rec"] for Lc in prog.launches()]
            prox = [i for i, f in enumerate(first) if ops[f] == 26]
            mac = [i for i, f in enumerate(first) if ops[f] in (1, 19, 20)]
            pr = _run(sysm, both, profile=True, **sel)
            ls = pr["launch_s"]
            out["profile"] = {"total_s": float(ls.sum()), "inputs_s": float(ls[:mac[0]].sum()),
                              "selection_s": float(ls[prox[-1] + 1:].sum()),
                              "selection_mac_s": float(sum(ls[i] for i in mac if i > prox[-1])),
                              "iterations_s": float(ls[mac[0]:prox[-1] + 1].sum())}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
