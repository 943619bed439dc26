"""Device seconds of a cross-validated lasso path with the one-standard-error rule (B, lgc_solver_create_lasso_cv_se with
LGC_CV_RULE_ONE_SE) against the same cross-validation with the arg-min (A, LGC_CV_RULE_MIN through the same call, on the same
shares), in one process: A B A B, then A A for the run-to-run spread.  One JSON line per dimension:
   python tests/tools/gpu_lasso_cv_se.py [--d 100] [--K 5] [--L 8] [--iters 15] [--width 64 --precision 56] [--profile]
Times are stats()["seconds_total"] (input labels + garble + evaluate + decode).  "time_ratio" is median B / median A,
"gate_ratio" the AND gates of B over A's, "aa_spread" |A - A| / A of the last two runs.  --profile adds one run of B with the
roles serialised per launch and reports the seconds of the launches the rule adds (those behind the last product launch)."""
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
    out = dict(st=s.stats(), beta=s.beta(), index=s.selected_index(), lmin=s.min_index())
    if profile:
        out["profile"] = s.profile(out["st"]["launches"])
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, nargs="+", default=[100])
    ap.add_argument("--K", type=int, default=5)
    ap.add_argument("--L", type=int, default=8)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--precision", type=int, default=56)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    w, p, K = a.width, a.precision, a.K
    ratios = [0.9 * 0.6 ** l for l in range(a.L)]
    for d in a.d:
        rng = np.random.default_rng(d)
        beta = rng.random(d) * (rng.random(d) < 0.3)
        folds, yy = [], np.zeros((2, K), dtype=np.uint64)
        for k in range(K):
            rows = 3 * d
            X = rng.standard_normal((rows, d)); X /= np.abs(X).max(axis=0)
            y = X @ beta + 0.1 * rng.standard_normal(rows)
            folds.append(split_shares(rng, *_words(X.T @ X / (rows * d), X.T @ y / (rows * d), d, p), 2, w))
            yy[1, k] = int(float(y @ y) / (rows * d) * 2.0 ** p)
        shares = np.ascontiguousarray(np.hstack(folds + [yy]))
        sysm = lgc.make_system(d, w, p, "lasso", a.iters, 1e-3, 2, 1, 0, 0)
        kw = dict(l1_ratios=ratios, folds=K, reveal_index=True)
        t = {"A": [], "B": []}
        for _ in range(2):
            ra = _run(sysm, shares, rule="min", **kw)
            t["A"].append(ra["st"]["seconds_total"])
            rb = _run(sysm, shares, rule="1se", **kw)
            t["B"].append(rb["st"]["seconds_total"])
            assert 0 <= rb["index"] <= rb["lmin"] < a.L and rb["lmin"] == ra["index"]      # (the ratios decrease: pi is the identity)
        aa = [_run(sysm, shares, rule="min", **kw)["st"]["seconds_total"] for _ in range(2)]
        out = {"d": d, "K": K, "L": a.L, "width": w, "iters": a.iters, "seconds": t, "aa_seconds": aa,
               "selected": rb["index"], "minimum": rb["lmin"],
               "time_ratio": statistics.median(t["B"]) / statistics.median(t["A"]),
               "aa_spread": abs(aa[0] - aa[1]) / min(aa),
               "and_gates": {"A": ra["st"]["and_gates"], "B": rb["st"]["and_gates"]},
               "gate_ratio": rb["st"]["and_gates"] / ra["st"]["and_gates"],
               "launches": {"A": ra["st"]["launches"], "B": rb["st"]["launches"]}}
        if a.profile:
            pr = _run(sysm, shares, profile=True, rule="1se", **kw)
            g, e = pr["profile"]
            prog = lgc.Program(sysm, rule="1se", **kw)
            last_mac = max(i for i, Lc in enumerate(prog.launches()) if Lc["mac_only"])
            out["profile"] = {"serialised_total": float(g.sum() + e.sum()), "after_last_product_launch": float(g[last_mac + 1:].sum() + e[last_mac + 1:].sum()),
                              "launches_after": len(g) - last_mac - 1}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
