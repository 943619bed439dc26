"""Device seconds of a lasso path cross-validated over K folds in the circuit (B, lgc_solver_create_lasso_cv) against K + 1
plain paths that reveal every model (A, lgc_solver_create_lasso_path, one after the other on systems of the same size), in
one process: A B A B, then A A for the run-to-run spread.  One JSON line per dimension:
   python tests/tools/gpu_lasso_cv.py [--d 100] [--K 5] [--L 8] [--iters 15] [--width 64 --precision 56]
Times are stats()["seconds_total"] (input labels + garble + evaluate + decode), A's summed over its K + 1 solves.
"time_ratio" is median B / median A, "gate_ratio" the AND gates of B over those of ONE plain path (predicted
(K + 1) + K / (iters - 1)), "aa_spread" |A - A| / A of the last two runs.  beta* is checked to be row l* of the plain path on
the full system: shares whose folds are all equal make the full system the fold itself, whatever K."""
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


def _run(sysm, shares, **kw):
    s = lgc.Solver(sysm, seed=bytes(range(16)), **kw)
    s.set_shares(shares)
    s.run()
    out = dict(st=s.stats(), beta=s.beta(), index=s.selected_index() if kw.get("folds") else None)
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
    a = ap.parse_args()
    w, p, K = a.width, a.precision, a.K
    ratios = [0.9 * 0.6 ** l for l in range(a.L)]
    for d in a.d:
        rng = np.random.default_rng(d)
        beta = rng.random(d) * (rng.random(d) < 0.3)
        folds = []
        for _ in range(K):
            rows = 3 * d
            X = rng.standard_normal((rows, d)); X /= np.abs(X).max(axis=0)
            y = X @ beta + 0.1 * rng.standard_normal(rows)
            folds.append(split_shares(rng, *_words(X.T @ X / (rows * d), X.T @ y / (rows * d), d, p), 2, w))
        cv_shares = np.ascontiguousarray(np.hstack(folds))
        sysm = lgc.make_system(d, w, p, "lasso", a.iters, 1e-3, 2, 1, 0, 0)
        cv = dict(l1_ratios=ratios, folds=K, reveal_index=True)

        def plain_paths():
            runs = [_run(sysm, folds[k % K], l1_ratios=ratios) for k in range(K + 1)]
            return sum(r["st"]["seconds_total"] for r in runs), runs[0]["st"]
        t = {"A": [], "B": []}
        for _ in range(2):
            ta, sta = plain_paths()
            t["A"].append(ta)
            rb = _run(sysm, cv_shares, **cv)
            t["B"].append(rb["st"]["seconds_total"])
            assert 0 <= rb["index"] < a.L
        aa = [plain_paths()[0] for _ in range(2)]
        # K equal folds: every training system and the full system are the fold itself (sums of K equal words divide exactly)
        same = _run(sysm, np.ascontiguousarray(np.hstack([folds[0]] * K)), **cv)
        ref = _run(sysm, folds[0], l1_ratios=ratios)
        assert (ref["beta"][same["index"]] == same["beta"]).all(), "beta* is not row l* of the plain path on the full system"
        print(json.dumps({"d": d, "K": K, "L": a.L, "width": w, "iters": a.iters, "ratios": ratios, "seconds": t, "aa_seconds": aa,
                          "selected": rb["index"],
                          "time_ratio": statistics.median(t["B"]) / statistics.median(t["A"]),
                          "aa_spread": abs(aa[0] - aa[1]) / min(aa),
                          "and_gates": {"A_one_path": sta["and_gates"], "B": rb["st"]["and_gates"]},
                          "gate_ratio": rb["st"]["and_gates"] / sta["and_gates"],
                          "gate_ratio_predicted": (K + 1) + K / (a.iters - 1),
                          "launches": {"A_one_path": sta["launches"], "B": rb["st"]["launches"]}}), flush=True)


if __name__ == "__main__":
    main()
