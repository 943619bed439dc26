"""Device seconds of the ridge lambda sweep cross-validated over K folds in the circuit (B, lgc_solver_create_ridge_cv) against
the K + 1 existing sweeps of the same L values that reveal every model (A, lgc_solver_create_sweep, one after the other on
systems of the same size), in one process: A B A B, then A A for the run-to-run spread.  One JSON line per dimension:
   python tests/tools/gpu_ridge_cv.py [--d 100] [--K 5] [--L 8] [--alg cgd --iters 15] [--width 64 --precision 56]
Times are stats()["seconds_total"] (input labels + garble + evaluate + decode), A's summed over its K + 1 solves.
"time_ratio" is median B / median A, "gate_ratio" the AND gates of B over those of the K + 1 sweeps (predicted for cgd:
about 1 + K / ((K + 1) iters) for the scoring, less the K repeated prefixes B saves), "aa_spread" |A - A| / A of the last two
runs.  beta* is checked to be row l* of the plain sweep on the full system: shares whose folds are all equal make the full
system the fold itself, whatever K (the sweep's lambda enters after the division by d, as the cross-validation's does)."""
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
    ap.add_argument("--alg", default="cgd")
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--precision", type=int, default=56)
    ap.add_argument("--gates-only", action="store_true", help="lower the programs and print the gate figures: needs no GPU")
    a = ap.parse_args()
    w, p, K = a.width, a.precision, a.K
    iters = a.iters if a.alg == "cgd" else 0
    lams = [1e-4 * 4.0 ** l for l in range(a.L)]
    for d in a.d:
        sysm = lgc.make_system(d, w, p, a.alg, iters, 1e-3, 2, 1, 0, 0)
        cv = dict(lambdas=lams, folds=K, reveal_index=True)
        if a.gates_only:
            pa, pb = lgc.Program(sysm, lambdas=lams), lgc.Program(sysm, **cv)
            ga, gb = int(pa.info.total_gates), int(pb.info.total_gates)
            print(json.dumps({"d": d, "K": K, "L": a.L, "width": w, "alg": a.alg, "iters": iters,
                              "and_gates": {"A_one_sweep": ga, "A": (K + 1) * ga, "B": gb}, "gate_ratio": gb / ((K + 1) * ga),
                              "launches": {"A_one_sweep": int(pa.info.n_launches), "B": int(pb.info.n_launches)}}), flush=True)
            continue
        rng = np.random.default_rng(d)
        beta = rng.random(d)
        folds = []
        for _ in range(K):
            rows = 3 * d
            X = rng.standard_normal((rows, d)); X /= np.abs(X).max(axis=0)
            y = X @ beta + 0.1 * rng.standard_normal(rows)
            folds.append(split_shares(rng, *_words(X.T @ X / rows, X.T @ y / rows, d, p), 2, w))
        cv_shares = np.ascontiguousarray(np.hstack(folds))

        def plain_sweeps():
            runs = [_run(sysm, folds[k % K], lambdas=lams) for k in range(K + 1)]
            return sum(r["st"]["seconds_total"] for r in runs), runs[0]["st"]
        t = {"A": [], "B": []}
        for _ in range(2):
            ta, sta = plain_sweeps()
            t["A"].append(ta)
            rb = _run(sysm, cv_shares, **cv)
            t["B"].append(rb["st"]["seconds_total"])
            assert 0 <= rb["index"] < a.L
        aa = [plain_sweeps()[0] for _ in range(2)]
        # K equal folds: every training system and the full system are the fold itself (sums of K equal words divide exactly)
        same = _run(sysm, np.ascontiguousarray(np.hstack([folds[0]] * K)), **cv)
        ref = _run(sysm, folds[0], lambdas=lams)
        assert (ref["beta"][same["index"]] == same["beta"]).all(), "beta* is not row l* of the plain sweep on the full system"
        ga = (K + 1) * sta["and_gates"]
        print(json.dumps({"d": d, "K": K, "L": a.L, "width": w, "alg": a.alg, "iters": iters, "lambdas": lams, "seconds": t, "aa_seconds": aa,
                          "selected": rb["index"],
                          "time_ratio": statistics.median(t["B"]) / statistics.median(t["A"]),
                          "aa_spread": abs(aa[0] - aa[1]) / min(aa),
                          "and_gates": {"A_one_sweep": sta["and_gates"], "A": ga, "B": rb["st"]["and_gates"]},
                          "gate_ratio": rb["st"]["and_gates"] / ga,
                          "gate_ratio_predicted": (1 + K / ((K + 1) * iters)) if iters else None,
                          "launches": {"A_one_sweep": sta["launches"], "B": rb["st"]["launches"]}}), flush=True)


if __name__ == "__main__":
    main()
