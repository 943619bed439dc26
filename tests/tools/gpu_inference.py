"""Device seconds of the Cholesky solve with standard errors, residual variance and R^2 (B, lgc_solver_create_inference with
LGC_INFER_SE | LGC_INFER_FIT) against the plain Cholesky solve of the same system (A, lgc_solver_create), in one process:
A B A B, then A A for the run-to-run spread.  One JSON line per dimension:
   python tests/tools/gpu_inference.py [--d 100 500] [--width 64 --precision 56]
   python tests/tools/gpu_inference.py --gates-only --d 100 500      # lowers the programs and prints the cost figures: no GPU
Times are stats()["seconds_total"] (input labels + garble + evaluate + decode).  "time_ratio" is median B / median A,
"gate_ratio" the lowered AND gates of B over A's (about 2: the d^3 / 6 products and d^2 / 2 divisions of the factorisation are
each doubled by the inverse columns), "aa_spread" |A - A| / A of the last two runs.  B's beta is checked against A's, word for
word.  No pass / fail threshold: the figures go to DESIGN.md 2.8."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "linreg-mpc_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import linreg_gc as lgc  # noqa: E402

LAM = 1e-3


def _shares(rng, d, w, p):
    """two shares [A, b, yy] of a studentised system on the two-party path (lambda on the diagonal), n = 2 d + 60 rows"""
    n = 2 * d + 60
    X = rng.standard_normal((n, d)); X = (X - X.mean(axis=0)) / X.std(axis=0)
    y = X @ (rng.random(d) / np.sqrt(d)) + 0.4 * rng.standard_normal(n); y = (y - y.mean()) / y.std()
    G, b, yy = X.T @ X / n, X.T @ y / n, float(y @ y) / n
    m = (1 << w) - 1
    tot = np.array([int((G[i, j] + (LAM if i == j else 0.0)) * 2.0 ** p) & m for i in range(d) for j in range(i + 1)] +
                   [int(v * 2.0 ** p) & m for v in b] + [int(yy * 2.0 ** p) & m], dtype=np.uint64)
    sh = rng.integers(0, 2 ** 63, size=(2, tot.size), dtype=np.uint64) & np.uint64(m)
    with np.errstate(over="ignore"):
        sh[0] = (tot - sh[1]) & np.uint64(m)
    return sh, n


def _run(sysm, shares, **kw):
    s = lgc.Solver(sysm, seed=bytes(range(16)), **kw)
    s.set_shares(shares)
    s.run()
    out = dict(st=s.stats(), beta=s.beta().tolist())
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, nargs="+", default=[100])
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--precision", type=int, default=56)
    ap.add_argument("--gates-only", action="store_true", help="lower the programs and print the cost figures: needs no GPU")
    a = ap.parse_args()
    w, p = a.width, a.precision
    for d in a.d:
        sysm = lgc.make_system(d, w, p, "cholesky", 0, LAM, 2, 0, 0, 0)
        if a.gates_only:
            progs = {"plain": lgc.Program(sysm), "fit": lgc.Program(sysm, inference=("fit",), resid_scale=1.25),
                     "se_fit": lgc.Program(sysm, inference=("se", "fit"), resid_scale=1.25)}
            g = {k: int(q.info.total_gates) for k, q in progs.items()}
            print(json.dumps({"d": d, "width": w, "and_gates": g, "launches": {k: int(q.info.n_launches) for k, q in progs.items()},
                              "gate_ratio": {"fit": g["fit"] / g["plain"], "se_fit": g["se_fit"] / g["plain"]}}), flush=True)
            continue
        rng = np.random.default_rng(d)
        shares, n = _shares(rng, d, w, p)
        plain = np.ascontiguousarray(shares[:, :-1])
        inf = dict(inference=("se", "fit"), resid_scale=n / (n - d))
        t = {"A": [], "B": []}
        for _ in range(2):
            ra = _run(sysm, plain)
            t["A"].append(ra["st"]["seconds_total"])
            rb = _run(sysm, shares, **inf)
            t["B"].append(rb["st"]["seconds_total"])
            assert rb["beta"] == ra["beta"], "beta of the inference program is not the plain solve's"
        aa = [_run(sysm, plain)["st"]["seconds_total"] for _ in range(2)]
        print(json.dumps({"d": d, "width": w, "seconds": t, "aa_seconds": aa,
                          "time_ratio": statistics.median(t["B"]) / statistics.median(t["A"]),
                          "aa_spread": abs(aa[0] - aa[1]) / min(aa),
                          "and_gates": {"A": ra["st"]["and_gates"], "B": rb["st"]["and_gates"]},
                          "gate_ratio": rb["st"]["and_gates"] / ra["st"]["and_gates"],
                          "launches": {"A": ra["st"]["launches"], "B": rb["st"]["launches"]}}), flush=True)


if __name__ == "__main__":
    main()
