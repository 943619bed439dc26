"""Device seconds of one co-located association scan (B, lgc_solver_create_scan with LGC_SCAN_SE: c covariates, M candidates)
set against M times the plain Cholesky solve of one augmented system of size D = c + 1 (A, lgc_solver_create), in one process:
A B A B, then A A for the run-to-run spread.  One JSON line:
   python tests/tools/gpu_scan.py [--c 10] [--M 10000] [--width 64 --precision 56]
   python tests/tools/gpu_scan.py --gates-only --c 1 2 5 10 20      # the lowered AND gates per candidate: no GPU
Times are stats()["seconds_total"] (input labels + garble + evaluate + decode).  "speedup" is M x median A / median B.  Three
coefficients of B are checked against A's last coefficient on the augmented system, word for word.  --gates-only prints, per
c, the AND gates one more candidate adds (the difference of two programs, divided by the difference of their M) with and
without the standard errors.  No pass / fail threshold: the figures go to DESIGN.md 2.9."""
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


def _words(rng, c, M, w, p):
    """the share sum of a studentised scan system on the data-provider path (diagonals divided by D), n = 4 D + 40 rows"""
    D, n = c + 1, 4 * (c + 1) + 40
    X = rng.standard_normal((n, c + M)); X = (X - X.mean(axis=0)) / X.std(axis=0)
    y = X[:, :c] @ (rng.random(c) / np.sqrt(c)) + 0.05 * X[:, c:c + 8].sum(axis=1) + 0.4 * rng.standard_normal(n); y = (y - y.mean()) / y.std()
    m = (1 << w) - 1
    q = lambda v: int(v * 2.0 ** p) & m
    Gc, H, b, gy, yy = X[:, :c].T @ X[:, :c] / n, X[:, c:].T @ X[:, :c] / n, X[:, :c].T @ y / n, X[:, c:].T @ y / n, float(y @ y) / n
    gg = (X[:, c:] ** 2).sum(axis=0) / n
    vals = [Gc[i, j] / D if i == j else Gc[i, j] for i in range(c) for j in range(i + 1)] + list(b) + [yy] + list(H.ravel()) + list(gg / D) + list(gy)
    return np.array([q(v) for v in vals], dtype=np.uint64), n


def _split(rng, tot, w):
    m = np.uint64((1 << w) - 1)
    sh = rng.integers(0, 2 ** 63, size=(2, tot.size), dtype=np.uint64) & m
    with np.errstate(over="ignore"):
        sh[0] = (tot - sh[1]) & m
    return sh


def _run(sysm, shares, **kw):
    s = lgc.Solver(sysm, seed=bytes(range(16)), **kw)
    s.set_shares(shares)
    s.run()
    out = dict(st=s.stats(), beta=s.beta().tolist())
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c", type=int, nargs="+", default=[10])
    ap.add_argument("--M", type=int, default=10000)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--precision", type=int, default=56)
    ap.add_argument("--gates-only", action="store_true", help="lower the programs and print the cost per candidate: needs no GPU")
    a = ap.parse_args()
    w, p, M = a.width, a.precision, a.M
    import scan_model as sm
    for c in a.c:
        sysm = lgc.make_system(c + 1, w, p, "cholesky", 0, LAM, 2, 1, 0, 0)
        if a.gates_only:
            out = {"c": c, "width": w, "plain_D_solve_and_gates": int(lgc.Program(sysm).info.total_gates)}
            for se in (False, True):
                g = [int(lgc.Program(sysm, scan=m, scan_se=se, resid_scale=1.25 if se else None).info.total_gates) for m in (M, 2 * M)]
                out["and_gates_per_candidate_se%d" % se] = (g[1] - g[0]) / M
                out["and_gates_M%d_se%d" % (M, se)] = g[0]
            print(json.dumps(out), flush=True)
            continue
        rng = np.random.default_rng(c)
        tot, n = _words(rng, c, M, w, p)
        shares = _split(rng, tot, w)
        pick = (0, M // 2, M - 1)
        aug = [_split(rng, sm.augmented_words(tot, c, M, m)[:-1], w) for m in pick]
        kw = dict(scan=M, scan_se=True, resid_scale=n / (n - c - 1))
        t = {"A": [], "B": []}
        for k in range(2):
            ra = _run(sysm, aug[k])
            t["A"].append(ra["st"]["seconds_total"])
            rb = _run(sysm, shares, **kw)
            t["B"].append(rb["st"]["seconds_total"])
            assert rb["beta"][pick[k]] == ra["beta"][c], "a scan coefficient is not the plain solve's"
        ra2 = _run(sysm, aug[2])
        assert rb["beta"][pick[2]] == ra2["beta"][c]
        aa = [ra2["st"]["seconds_total"], _run(sysm, aug[2])["st"]["seconds_total"]]
        ma, mb = statistics.median(t["A"]), statistics.median(t["B"])
        print(json.dumps({"c": c, "M": M, "width": w, "seconds": t, "aa_seconds": aa, "speedup_M_plain_over_scan": M * ma / mb,
                          "aa_spread": abs(aa[0] - aa[1]) / min(aa),
                          "and_gates": {"A": ra["st"]["and_gates"], "B": rb["st"]["and_gates"]},
                          "gate_ratio_M_plain_over_scan": M * ra["st"]["and_gates"] / rb["st"]["and_gates"],
                          "launches": {"A": ra["st"]["launches"], "B": rb["st"]["launches"]}}), flush=True)


if __name__ == "__main__":
    main()
