"""Wall seconds of a data provider's local block for K row folds: one lgc_p1_local_folds call (B) against K lgc_p1_local calls
behind lgc_p1_set_rows (A), in one process: A B A B ..., then A A for the run-to-run spread.  One JSON line:
   python tests/tools/gpu_p1_folds.py [--n 50000] [--own 500] [--K 5] [--width 64 --precision 56] [--reps 40]
Both calls end with their device-to-host copies, so the host clock around them covers the kernels (Gram, diagonal) and the
copies.  The data is on the device before the first timed call, and each form runs once untimed first.  "time_ratio" is median
B / median A, "aa_spread" |A - A| / A of the last two A runs.  Every word of B is checked against A."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "linreg-mpc_amd", "python"))
import numpy as np  # noqa: E402
import linreg_gc as lgc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--own", type=int, default=500)
    ap.add_argument("--K", type=int, default=5)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--precision", type=int, default=56)
    ap.add_argument("--reps", type=int, default=40)
    a = ap.parse_args()
    if lgc.device_count() < 1:
        raise SystemExit("gpu_p1_folds.py measures on an MI355X: no HIP device visible")
    n, own, K, w = a.n, a.own, a.K, a.width
    rng = np.random.default_rng(n + own)
    half = 1 << (w - 1)
    X = rng.integers(-half, half, (n, own), dtype=np.int64)
    y = rng.integers(-half, half, n, dtype=np.int64)
    p1 = lgc.Phase1(X, y, w, a.precision)
    rows = [lgc.fold_rows(n, K, k) for k in range(K)]

    def windowed():
        t0 = time.perf_counter()
        out = []
        for r0, r1 in rows:
            p1.set_rows(r0, r1)
            out.append(p1.local(0, own, with_y=True))
        p1.set_rows(0, n)
        return time.perf_counter() - t0, out

    def one_pass():
        t0 = time.perf_counter()
        out = p1.local_folds(0, own, K, with_y=True)
        return time.perf_counter() - t0, out

    _, ref = windowed()
    _, got = one_pass()
    for k in range(K):
        assert np.array_equal(got[0][k], ref[k][0]) and np.array_equal(got[1][k], ref[k][1]), "fold %d differs" % k
    t = {"A": [], "B": []}
    for _ in range(a.reps):
        t["A"].append(windowed()[0])
        t["B"].append(one_pass()[0])
    aa = [windowed()[0] for _ in range(2)]
    print(json.dumps({"n": n, "own": own, "K": K, "width": w, "seconds": t, "aa_seconds": aa,
                      "median_A_windowed": statistics.median(t["A"]), "median_B_one_pass": statistics.median(t["B"]),
                      "time_ratio": statistics.median(t["B"]) / statistics.median(t["A"]),
                      "aa_spread": abs(aa[0] - aa[1]) / min(aa), "bit_identical": True}), flush=True)
    p1.close()


if __name__ == "__main__":
    main()
