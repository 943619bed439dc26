"""Device seconds of one solve with k = 1 and with k = K targets (include/linreg_gc_targets.h), one JSON line:
   python tests/tools/gpu_targets.py --d 500 --alg cholesky --k 8 [--iters 15] [--width 64 --precision 56]
Both solves run on the same A; target 0 of the K-target solve is b of the single one, and its beta must agree bit for bit
("target0_equal").  Times are stats()["seconds_total"] (input labels + garble + evaluate + decode) of one run each."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "linreg-mpc_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import linreg_gc as lgc  # noqa: E402
import orc  # noqa: E402
from helpers import split_shares  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=500)
    ap.add_argument("--alg", default="cholesky", choices=["cholesky", "ldlt", "cgd"])
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--precision", type=int, default=56)
    a = ap.parse_args()
    d, w, p, K = a.d, a.width, a.precision, a.k
    oracle = orc.load()
    rng = np.random.default_rng(d + K)
    n = 3 * d
    X = rng.standard_normal((n, d)); X /= np.abs(X).max(axis=0)
    Xq = oracle.quantize(X, p, n, w)
    bs = []
    for t in range(K):
        y = X @ rng.random(d) + 0.1 * rng.standard_normal(n)
        A, b = oracle.aggregate(Xq, oracle.quantize(y, p, n, w), n, d, p, w)
        bs.append(b)
    iters = a.iters if a.alg == "cgd" else 0
    sysm = lgc.make_system(d, w, p, a.alg, iters, 1e-3, 2, 1, 0, 0)
    out = {"d": d, "alg": a.alg, "width": w, "iters": iters, "k": K}
    betas = {}
    for k in (1, K):
        t0 = time.time()
        s = lgc.Solver(sysm, seed=bytes(range(16)), targets=k)
        s.set_shares(split_shares(rng, A, np.concatenate(bs[:k]), 2, w))
        t1 = time.time()
        s.run()
        st = s.stats()
        betas[k] = s.beta()
        s.close()
        out["k%d" % k] = {"seconds": st["seconds_total"], "and_gates": st["and_gates"], "launches": st["launches"],
                          "create_s": round(t1 - t0, 3)}
    out["ratio"] = out["k%d" % K]["seconds"] / out["k1"]["seconds"]
    out["target0_equal"] = betas[1][0].tolist() == betas[K][0].tolist()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
