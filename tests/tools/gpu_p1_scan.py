"""Device milliseconds of the integer block of lgc_p1_local_scan (include/linreg_gc_scan.h), G^T Z mod 2^w for `cand` candidate
columns and nz columns of Z = [own covariates, y]: p1_scan_kernel (B) against p1_rect_kernel as it would serve the same call
(A), on the same data in one process: an untimed run of each, then A B A B ..., then A A for the run-to-run spread.  One JSON line:
   python tests/tools/gpu_p1_scan.py [--n 10000] [--cand 10000] [--nz 11] [--width 64 --precision 56] [--reps 10]
Times are HIP events around the kernel launches alone (lgc_test_p1_scan_block, linreg_gc_debug.h): neither the floating-point
diagonal nor the copies.  The columns are laid out [candidates, covariates] so that Z is a contiguous run of columns, which
p1_rect_kernel needs and p1_scan_kernel does not.  "time_ratio" is median B / median A.  Every word of B is checked against A."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "linreg-mpc_amd", "python"))
import numpy as np  # noqa: E402
import linreg_gc as lgc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--cand", type=int, default=10000)
    ap.add_argument("--nz", type=int, default=11)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--precision", type=int, default=56)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if lgc.device_count() < 1:
        raise SystemExit("gpu_p1_scan.py measures on an MI355X: no HIP device visible")
    n, M, nz, w = a.n, a.cand, a.nz, a.width
    nc = nz - 1
    rng = np.random.default_rng(n + M)
    half = 1 << (w - 1)
    X = rng.integers(-half, half, (n, M + nc), dtype=np.int64)
    y = rng.integers(-half, half, n, dtype=np.int64)
    p1 = lgc.Phase1(X, y, w, a.precision)
    del X
    fn = lgc.lib().lgc_test_p1_scan_block
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double)]

    def run(use_rect):
        out = np.zeros(M * nz, dtype=np.uint64)
        ms = C.c_double()
        rc = fn(p1._h, M, M + nc, 0, M, 1, use_rect, out.ctypes.data_as(C.c_void_p), C.byref(ms))
        if rc:
            raise SystemExit(lgc.lib().lgc_last_error().decode())
        return ms.value, out

    _, ref = run(1)
    _, got = run(0)
    assert np.array_equal(ref, got), "p1_scan_kernel differs from p1_rect_kernel"
    t = {"A": [], "B": []}
    for _ in range(a.reps):
        t["A"].append(run(1)[0])
        t["B"].append(run(0)[0])
    aa = [run(1)[0] for _ in range(2)]
    bytes_g = n * M * 8
    mb = statistics.median(t["B"])
    print(json.dumps({"n": n, "candidates": M, "nz": nz, "width": w, "ms": t, "aa_ms": aa,
                      "median_A_rect_ms": statistics.median(t["A"]), "median_B_scan_ms": mb,
                      "time_ratio": mb / statistics.median(t["A"]), "aa_spread": abs(aa[0] - aa[1]) / min(aa),
                      "scan_read_of_G_TBps": bytes_g / (mb * 1e-3) / 1e12, "bit_identical": True}), flush=True)
    p1.close()


if __name__ == "__main__":
    main()
