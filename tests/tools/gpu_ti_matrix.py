"""Device milliseconds of one provider's work for the cross block with ONE peer, a x b column pairs over n rows, with device I/O:
A = the per-pair protocol's calls for those a b pairs (lgc_p1_mask, lgc_p1_ti_a_batch, lgc_p1_dot, in batches of --batch pairs),
B = the matrix-triple mode's (lgc_p1_matrix_mask and one lgc_p1_matrix_share_b), on the same data in one process: an untimed run
of each, then A B A B ..., then A A for the run-to-run spread.  One JSON line:
   python tests/tools/gpu_ti_matrix.py [--n 50000] [--a 100] [--b 100] [--width 64 --precision 56] [--reps 2] [--batch 1000]
Times are HIP events on the null stream (the stream of these calls) around the calls of one form: the kernels, the small copies
of column lists and sums, and the gaps between them; not the allocation of the buffers.  "time_ratio" is median B / median A."""
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
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--a", type=int, default=100)
    ap.add_argument("--b", type=int, default=100)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--precision", type=int, default=56)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1000)
    o = ap.parse_args()
    if lgc.device_count() < 1:
        raise SystemExit("gpu_ti_matrix.py measures on an MI355X: no HIP device visible")
    n, a, b, w = o.n, o.a, o.b, o.width
    wb = w // 8
    L = lgc.lib()
    try:                                                   # the HIP runtime the library already runs on, for the events
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    vp = C.c_void_p
    for f, args in (("lgc_dev_alloc", [C.c_int, C.c_size_t, C.POINTER(vp), vp]), ("lgc_dev_upload", [vp, vp, C.c_size_t])):
        getattr(L, f).argtypes = args; getattr(L, f).restype = C.c_int
    L.lgc_dev_free.argtypes = [vp]; L.lgc_dev_free.restype = None
    hip.hipEventCreate.argtypes = [C.POINTER(vp)]; hip.hipEventRecord.argtypes = [vp, vp]; hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
    e0, e1 = vp(), vp()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

    rng = np.random.default_rng(n + a)
    half = 1 << (w - 1)
    X = rng.integers(-half, half, (n, a + b), dtype=np.int64)
    ph = lgc.Phase1(X, None, w, o.precision)
    del X
    ph.set_device_io(True)

    def dev(nbytes, fill=None):
        p = vp()
        assert L.lgc_dev_alloc(0, nbytes, C.byref(p), None) == 0, L.lgc_last_error()
        if fill is not None:
            assert L.lgc_dev_upload(p, fill.ctypes.data_as(vp), fill.nbytes) == 0
        return p

    # A: the pairs (i, j), i among the a own columns, j among the peer's b, in batches; the vectors of a batch are random words
    B_ = min(o.batch, a * b)
    V = dev(B_ * n * 8, rng.integers(0, 1 << 63, B_ * n, dtype=np.uint64))
    In = dev(B_ * n * 8, rng.integers(0, 1 << 63, B_ * n, dtype=np.uint64))
    Out = dev(B_ * n * 8)
    pair_cols = np.repeat(np.arange(b, a + b, dtype=np.uint32), b)            # the own column of every pair
    sub = np.zeros(B_, dtype=np.uint64)
    shares = np.zeros(B_, dtype=np.uint64)
    cp = lambda arr: arr.ctypes.data_as(vp)

    def form_a():
        for q0 in range(0, a * b, B_):
            nb = min(B_, a * b - q0)
            cols = np.ascontiguousarray(pair_cols[q0:q0 + nb])
            assert L.lgc_p1_mask(ph._h, cp(cols), nb, V, 1, Out) == 0                              # as party b: b + x
            assert L.lgc_p1_ti_a_batch(ph._h, cp(cols), nb, V, In, cp(sub), Out, cp(shares)) == 0  # as party a: a - y and the share
            assert L.lgc_p1_dot(ph._h, In, None, cp(cols), nb, cp(sub), cp(shares)) == 0           # as party b: <a - y, b> - r

    # B: this provider is B of the instance (it reads X for its share); E comes from the peer, T from the initializer
    seed = bytes(range(16))
    cols_b = np.arange(0, b, dtype=np.uint32)
    E = dev(n * a * wb, rng.integers(0, 1 << 31, n * a * (wb // 4), dtype=np.uint32))
    F = dev(n * b * wb)
    T = np.zeros((a, b), dtype=np.uint32 if w == 32 else np.uint64)

    def form_b():
        ph.matrix_mask(cols_b, seed, out_ptr=F.value)
        return ph.matrix_share_b(cols_b, E.value, a, T)

    def timed(fn):
        hip.hipEventRecord(e0, None)
        fn()
        hip.hipEventRecord(e1, None)
        hip.hipEventSynchronize(e1)
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value

    form_a(); form_b()
    t = {"A": [], "B": []}
    for _ in range(o.reps):
        t["A"].append(timed(form_a))
        t["B"].append(timed(form_b))
    aa = [timed(form_a) for _ in range(2)]
    ma, mb = statistics.median(t["A"]), statistics.median(t["B"])
    print(json.dumps({"n": n, "a": a, "b": b, "width": w, "pairs": a * b, "batch": B_, "ms": t, "aa_ms": aa, "median_A_per_pair_ms": ma,
                      "median_B_matrix_ms": mb, "time_ratio": mb / ma, "aa_spread": abs(aa[0] - aa[1]) / min(aa)}), flush=True)
    for p in (V, In, Out, E, F):
        L.lgc_dev_free(p)
    ph.close()


if __name__ == "__main__":
    main()
