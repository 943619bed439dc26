"""Device milliseconds of BOTH parties' OT work for the cross block of one provider pair, r x s columns over n rows, in one process
with device I/O:
A = the matrix calls (include/linreg_gc_ot_matrix.h) in the batches of the host's rule (M <= 2^24 OTs and y <= 256 MiB),
B = the half-payload calls (include/linreg_gc_ot_half.h) on the same operands, in the batches of their rule (the half y <= 256 MiB),
an untimed run of each, then A B A B ..., then A A for the run-to-run spread.  One JSON line:
   python tests/tools/gpu_ot_half.py [--n 10000] [--r 50] [--s 50] [--width 64] [--reps 2]
Times are HIP events on the null stream around the calls of one form (every call ends with a synchronisation of its session's
stream, so the events bracket all of its device work and the small share downloads; not the allocation of the buffers), with the
wall clock beside them.  "time_ratio" is median B / median A.  Both forms run the same AES blocks (3 per OT for the extension, 3
per pad block), so the predicted ratio is 1; only the bytes of y differ, (W / 2 + 1) / W.  "excess_over_3_spreads" is true when B
is slower than A by more than three times the A A spread.  The shares of both forms are recombined and compared in the run."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "linreg-mpc_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import linreg_gc as lgc  # noqa: E402
import ot_half_model  # noqa: E402      (the models state the batch rule of each form)
import ot_matrix_model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--r", type=int, default=50)
    ap.add_argument("--s", type=int, default=50)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--reps", type=int, default=2)
    o = ap.parse_args()
    if lgc.device_count() < 1:
        raise SystemExit("gpu_ot_half.py measures on an MI355X: no HIP device visible")
    n, r, s, w = o.n, o.r, o.s, o.width
    mask = np.uint64((1 << w) - 1)
    L = lgc.lib()
    try:                                                   # the HIP runtime the library already runs on, for the events
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    vp = C.c_void_p
    for f, args in (("lgc_dev_alloc", [C.c_int, C.c_size_t, C.POINTER(vp), vp]), ("lgc_dev_upload", [vp, vp, C.c_size_t]),
                    ("lgc_dev_download", [vp, vp, C.c_size_t])):
        getattr(L, f).argtypes = args; getattr(L, f).restype = C.c_int
    L.lgc_dev_free.argtypes = [vp]; L.lgc_dev_free.restype = None
    hip.hipEventCreate.argtypes = [C.POINTER(vp)]; hip.hipEventRecord.argtypes = [vp, vp]; hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
    e0, e1 = vp(), vp()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

    rng = np.random.default_rng(n + r)
    seeds0 = rng.integers(0, 256, size=(128, 16), dtype=np.uint8); seeds1 = rng.integers(0, 256, size=(128, 16), dtype=np.uint8)
    delta = rng.integers(0, 256, size=16, dtype=np.uint8)
    seeds_s = np.where(np.unpackbits(delta, bitorder="little")[:, None] == 1, seeds1, seeds0)
    xr = rng.integers(0, 1 << 63, (n, r), dtype=np.uint64) & mask
    xs = rng.integers(0, 1 << 63, (n, s), dtype=np.uint64) & mask

    def dev(nbytes, fill=None):
        p = vp()
        assert L.lgc_dev_alloc(0, nbytes, C.byref(p), None) == 0, L.lgc_last_error()
        if fill is not None:
            fill = np.ascontiguousarray(fill)
            assert L.lgc_dev_upload(p, fill.ctypes.data_as(vp), fill.nbytes) == 0
        return p

    def down(p, count):
        out = np.zeros(count, dtype=np.uint64)
        assert L.lgc_dev_download(out.ctypes.data_as(vp), p, out.nbytes) == 0
        return out

    at = lambda p, off: p.value + off
    xr_dev, xs_dev = dev(n * r * 8, xr), dev(n * s * 8, xs)
    sh = dev(r * s * 8)
    forms, bufs, sessions = {}, [xr_dev, xs_dev, sh], []
    for name, half in (("A", False), ("B", True)):
        rows_ = (ot_half_model if half else ot_matrix_model).batch_rows(n, r, s, w)
        y_bytes = L.lgc_ot_gilboa_half_y_bytes if half else L.lgc_ot_gilboa_matrix_y_bytes
        u, y = dev(L.lgc_ot_u_bytes(rows_[0] * r * w)), dev(y_bytes(rows_[0], r, s, w))
        S = lgc.OtSender(delta.tobytes(), seeds_s); R = lgc.OtReceiver(seeds0, seeds1)
        S.set_device_io(True); R.set_device_io(True)
        start, send, finish = ((R.gilboa_half_start_ptr, S.gilboa_half_ptr, R.gilboa_half_finish_ptr) if half else
                               (R.gilboa_matrix_start_ptr, S.gilboa_matrix_ptr, R.gilboa_matrix_finish_ptr))

        def form(rows_=rows_, u=u, y=y, start=start, send=send, finish=finish):
            tot = np.zeros(r * s, dtype=np.uint64)
            k0 = 0
            for rows in rows_:
                start(at(xr_dev, k0 * r * 8), rows, r, s, w, u.value)
                send(at(xs_dev, k0 * s * 8), rows, r, s, w, u.value, y.value, sh.value)
                tot += down(sh, r * s)
                finish(y.value, sh.value)
                tot += down(sh, r * s)
                k0 += rows
            return (tot & mask).reshape(r, s)

        forms[name] = (form, rows_, sum(y_bytes(b, r, s, w) for b in rows_))
        bufs += [u, y]; sessions += [S, R]

    def timed(fn):
        hip.hipEventRecord(e0, None)
        t0 = time.perf_counter()
        fn()
        hip.hipEventRecord(e1, None)
        hip.hipEventSynchronize(e1)
        wall = (time.perf_counter() - t0) * 1e3
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value, wall

    with np.errstate(over="ignore"):
        pa, pb = forms["A"][0](), forms["B"][0]()
        want = (xr.T @ xs) & mask
    shares_agree = bool(np.array_equal(pa, pb) and np.array_equal(pa, want))
    t = {"A": [], "B": []}
    wall = {"A": [], "B": []}
    for _ in range(o.reps):
        for k in ("A", "B"):
            ev, wc = timed(forms[k][0])
            t[k].append(ev); wall[k].append(wc)
    aa = [timed(forms["A"][0])[0] for _ in range(2)]
    ma, mb = statistics.median(t["A"]), statistics.median(t["B"])
    spread = abs(aa[0] - aa[1]) / min(aa)
    ots = n * r * w
    nblk = (s * w + 127) // 128
    print(json.dumps({"n": n, "r": r, "s": s, "width": w, "batches_A": len(forms["A"][1]), "batches_B": len(forms["B"][1]), "ms": t, "wall_ms": wall,
                      "aa_ms": aa, "median_A_matrix_ms": ma, "median_B_half_ms": mb, "time_ratio": mb / ma, "aa_spread": spread,
                      "spread_A": (max(t["A"]) - min(t["A"])) / min(t["A"]), "spread_B": (max(t["B"]) - min(t["B"])) / min(t["B"]),
                      "excess_over_3_spreads": bool(mb / ma - 1 > 3 * spread), "predicted_ratio": 1.0, "aes_blocks": 3 * ots + 3 * ots * nblk,
                      "y_bytes": [forms["A"][2], forms["B"][2]], "shares_agree": shares_agree}), flush=True)
    for x in sessions:
        x.close()
    for p in bufs:
        L.lgc_dev_free(p)
    if not shares_agree:
        raise SystemExit("the shares of the two forms do not recombine to the same block")


if __name__ == "__main__":
    main()
