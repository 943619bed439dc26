"""Device milliseconds of BOTH parties' OT work for the cross block of one provider pair, r x s column pairs over n rows, in one
process with device I/O:
A = the per-pair calls (lgc_ot_gilboa_recv_start / _send / _recv_finish) over the r s pairs, in their batches of 2^24 OTs,
B = the matrix calls (include/linreg_gc_ot_matrix.h) on the same operands, in the batches of the host's rule (M <= 2^24 OTs and
    y <= 256 MiB),
an untimed run of each, then A B A B ..., then A A for the run-to-run spread.  One JSON line:
   python tests/tools/gpu_ot_matrix.py [--n 10000] [--r 50] [--s 50] [--width 64] [--reps 2]
Times are HIP events on the null stream around the calls of one form (every call ends with a synchronisation of its session's
stream, so the events bracket all of its device work and the small share downloads; not the allocation of the buffers), with the
wall clock beside them.  "time_ratio" is median B / median A; "predicted_ratio" counts AES blocks per product bit from the kernels:
6 in form A (per OT two column-PRG blocks on the receiver and one on the sender, two hashes on the sender and one on the receiver),
in form B 3 / s for the extension and 3 nblk / s for the pads: (1.5 + 3 / s) / 6 at W = 64 and even s, (0.75 + 3 / s) / 6 at W = 32
and s a multiple of 4.  The shares of both forms are recombined
and compared in the run."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "linreg-mpc_amd", "python"))
import numpy as np  # noqa: E402
import linreg_gc as lgc  # noqa: E402


def batch_rows(n, r, s, w):
    per = max(min((1 << 24) // (r * w), (256 << 20) // (r * w * s * (w // 8))), 1)
    return [min(per, n - k) for k in range(0, n, per)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--r", type=int, default=50)
    ap.add_argument("--s", type=int, default=50)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--reps", type=int, default=2)
    o = ap.parse_args()
    if lgc.device_count() < 1:
        raise SystemExit("gpu_ot_matrix.py measures on an MI355X: no HIP device visible")
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
    # A: pair q = ir * s + j holds column ir of the receiver and column j of the sender, pair-major, n words each
    npairs = r * s
    per = max(min((1 << 24) // (n * w), npairs), 1)
    a_dev = dev(npairs * n * 8, np.repeat(xr.T, s, axis=0)); b_dev = dev(npairs * n * 8, np.tile(xs.T, (r, 1)))
    u_a = dev(L.lgc_ot_u_bytes(per * n * w)); y_a = dev(per * n * w * 8); sh_a = dev(per * 8)
    Sa = lgc.OtSender(delta.tobytes(), seeds_s); Ra = lgc.OtReceiver(seeds0, seeds1)
    Sa.set_device_io(True); Ra.set_device_io(True)

    def form_a():
        ss, sr = np.zeros(npairs, dtype=np.uint64), np.zeros(npairs, dtype=np.uint64)
        for q0 in range(0, npairs, per):
            nb = min(per, npairs - q0)
            Ra.gilboa_start_ptr(at(a_dev, q0 * n * 8), nb, n, w, u_a.value)
            Sa.gilboa_ptr(at(b_dev, q0 * n * 8), nb, n, w, u_a.value, y_a.value, sh_a.value)
            ss[q0:q0 + nb] = down(sh_a, nb)
            Ra.gilboa_finish_ptr(y_a.value, sh_a.value)
            sr[q0:q0 + nb] = down(sh_a, nb)
        return ((ss + sr) & mask).reshape(r, s)

    # B: whole rows per batch
    rows_b = batch_rows(n, r, s, w)
    xr_dev, xs_dev = dev(n * r * 8, xr), dev(n * s * 8, xs)
    u_b = dev(L.lgc_ot_u_bytes(rows_b[0] * r * w)); y_b = dev(L.lgc_ot_gilboa_matrix_y_bytes(rows_b[0], r, s, w)); sh_b = dev(r * s * 8)
    Sb = lgc.OtSender(delta.tobytes(), seeds_s); Rb = lgc.OtReceiver(seeds0, seeds1)
    Sb.set_device_io(True); Rb.set_device_io(True)

    def form_b():
        tot = np.zeros(r * s, dtype=np.uint64)
        k0 = 0
        for rows in rows_b:
            Rb.gilboa_matrix_start_ptr(at(xr_dev, k0 * r * 8), rows, r, s, w, u_b.value)
            Sb.gilboa_matrix_ptr(at(xs_dev, k0 * s * 8), rows, r, s, w, u_b.value, y_b.value, sh_b.value)
            tot += down(sh_b, r * s)
            Rb.gilboa_matrix_finish_ptr(y_b.value, sh_b.value)
            tot += down(sh_b, r * s)
            k0 += rows
        return (tot & mask).reshape(r, s)

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
        pa, pb = form_a(), form_b()
        want = (xr.T @ xs) & mask
    shares_agree = bool(np.array_equal(pa, pb) and np.array_equal(pa, want))
    t = {"A": [], "B": []}
    wall = {"A": [], "B": []}
    for _ in range(o.reps):
        for k, fn in (("A", form_a), ("B", form_b)):
            ev, wc = timed(fn)
            t[k].append(ev); wall[k].append(wc)
    aa = [timed(form_a)[0] for _ in range(2)]
    ma, mb = statistics.median(t["A"]), statistics.median(t["B"])
    ots_a, ots_b = n * r * s * w, n * r * w
    nblk = (s * w + 127) // 128
    blocks_a, blocks_b = 6 * ots_a, 3 * ots_b + 3 * ots_b * nblk                 # AES blocks: extension 2 + 1 per OT; hashes 2 + 1 per OT (A), per block (B)
    print(json.dumps({"n": n, "r": r, "s": s, "width": w, "batches_A": -(-npairs // per), "batches_B": len(rows_b), "ms": t, "wall_ms": wall,
                      "aa_ms": aa, "median_A_per_pair_ms": ma, "median_B_matrix_ms": mb, "time_ratio": mb / ma,
                      "aa_spread": abs(aa[0] - aa[1]) / min(aa), "predicted_ratio": blocks_b / blocks_a, "aes_blocks": [blocks_a, blocks_b],
                      "wire_bytes": [24 * ots_a, 16 * ots_b + ots_b * s * w // 8], "shares_agree": shares_agree}), flush=True)
    for x in (Sa, Ra, Sb, Rb):
        x.close()
    for p in (a_dev, b_dev, u_a, y_a, sh_a, xr_dev, xs_dev, u_b, y_b, sh_b):
        L.lgc_dev_free(p)
    if not shares_agree:
        raise SystemExit("the shares of the two forms do not recombine to the same block")


if __name__ == "__main__":
    main()
