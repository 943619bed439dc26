"""The half-payload form of the matrix Gilboa product (include/linreg_gc_ot_half.h, csrc/ot.hip) bit for bit on the MI355X.

Both parties derive their pads from the same rows and tweaks, so a kernel that REUSES a tweak or puts a field into the wrong
place on both sides still gives shares that recombine.  Only the transcript shows it: every comparison is np.array_equal on
the whole of u, the packed y and both share blocks against tests/ot_half_model.py (OpenSSL and numpy).

Every case runs two batches on one session pair, the second a small ragged one: the PRG counter and the tweak cross a
boundary.  The shapes (W, rows, r, s) come from ot.hip's launch geometry (ot_block_geom); each names its constant:
    slot, chunk           a lane owns slot ir * nblk + c of the r * nblk slots, a wave one chunk of 64 slots: nsc = ceil(slots / 64)
    unit, kbu, ks         a unit is the pair of OTs of one (k, ir) that fills the same words: q = 0 is bits (0, W / 2) and writes
                          words 0 and W / 2, 1 <= q < W / 2 is bits (q, W - q) and writes word q.  The kbu = rows * W / 2 units are
                          cut into ks = min(kbu, 16 kOtGroups / nsc) slices; a lane takes one unit per trip (slice, slice + ks, ...)
    kOtGroups = 512       16 * 512 = 8192 waves at the most: with nsc = 1 a second trip starts at kbu > 8192
                          NOT covered: nsc > 8192 (more than 524 288 slots, at least 1.6e7 OTs), where ks = 1 and the launch has more
                          than kOtGroups workgroups: too large for a test
    whole-block stores    when s * W is a multiple of 128 a lane stores / loads its block of a run of y as 16 bytes, else word by word"""
import ctypes as C

import numpy as np
import pytest

import ot_half_model as hm
import ot_matrix_model as om
from test_ot import _setup
from test_ot_edges_gpu import _check_gilboa_mirror, _check_labels_mirror, _full, _label_inputs

pytestmark = pytest.mark.gpu

LGC_ESTATE = -5                                # include/linreg_gc.h
SHAPE2 = {64: (1, 3, 3), 32: (1, 5, 5)}        # second batch: M = 192 / 160 OTs, nblk = 2, a one-word tail
SHAPES = [
    (64, 1, 1, 1),         # one slot, 32 units on 32 waves, and the q = 0 unit's two stores
    (64, 3, 3, 2),         # s * W = 128 exactly: whole-block stores
    (32, 7, 2, 4),         # exact block at W = 32: whole-block stores
    (64, 5, 3, 5),         # nblk = 3, the last block half used: word stores
    (32, 1, 3, 3),         # a 96-bit tail in the only block; kbu = 16: exactly one workgroup
    (32, 9, 5, 9),         # nblk = 3, one word in the tail
    (64, 2, 13, 11),       # 78 slots: no multiple of 64, nsc = 2, the second chunk has 14 live lanes
    (64, 257, 1, 2),       # kOtGroups: nsc = 1, kbu = 8224 > 8192 waves: slices 0..31 take a second trip
    (32, 513, 1, 5),       # the same at W = 32: kbu = 8208, slices 0..15 take a second trip; nblk = 2 with a one-word tail
    (64, 90, 5, 52),       # nsc = 3: ks = 8192 / 3 = 2730, 8190 waves: the last workgroup has two idle waves; kbu = 2880 > ks
    (64, 600, 7, 70),      # nblk = 35, 245 slots: nsc = 4, ks = 2048 of kbu = 19 200: nine full trips and a partial tenth
]


def _run_case(lgc, w, rows, r, s, ones=False):
    """two half batches ((rows, r, s), then SHAPE2[w]) on a fresh session pair; deterministic in the shape"""
    rng = np.random.default_rng(w * 1000003 + rows * 10007 + r * 101 + s)
    seeds0, seeds1, delta, seeds_s = _setup(rng)
    S = lgc.OtSender(delta.tobytes(), seeds_s); R = lgc.OtReceiver(seeds0, seeds1)
    batches, ctr, tw = [], 0, 0
    try:
        for rows_, r_, s_ in ((rows, r, s), SHAPE2[w]):
            xr, xs = _full(rng, (rows_, r_), w), _full(rng, (rows_, s_), w)
            if ones:
                xr[:], xs[:] = om.mask(w), om.mask(w)
            u = R.gilboa_half_start(xr, s_, w)
            y, ss = S.gilboa_half(xs, r_, w, u)
            sr = R.gilboa_half_finish(y)
            batches.append(((xr, xs), (u, y, ss, sr), ctr, tw))
            ctr += (om.ots(rows_, r_, w) + 127) // 128
            tw += om.ots(rows_, r_, w) * om.nblk(s_, w)
    finally:
        S.close(); R.close()
    return (seeds0, seeds1, delta), batches


def _check(keys, w, inputs, got, ctr, tw):
    seeds0, seeds1, delta = keys
    xr, xs = inputs
    u, y, ss, sr = got
    shape = (w,) + xr.shape + xs.shape[1:]
    exp = hm.run(seeds0, seeds1, delta, xr, xs, w, ctr, tw)
    assert y.dtype == exp["y"].dtype and y.shape == exp["y"].shape and y.nbytes == hm.y_bytes(*shape[1:], w), shape
    assert np.array_equal(np.asarray(u, dtype=np.uint8).reshape(-1), exp["u"]), shape
    assert np.array_equal(y, exp["y"]), shape
    assert np.array_equal(ss, exp["share_s"]) and np.array_equal(sr, exp["share_r"]), shape
    with np.errstate(over="ignore"):
        assert np.array_equal((ss + sr) & om.mask(w), om.product(xr, xs, w)), shape


@pytest.mark.parametrize("w,rows,r,s", SHAPES)
def test_half_matches_model(lgc, w, rows, r, s):
    keys, batches = _run_case(lgc, w, rows, r, s)
    for inputs, got, ctr, tw in batches:
        _check(keys, w, inputs, got, ctr, tw)


@pytest.mark.parametrize("w,rows,r,s", [(64, 5, 3, 5), (32, 7, 2, 4)])
def test_all_ones_operands(lgc, w, rows, r, s):
    """Xs all ones and Xr all ones: every field of y' sees its largest correlation and every choice bit is set"""
    keys, batches = _run_case(lgc, w, rows, r, s, ones=True)
    for inputs, got, ctr, tw in batches:
        _check(keys, w, inputs, got, ctr, tw)


def test_receives_of_four_kinds_in_flight(lgc, gccpu):
    """a half batch, a matrix batch, a per-pair Gilboa batch and a label batch started before any is finished: each equals its
    reference at the counter and tweak positions the START order implies (the matrix reference is tests/ot_matrix_model.py, the
    per-pair and label references are tests/test_ot_edges_gpu.py's).  A finish of another kind than the oldest start is refused and
    leaves it in flight, a half finish on a matrix receive as well as a matrix finish on a half receive"""
    rng = np.random.default_rng(778)
    seeds0, seeds1, delta, seeds_s = _setup(rng)
    keys = (seeds0, seeds1, delta)
    w, rows, r, s = 64, 5, 3, 5
    xr, xs = _full(rng, (rows, r), w), _full(rng, (rows, s), w)
    xr1, xs1 = _full(rng, (4, 2), 32), _full(rng, (4, 5), 32)
    a2, b2 = _full(rng, (3, 17), 32), _full(rng, (3, 17), 32)
    lab = _label_inputs(rng, 131)
    S = lgc.OtSender(delta.tobytes(), seeds_s); R = lgc.OtReceiver(seeds0, seeds1)
    L = lgc.lib()
    try:
        u0 = R.gilboa_half_start(xr, s, w)
        u1 = R.gilboa_matrix_start(xr1, 5, 32)
        u2 = R.gilboa_start(a2, 32)
        u3 = R.labels_start(lab[0])
        y0, ss0 = S.gilboa_half(xs, r, w, u0)
        buf = np.zeros(4096, dtype=np.uint64)
        vp = lambda v: v.ctypes.data_as(C.c_void_p)
        assert L.lgc_ot_gilboa_matrix_recv_finish(R._h, vp(buf), vp(buf)) == LGC_ESTATE            # the oldest is a half receive
        assert L.lgc_ot_gilboa_recv_finish(R._h, vp(buf), vp(buf)) == LGC_ESTATE
        assert L.lgc_ot_labels_recv_finish(R._h, vp(buf), vp(buf)) == LGC_ESTATE
        with pytest.raises(lgc.LgcError):
            R.gilboa_matrix_finish(y0)                                                              # (the binding keeps its own queue too)
        sr0 = R.gilboa_half_finish(y0)
        assert L.lgc_ot_gilboa_half_recv_finish(R._h, vp(buf), vp(buf)) == LGC_ESTATE              # now the oldest is a matrix one
        y1, ss1 = S.gilboa_matrix(xs1, 2, 32, u1); sr1 = R.gilboa_matrix_finish(y1)
        assert L.lgc_ot_gilboa_half_recv_finish(R._h, vp(buf), vp(buf)) == LGC_ESTATE              # a per-pair one
        y2, ss2 = S.gilboa(b2, 32, u2); sr2 = R.gilboa_finish(y2)
        e3 = S.labels(lab[1], lab[2], u3); out3 = R.labels_finish(e3)
        with pytest.raises(lgc.LgcError):                                                           # nothing in flight any more
            R.gilboa_half_finish(y0)
    finally:
        S.close(); R.close()
    m0, m1, m2 = om.ots(rows, r, w), om.ots(4, 2, 32), 3 * 17 * 32
    ctr1 = (m0 + 127) // 128; ctr2 = ctr1 + (m1 + 127) // 128; ctr3 = ctr2 + (m2 + 127) // 128
    tw1 = m0 * om.nblk(s, w); tw2 = tw1 + m1 * om.nblk(5, 32); tw3 = tw2 + m2
    _check(keys, w, (xr, xs), (u0, y0, ss0, sr0), 0, 0)
    exp = om.run(seeds0, seeds1, delta, xr1, xs1, 32, ctr1, tw1)
    assert np.array_equal(np.asarray(u1, dtype=np.uint8).reshape(-1), exp["u"]) and np.array_equal(y1, exp["y"])
    assert np.array_equal(ss1, exp["share_s"]) and np.array_equal(sr1, exp["share_r"])
    _check_gilboa_mirror(gccpu, keys, 32, (a2, b2), (u2, y2, ss2, sr2), ctr2, tw2)
    _check_labels_mirror(gccpu, keys, lab, (u3, e3, out3), ctr3, tw3)


def test_device_io_matches_host_io(lgc):
    """lgc_ot_*_set_device_io: operands, u, y and the shares in device memory (torch tensors) give the bytes of a host-I/O session
    with the same seeds, over a word-store shape, two whole-block shapes and a second-trip one on one session pair each way; the two
    whole-block shapes once more with y 8 and 4 bytes off a 16-byte boundary, where the library must fall back to word stores and
    loads.  At width 32 only the low 32 bits of a device-resident share word are defined."""
    import torch
    rng = np.random.default_rng(557)
    seeds0, seeds1, delta, seeds_s = _setup(rng)
    L = lgc.lib()
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.int64)).cuda()
    host = lambda t, dt: t.cpu().numpy().view(dt)
    Sh = lgc.OtSender(delta.tobytes(), seeds_s); Rh = lgc.OtReceiver(seeds0, seeds1)
    Sd = lgc.OtSender(delta.tobytes(), seeds_s); Rd = lgc.OtReceiver(seeds0, seeds1)
    try:
        Sd.set_device_io(True); Rd.set_device_io(True)
        for w, rows, r, s, off in ((64, 5, 3, 5, 0), (32, 7, 2, 4, 0), (64, 3, 3, 2, 0), (32, 513, 1, 5, 0), (64, 3, 3, 2, 8), (32, 7, 2, 4, 4)):
            xr, xs = _full(rng, (rows, r), w), _full(rng, (rows, s), w)
            m = om.ots(rows, r, w)
            u = Rh.gilboa_half_start(xr, s, w)
            y, ss = Sh.gilboa_half(xs, r, w, u)
            sr = Rh.gilboa_half_finish(y)
            dxr, dxs = dev(xr), dev(xs)
            yb = L.lgc_ot_gilboa_half_y_bytes(rows, r, s, w)
            assert yb == y.nbytes == hm.y_bytes(rows, r, s, w)
            du = torch.empty(L.lgc_ot_u_bytes(m), dtype=torch.uint8, device="cuda"); dy = torch.empty(yb + 16, dtype=torch.uint8, device="cuda")
            assert dy.data_ptr() % 16 == 0
            dy = dy[off:off + yb]
            dss = torch.zeros(r * s, dtype=torch.int64, device="cuda"); dsr = torch.zeros(r * s, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            Rd.gilboa_half_start_ptr(dxr.data_ptr(), rows, r, s, w, du.data_ptr())
            Sd.gilboa_half_ptr(dxs.data_ptr(), rows, r, s, w, du.data_ptr(), dy.data_ptr(), dss.data_ptr())
            Rd.gilboa_half_finish_ptr(dy.data_ptr(), dsr.data_ptr())
            torch.cuda.synchronize()
            gss, gsr = host(dss, np.uint64).reshape(r, s) & om.mask(w), host(dsr, np.uint64).reshape(r, s) & om.mask(w)
            assert np.array_equal(host(du, np.uint8), u), (w, rows, r, s)
            assert np.array_equal(host(dy, y.dtype).reshape(y.shape), y), (w, rows, r, s)
            assert np.array_equal(gss, ss) and np.array_equal(gsr, sr), (w, rows, r, s)
            with np.errstate(over="ignore"):
                assert np.array_equal((gss + gsr) & om.mask(w), om.product(xr, xs, w))
    finally:
        for x in (Sh, Rh, Sd, Rd):
            x.close()
