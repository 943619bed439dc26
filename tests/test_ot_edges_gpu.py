"""The IKNP OT extension (csrc/ot.hip) bit for bit at every loop and grid edge of its kernels.

Both parties derive their masks from the same AES-128-CTR columns and the same tweaked hashes, so a kernel that REUSES a
counter block or a tweak (the second block of a two-per-trip loop, a second grid-stride trip, a batch resumed at the wrong
stream position) still produces shares that recombine and labels that arrive: no functional check can see it.  Only the
transcript can: every comparison here is np.array_equal on the whole of u, e / y, out and both share vectors, against the
CPU mirror (oracle/gc_cpu.cpp through gccpu) always and, on one large case per kernel family (marked +openssl), against
the OpenSSL / numpy restatement of helpers.py as well, so that the product's own key schedule is not the only witness.
tests/test_keystream_refs_cpu.py shows that the two references agree with each other.

Every case runs two batches on one session pair (the second a small ragged one): ctr and tweak advance across the
boundary.  The shapes come from ot.hip's launch geometry; each names its constant, so a change there shows what to move:
    kOtGroups = 512       workgroups of a payload launch: labels gx <= 512, Gilboa gy = min(npairs, 512), gx <= 512 / gy
    2048 items            per workgroup: gx = ceil(items / 2048); a workgroup is 1024 lanes x two items per trip
    cols cap 4            ot_cols_kernel: gx = clamp(ceil(m128 / 2048), 1, 4) workgroups per column, two blocks per trip
    512-OT group          ot_transpose_kernel: one wave per 512 OTs, 16-byte loads guarded by first + t + 1 < w64 = 2 m128"""
import ctypes as C

import numpy as np
import pytest

from helpers import iknp_gilboa_restatement, iknp_labels_restatement, iknp_restatement
from test_ot import _ip, _setup

pytestmark = pytest.mark.gpu

LABEL_M2 = 131                         # second batch of a label case: ragged (one block of 128 and 3 OTs)
GILBOA_SHAPE2 = {64: (1, 3), 32: (2, 5)}   # second batch of a Gilboa case: 192 / 320 OTs, one and a half / two and a half blocks


def _full(rng, shape, w):
    v = rng.integers(0, 2 ** 63, size=shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=shape, dtype=np.uint64)
    return v & np.uint64((1 << w) - 1)


def _cbits(a, w):
    return a.view(np.uint8) if w == 64 else a.astype(np.uint32).view(np.uint8)


def _label_inputs(rng, m):
    choice = rng.integers(0, 2, size=m, dtype=np.uint8)
    return choice, rng.integers(0, 256, size=(m, 16), dtype=np.uint8), rng.integers(0, 256, size=(m, 16), dtype=np.uint8)


def _run_label_case(lgc, m):
    """two label batches (m, then LABEL_M2) on a fresh session pair; deterministic in m.
    Returns the keys and, per batch, (inputs, transcript, ctr0, tweak0)."""
    rng = np.random.default_rng(1000 + m)
    seeds0, seeds1, delta, seeds_s = _setup(rng)
    S = lgc.OtSender(delta.tobytes(), seeds_s); R = lgc.OtReceiver(seeds0, seeds1)
    batches, ctr, tw = [], 0, 0
    try:
        for mm in (m, LABEL_M2):
            choice, m0, m1 = _label_inputs(rng, mm)
            u = R.labels_start(choice)
            e = S.labels(m0, m1, u)
            out = R.labels_finish(e)
            assert np.array_equal(out, np.where(choice[:, None] == 1, m1, m0)), mm      # the chosen labels are delivered
            batches.append(((choice, m0, m1), (u, e, out), ctr, tw))
            ctr += (mm + 127) // 128
            tw += mm
    finally:
        S.close(); R.close()
    return (seeds0, seeds1, delta), batches


def _check_labels_mirror(gccpu, keys, inputs, got, ctr, tw):
    seeds0, seeds1, delta = keys
    choice, m0, m1 = inputs
    u, e, out = got
    m = len(choice)
    cu, rt, rq = gccpu.iknp_extend(seeds0, seeds1, delta.tobytes(), np.packbits(choice, bitorder="little"), m, ctr)
    ce, cout = gccpu.iknp_labels(rt, rq, delta.tobytes(), choice, m0, m1, tw)
    assert np.array_equal(u, cu), m
    assert np.array_equal(e, ce), m
    assert np.array_equal(out, cout), m


def _check_labels_openssl(keys, inputs, got, ctr, tw):
    seeds0, seeds1, delta = keys
    choice, m0, m1 = inputs
    u, e, out = got
    m = len(choice)
    U, rows_t, rows_q = iknp_restatement(seeds0, seeds1, delta, np.packbits(choice, bitorder="little"), m, ctr)
    e0, e1, exp_out = iknp_labels_restatement(rows_t, rows_q, delta, choice, m0, m1, tw)
    assert np.array_equal(np.asarray(u, dtype=np.uint8).reshape(-1), U.reshape(-1)), m
    ge = np.asarray(e, dtype=np.uint8).reshape(m, 2, 16)
    assert np.array_equal(ge[:, 0], e0) and np.array_equal(ge[:, 1], e1), m
    assert np.array_equal(np.asarray(out, dtype=np.uint8).reshape(m, 16), exp_out), m


LABEL_M = (
    [1]                                                     # a single lane of a single wave
    # 512-OT transpose group, w64 = 2 m128: m128 = k puts the guard first + t + 1 < w64 at m128 mod 4 = 1, 2, 3, 0, 1 inside a
    # wave's eight words (k = 5: a second wave that holds a single block); 128 k + 1 adds a ragged block of one OT
    + [128 * k + r for k in (1, 2, 3, 4, 5) for r in (0, 1)]
    + [1024, 1025]                                          # 1024 lanes: one trip, no `two`; the first `two` of the labels kernels
    + [2049]                                                # 2048 items per workgroup: labels gx = 2
    + [128 * 1025]                                          # 1024 lanes: cols m128 = 1025, the first `two` of ot_cols_kernel
    + [128 * 2049]                                          # 2048 items per workgroup: cols gx = 2
)
# one past 2 * kOtGroups (512) * 1024 lanes: the labels kernels start a second trip with a lone OT; m128 = 8193, one past
# 2 * (cols cap 4) * 1024: ot_cols_kernel starts a second trip with a lone block
LABEL_M_BIG = 2 * 512 * 1024 + 1


@pytest.mark.parametrize("m", LABEL_M + [LABEL_M_BIG])
def test_labels_match_mirror(lgc, gccpu, m):
    keys, batches = _run_label_case(lgc, m)
    for inputs, got, ctr, tw in batches:
        _check_labels_mirror(gccpu, keys, inputs, got, ctr, tw)


def test_labels_big_match_openssl(lgc):
    """+openssl: the second-trip label case against the restatement that shares nothing with the product"""
    keys, batches = _run_label_case(lgc, LABEL_M_BIG)
    for inputs, got, ctr, tw in batches:
        _check_labels_openssl(keys, inputs, got, ctr, tw)


# ---------------------------------------------------------------------------------------------------------------- Gilboa
def _run_gilboa_case(lgc, w, npairs, n):
    """two Gilboa batches ((npairs, n), then GILBOA_SHAPE2[w]) on a fresh session pair; deterministic in the shape"""
    rng = np.random.default_rng(w * 1000003 + npairs * 1009 + n)
    seeds0, seeds1, delta, seeds_s = _setup(rng)
    S = lgc.OtSender(delta.tobytes(), seeds_s); R = lgc.OtReceiver(seeds0, seeds1)
    batches, ctr, tw = [], 0, 0
    try:
        for shape in ((npairs, n), GILBOA_SHAPE2[w]):
            a = _full(rng, shape, w); b = _full(rng, shape, w)
            u = R.gilboa_start(a, w)
            y, ss = S.gilboa(b, w, u)
            sr = R.gilboa_finish(y)
            assert [(int(x) + int(z)) & ((1 << w) - 1) for x, z in zip(ss, sr)] == _ip(a.tolist(), b.tolist(), w), shape
            batches.append(((a, b), (u, y, ss, sr), ctr, tw))
            m = shape[0] * shape[1] * w
            ctr += (m + 127) // 128
            tw += m
    finally:
        S.close(); R.close()
    return (seeds0, seeds1, delta), batches


def _check_gilboa_mirror(gccpu, keys, w, inputs, got, ctr, tw):
    seeds0, seeds1, delta = keys
    a, b = inputs
    u, y, ss, sr = got
    m = a.size * w
    cu, rt, rq = gccpu.iknp_extend(seeds0, seeds1, delta.tobytes(), _cbits(a, w), m, ctr)
    cy, css, csr = gccpu.iknp_gilboa(rt, rq, delta.tobytes(), a, b, w, tw)
    assert np.array_equal(u, cu), a.shape
    assert np.array_equal(y, cy), a.shape
    assert np.array_equal(ss, css) and np.array_equal(sr, csr), a.shape


def _check_gilboa_openssl(keys, w, inputs, got, ctr, tw):
    seeds0, seeds1, delta = keys
    a, b = inputs
    u, y, ss, sr = got
    U, rows_t, rows_q = iknp_restatement(seeds0, seeds1, delta, _cbits(a, w), a.size * w, ctr)
    ey, ess, esr = iknp_gilboa_restatement(rows_t, rows_q, delta, a, b, w, tw)
    assert np.array_equal(np.asarray(u, dtype=np.uint8).reshape(-1), U.reshape(-1)), a.shape
    assert np.array_equal(y, ey), a.shape
    assert np.array_equal(ss, ess) and np.array_equal(sr, esr), a.shape


# +openssl.  npairs = 3 is no power of two: gy = 3, gx = min(ceil(384 000 / 2048), kOtGroups (512) / 3 = 170) = 170, stride
# 170 * 1024 = 174 080; mpp = 6000 * 64 = 384 000 > 2 * stride: every lane of the first trip takes `two`, and a second trip
# (t from 348 160) runs in part of the grid without it
GILBOA_BIG = (64, 3, 6000)
GILBOA_SHAPES = [
    (32, 1, 1),            # a single partial wave: 32 OTs, a quarter block
    (32, 3, 17),           # npairs * n odd: ot_pack_choice_words_kernel's last word has hi = 0; m mod 64 = 32
    # kOtGroups = 512: npairs = 513 gives gy = 512 and the pair loop's second trip (q = 512), gx = 512 / 512 = 1, stride 1024 lanes;
    # mpp = n * 64 = 1024: one trip, no `two`; 1088: the first `two`; 2112 = 2048 + 64: a second t trip
    (64, 513, 16), (64, 513, 17), (64, 513, 33),
    (32, 515, 67),         # the same at w = 32: pairs 512..514 on the second q trip, mpp = 67 * 32 = 2144 = 2048 + 96
    GILBOA_BIG,
    # cols cap 4: m128 = 16500 * 64 / 128 = 8250 > 2 * 4 * 1024, ot_cols_kernel's second trip through the Gilboa path (58 blocks,
    # no `two`); npairs = 1: gy = 1, gx = min(ceil(1 056 000 / 2048), kOtGroups) = 512
    (64, 1, 16500),
]


@pytest.mark.parametrize("w,npairs,n", GILBOA_SHAPES)
def test_gilboa_matches_mirror(lgc, gccpu, w, npairs, n):
    keys, batches = _run_gilboa_case(lgc, w, npairs, n)
    for inputs, got, ctr, tw in batches:
        _check_gilboa_mirror(gccpu, keys, w, inputs, got, ctr, tw)


def test_gilboa_big_matches_openssl(lgc):
    """+openssl: the non-power-of-two grid with a second t trip against the restatement that shares nothing with the product"""
    w = GILBOA_BIG[0]
    keys, batches = _run_gilboa_case(lgc, *GILBOA_BIG)
    for inputs, got, ctr, tw in batches:
        _check_gilboa_openssl(keys, w, inputs, got, ctr, tw)


# ------------------------------------------------------------------------------------------------------------- in flight
def test_receives_in_flight_keep_start_order(lgc, gccpu):
    """three receives started before the first is finished: a Gilboa batch with npairs = 513 (kOtGroups: a second pair trip), a
    label batch (m = 2049: labels gx = 2), a ragged w = 32 Gilboa batch.  Finished in order, every transcript equals the mirror's
    at the ctr / tweak positions that the START order implies"""
    rng = np.random.default_rng(4242)
    seeds0, seeds1, delta, seeds_s = _setup(rng)
    keys = (seeds0, seeds1, delta)
    S = lgc.OtSender(delta.tobytes(), seeds_s); R = lgc.OtReceiver(seeds0, seeds1)
    try:
        a1, b1 = _full(rng, (513, 16), 64), _full(rng, (513, 16), 64)
        lab = _label_inputs(rng, 2049)
        a3, b3 = _full(rng, (3, 17), 32), _full(rng, (3, 17), 32)
        u1 = R.gilboa_start(a1, 64)
        u2 = R.labels_start(lab[0])
        u3 = R.gilboa_start(a3, 32)
        y1, ss1 = S.gilboa(b1, 64, u1); sr1 = R.gilboa_finish(y1)
        e2 = S.labels(lab[1], lab[2], u2); out2 = R.labels_finish(e2)
        y3, ss3 = S.gilboa(b3, 32, u3); sr3 = R.gilboa_finish(y3)
    finally:
        S.close(); R.close()
    assert [(int(x) + int(z)) & (2 ** 64 - 1) for x, z in zip(ss1, sr1)] == _ip(a1.tolist(), b1.tolist(), 64)
    assert np.array_equal(out2, np.where(lab[0][:, None] == 1, lab[2], lab[1]))
    assert [(int(x) + int(z)) & (2 ** 32 - 1) for x, z in zip(ss3, sr3)] == _ip(a3.tolist(), b3.tolist(), 32)
    m1, m2 = 513 * 16 * 64, 2049
    ctr2 = (m1 + 127) // 128; ctr3 = ctr2 + (m2 + 127) // 128
    _check_gilboa_mirror(gccpu, keys, 64, (a1, b1), (u1, y1, ss1, sr1), 0, 0)
    _check_labels_mirror(gccpu, keys, lab, (u2, e2, out2), ctr2, m1)
    _check_gilboa_mirror(gccpu, keys, 32, (a3, b3), (u3, y3, ss3, sr3), ctr3, m1 + m2)


# ------------------------------------------------------------------------------------------------------------ device I/O
def test_device_io_matches_host_io(lgc):
    """lgc_ot_*_set_device_io: operands, u, y / e, out and the shares in device memory (torch tensors, as bench.py's OT
    accounting holds them) give the bytes of a host-I/O session with the same seeds.  One session pair each way runs
    (64, 513, 33) (kOtGroups: second pair trip; mpp = 2112: second t trip), (32, 3, 17) (odd word count) and a label batch of
    m = 2049 (labels gx = 2, ragged).  At width 32 only the low 32 bits of a device-resident share word are defined
    (include/linreg_gc.h): the accumulator is copied as it is, and the host path masks after the copy."""
    import torch
    rng = np.random.default_rng(555)
    seeds0, seeds1, delta, seeds_s = _setup(rng)
    L = lgc.lib()
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.int64 if v.dtype == np.uint64 else np.uint8)).cuda()
    host = lambda t, dt: t.cpu().numpy().view(dt)
    gil = [(w, _full(rng, (npairs, n), w), _full(rng, (npairs, n), w)) for w, npairs, n in ((64, 513, 33), (32, 3, 17))]
    choice, m0, m1 = _label_inputs(rng, 2049)
    Sh = lgc.OtSender(delta.tobytes(), seeds_s); Rh = lgc.OtReceiver(seeds0, seeds1)
    Sd = lgc.OtSender(delta.tobytes(), seeds_s); Rd = lgc.OtReceiver(seeds0, seeds1)
    try:
        Sd.set_device_io(True); Rd.set_device_io(True)
        for w, a, b in gil:
            npairs, n = a.shape
            m = npairs * n * w
            mask = (1 << w) - 1
            u = Rh.gilboa_start(a, w)
            y, ss = Sh.gilboa(b, w, u)
            sr = Rh.gilboa_finish(y)
            da, db = dev(a), dev(b)
            du = torch.empty(L.lgc_ot_u_bytes(m), dtype=torch.uint8, device="cuda"); dy = torch.empty(m, dtype=torch.int64, device="cuda")
            dss = torch.zeros(npairs, dtype=torch.int64, device="cuda"); dsr = torch.zeros(npairs, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            Rd.gilboa_start_ptr(da.data_ptr(), npairs, n, w, du.data_ptr())
            Sd.gilboa_ptr(db.data_ptr(), npairs, n, w, du.data_ptr(), dy.data_ptr(), dss.data_ptr())
            Rd.gilboa_finish_ptr(dy.data_ptr(), dsr.data_ptr())
            torch.cuda.synchronize()
            gss, gsr = host(dss, np.uint64), host(dsr, np.uint64)
            assert np.array_equal(host(du, np.uint8), u), (w, npairs, n)
            assert np.array_equal(host(dy, np.uint64), y), (w, npairs, n)         # y is masked to w bits by the kernel itself
            if w == 32:
                # only the low 32 bits of a device-resident share are defined; recorded, not asserted: whether the rest is set
                print("w = 32 device shares with bits >= 32 set: sender %d of %d, receiver %d of %d"
                      % (int((gss >> np.uint64(32)).astype(bool).sum()), npairs, int((gsr >> np.uint64(32)).astype(bool).sum()), npairs))
                gss, gsr = gss & np.uint64(mask), gsr & np.uint64(mask)
            assert np.array_equal(gss, ss) and np.array_equal(gsr, sr), (w, npairs, n)
            assert [(int(x) + int(z)) & mask for x, z in zip(gss, gsr)] == _ip(a.tolist(), b.tolist(), w)
        m = len(choice)
        u = Rh.labels_start(choice)
        e = Sh.labels(m0, m1, u)
        out = Rh.labels_finish(e)
        dc, d0, d1 = dev(choice), dev(m0), dev(m1)
        du = torch.empty(L.lgc_ot_u_bytes(m), dtype=torch.uint8, device="cuda")
        de = torch.empty(m * 32, dtype=torch.uint8, device="cuda"); dout = torch.empty(m * 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        vp = C.c_void_p
        assert L.lgc_ot_labels_recv_start(Rd._h, vp(dc.data_ptr()), m, vp(du.data_ptr())) == 0
        assert L.lgc_ot_labels_send(Sd._h, vp(d0.data_ptr()), vp(d1.data_ptr()), m, vp(du.data_ptr()), vp(de.data_ptr())) == 0
        assert L.lgc_ot_labels_recv_finish(Rd._h, vp(de.data_ptr()), vp(dout.data_ptr())) == 0
        torch.cuda.synchronize()
        assert np.array_equal(host(du, np.uint8), u)
        assert np.array_equal(host(de, np.uint8).reshape(m, 32), e)
        assert np.array_equal(host(dout, np.uint8).reshape(m, 16), out)
        assert np.array_equal(out, np.where(choice[:, None] == 1, m1, m0))
    finally:
        for s in (Sh, Rh, Sd, Rd):
            s.close()
