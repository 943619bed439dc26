"""The half-payload form of the matrix Gilboa product (include/linreg_gc_ot_half.h) without a GPU: the numpy / OpenSSL model of
the protocol (tests/ot_half_model.py) recombines to Xr^T Xs at both widths, tail shapes and extreme operands included; its
packing is a bijection; its u is the matrix mode's; the header's names are exported and documented; bin/linreg and
bin/secure_multiplication refuse the option pairs before connecting; LGC_EINVAL precedes device use; the batch rule of the model
and of the host (host/ot_matrix_plan.c, under the sanitizers in a program of its own)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ot_half_model as hm
import ot_matrix_model as om
from test_ot import _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "linreg-mpc_amd", "host")
NAMES = {"lgc_ot_gilboa_half_y_bytes", "lgc_ot_gilboa_half_recv_start", "lgc_ot_gilboa_half_send", "lgc_ot_gilboa_half_recv_finish"}
TAIL_SHAPES = [
    (64, 1, 1, 1), (64, 3, 3, 2), (64, 5, 3, 5), (64, 2, 13, 11),      # half a block, an exact block, nblk = 3 with a half tail, nblk = 6
    (32, 1, 3, 3), (32, 7, 2, 4), (32, 9, 5, 9), (32, 2, 1, 6),        # a 96-bit tail, an exact block, one word / two words in the tail
]


def _full(rng, shape, w):
    v = rng.integers(0, 2 ** 63, size=shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=shape, dtype=np.uint64)
    return v & np.uint64((1 << w) - 1)


def _sums_to_product(e, xr, xs, w):
    with np.errstate(over="ignore"):
        total = (e["share_s"] + e["share_r"]) & om.mask(w)
    assert np.array_equal(total, om.product(xr, xs, w)) and np.array_equal(total, om.product_int(xr, xs, w))
    assert not (e["share_s"] >> np.uint64(w - 1) >> np.uint64(1)).any() and not (e["share_r"] >> np.uint64(w - 1) >> np.uint64(1)).any()


# ---- the model
@pytest.mark.parametrize("w,rows,r,s", TAIL_SHAPES)
def test_model_shares_sum_to_the_product(w, rows, r, s):
    """share_s + share_r = Xr^T Xs mod 2^W, the product once in wrapping uint64 and once in Python integers; from a counter and a
    tweak that are not zero; y has the wire form's shape and size; the counters advance by ceil(M / 128) and M nblk; u is the
    matrix mode's u for the same inputs, and the individual shares are not the matrix mode's"""
    rng = np.random.default_rng(100 * w + 10 * rows + s)
    seeds0, seeds1, delta, _ = _setup(rng)
    xr, xs = _full(rng, (rows, r), w), _full(rng, (rows, s), w)
    e = hm.run(seeds0, seeds1, delta, xr, xs, w, 5, 12345)
    m = rows * r * w
    _sums_to_product(e, xr, xs, w)
    assert e["y"].shape == (rows * r * (w // 2 + 1), s) and e["y"].dtype == (np.uint32 if w == 32 else np.uint64)
    assert e["y"].nbytes == hm.y_bytes(rows, r, s, w) == rows * r * (w // 2 + 1) * s * w // 8
    assert e["share_s"].shape == (r, s) and e["share_r"].shape == (r, s)
    assert len(e["u"]) == (m + 127) // 128 * 128 * 16
    assert e["ctr"] == 5 + (m + 127) // 128 and e["tweak"] == 12345 + m * ((s * w + 127) // 128)
    full = om.run(seeds0, seeds1, delta, xr, xs, w, 5, 12345)
    assert np.array_equal(e["u"], full["u"]) and (e["ctr"], e["tweak"]) == (full["ctr"], full["tweak"])
    assert not np.array_equal(e["share_s"], full["share_s"])
    # the high half of word W / 2 of every (k, ir, j) is zero
    mid = e["y"].reshape(rows * r, w // 2 + 1, s)[:, w // 2].astype(np.uint64)
    assert not (mid >> np.uint64(w // 2)).any()


@pytest.mark.parametrize("w", [64, 32])
@pytest.mark.parametrize("case", ["xs_max", "xr_max", "xr_zero"])
def test_model_extreme_operands(w, case):
    """Xs all 2^W - 1 (every field of y' sees the largest correlation), Xr all 2^W - 1 (every choice bit set), Xr = 0 (none)"""
    rows, r, s = 3, 2, 3
    rng = np.random.default_rng(w + len(case))
    seeds0, seeds1, delta, _ = _setup(rng)
    xr, xs = _full(rng, (rows, r), w), _full(rng, (rows, s), w)
    if case == "xs_max":
        xs[:] = om.mask(w)
    elif case == "xr_max":
        xr[:] = om.mask(w)
    else:
        xr[:] = 0
    e = hm.run(seeds0, seeds1, delta, xr, xs, w, 3, 777)
    _sums_to_product(e, xr, xs, w)
    if case == "xr_zero":
        assert not om.product(xr, xs, w).any()


@pytest.mark.parametrize("w", [64, 32])
def test_pack_is_a_bijection(w):
    """unpack(pack(.)) is the identity on fields of W, W - 1, ..., 1 bits, random and all maximal; pack(unpack(.)) is the identity on
    words whose middle word has a zero high half; the high half of word W / 2 is zero; word 0 is the field of bit 0, word p holds bit p
    below and bit W - p above"""
    rng = np.random.default_rng(w)
    g, s = 5, 3
    masks = hm.field_masks(w)
    assert [int(v) for v in masks] == [(1 << (w - b)) - 1 for b in range(w)]
    for fields in (_full(rng, (g, w, s), w) & masks[None, :, None], np.broadcast_to(masks[None, :, None], (g, w, s)).copy()):
        y = hm.pack(fields, w)
        assert y.shape == (g, w // 2 + 1, s) and y.dtype == (np.uint32 if w == 32 else np.uint64)
        assert np.array_equal(hm.unpack(y, w), fields)
        assert np.array_equal(hm.pack(hm.unpack(y, w), w), y)
        assert not (y[:, w // 2].astype(np.uint64) >> np.uint64(w // 2)).any()
        assert np.array_equal(y[:, 0].astype(np.uint64), fields[:, 0])
        for p in (1, w // 2 - 1):
            word = [[int(a) | (int(b) << (w - p)) for a, b in zip(ra, rb)] for ra, rb in zip(fields[:, p].tolist(), fields[:, w - p].tolist())]
            assert y[:, p].astype(np.uint64).tolist() == word
    # all fields maximal: every word but the middle one is all ones
    y = hm.pack(np.broadcast_to(masks[None, :, None], (1, w, 1)).copy(), w).astype(np.uint64).ravel()
    assert all(int(v) == (1 << w) - 1 for v in y[:w // 2]) and int(y[w // 2]) == (1 << (w // 2)) - 1


def test_y_bytes():
    for rows, r, s in ((1, 1, 1), (3, 5, 7), (10000, 50, 50)):
        for w in (32, 64):
            assert hm.y_bytes(rows, r, s, w) == rows * r * (w // 2 + 1) * s * w // 8
    # n = 10^4, 51 columns (50 and y) against 50 at W = 64: 13 056 000 000 bytes in the matrix mode, 33/64 of it here; 17/32 at W = 32
    assert 10000 * 51 * 64 * 50 * 8 == 13056000000 and hm.y_bytes(10000, 51, 50, 64) == 6732000000 == 13056000000 * 33 // 64
    assert hm.y_bytes(7, 3, 5, 32) * 32 == om.ots(7, 3, 32) * 5 * 4 * 17


def test_model_batch_rule():
    """as many whole rows as keep M <= 2^24 and the half y <= 256 MiB, and at least one"""
    assert hm.batch_rows(10, 3, 2, 64) == [10]
    assert hm.rows_per_batch(50, 50, 64) == (256 << 20) // (50 * 33 * 50 * 8) == 406          # y binds: about twice the matrix mode's 209
    assert hm.batch_rows(10000, 50, 50, 64) == [406] * 24 + [256]
    assert hm.rows_per_batch(50, 50, 32) == (256 << 20) // (50 * 17 * 50 * 4) == 1579
    assert hm.batch_rows(100000, 8, 1, 64) == [32768, 32768, 32768, 1696]                      # M binds: 2^24 / (8 * 64)
    assert hm.batch_rows(3, 1 << 20, 4, 64) == [1, 1, 1]                                       # at least one row
    assert hm.rows_per_batch(8, 3, 64) == (1 << 24) // (8 * 64) and hm.rows_per_batch(8, 4, 64) == (256 << 20) // (8 * 33 * 4 * 8) < (1 << 24) // (8 * 64)
    for n, r, s, w in ((10000, 50, 50, 64), (100000, 8, 1, 64), (777, 5, 3, 32)):
        b = hm.batch_rows(n, r, s, w)
        assert sum(b) == n and all(x * r * w <= 1 << 24 and hm.y_bytes(x, r, s, w) <= 256 << 20 for x in b)


def test_host_batch_rule_equals_the_model_under_sanitizers(tmp_path):
    """host/ot_matrix_plan.c compiled with ASan + UBSan into a program of its own (tests/tools/asan_ot_half.c) and run: the rows of
    a batch are the model's for shapes on both sides of both bounds (at W = 64 the y bound binds from s = 4, at W = 32 from s = 8);
    nothing is loaded into python"""
    import shutil
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    shapes = [(3, 2, 64), (50, 50, 64), (50, 51, 64), (50, 50, 32), (8, 1, 64), (8, 3, 64), (8, 4, 64), (5, 7, 32), (5, 8, 32), (1, 1, 32),
              (1 << 20, 4, 64), (4096, 64, 64), (4097, 3, 32)]
    exe = str(tmp_path / "asan_ot_half")
    cc = subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", HOST,
                         os.path.join(ROOT, "tests", "tools", "asan_ot_half.c"), os.path.join(HOST, "ot_matrix_plan.c"), "-o", exe],
                        capture_output=True, text=True)
    if cc.returncode != 0 and "cannot find" in cc.stderr and "san" in cc.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert cc.returncode == 0, cc.stderr[-2000:]
    run = subprocess.run([exe] + [str(v) for sh in shapes for v in sh], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("all ok"), (run.stdout[-1500:], run.stderr[-3000:])
    got = [int(x) for x in run.stdout.split()[:-2]]
    assert got == [hm.rows_per_batch(r, s, w) for r, s, w in shapes]
    assert hm.rows_per_batch(8, 3, 64) == (1 << 24) // (8 * 64) and hm.rows_per_batch(5, 7, 32) == (1 << 24) // (5 * 32)      # the OT bound binds
    assert hm.rows_per_batch(8, 4, 64) < (1 << 24) // (8 * 64) and hm.rows_per_batch(5, 8, 32) < (1 << 24) // (5 * 32)        # the y bound binds


# ---- the header, the exports, the documents
def test_header_is_exported_and_documented(lgc):
    hdr = open(os.path.join(ROOT, "include", "linreg_gc_ot_half.h")).read()
    names = set(re.findall(r"^[a-z][^\n(]*?\b(lgc_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    assert names == NAMES
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for nme in names:
        assert hasattr(lgc.lib(), nme), nme
        assert nme in doc.split("### 1.19", 1)[1], nme
    assert "linreg_gc_ot_half.h" in doc and "### 1.19" in doc and "--ot_half" in doc.split("### 1.19", 1)[1]
    assert "ot_gilboa_half_send_kernel" in design and "ot_gilboa_half_recv_kernel" in design and "--ot_half" in design
    assert "--ot_half" in readme
    for m in ("gilboa_half_start", "gilboa_half_finish", "gilboa_half_start_ptr", "gilboa_half_finish_ptr"):
        assert hasattr(lgc.OtReceiver, m), m
    for m in ("gilboa_half", "gilboa_half_ptr"):
        assert hasattr(lgc.OtSender, m), m
    # linreg_gc.h and linreg_gc_ot_matrix.h keep their entry points: the new ones live in the new header alone
    for old in ("linreg_gc.h", "linreg_gc_ot_matrix.h"):
        assert "gilboa_half" not in open(os.path.join(ROOT, "include", old)).read(), old


# ---- the option pairs refused before any connection
def _run(exe, *args):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    inp = os.path.join(ROOT, "tests", "golden", "readme_example.in")             # n = 10, d = 5
    return subprocess.run([os.path.join(HOST, "bin", exe), inp, "56", "3"] + list(args), capture_output=True, timeout=60)


@pytest.mark.parametrize("exe,args,want", [
    ("linreg", ["cgd", "10", "0.001", "--ot_half"], b"--ot_half needs --use_ot --ot_matrix"),
    ("linreg", ["cgd", "10", "0.001", "--use_ot", "--ot_half"], b"--ot_half needs --use_ot --ot_matrix"),
    ("linreg", ["cgd", "10", "0.001", "--ot_half", "--ot_matrix"], b"--ot_half needs --use_ot --ot_matrix"),
    ("linreg", ["cgd", "10", "0.001", "--use_ot", "--ot_matrix", "--ot_half", "--ot_ring"], b"--ot_matrix and --ot_ring exclude each other"),
    ("linreg", ["cholesky", "0", "0.001", "--scan=2", "--use_ot", "--ot_matrix", "--ot_half"], b"--ot_matrix and --scan exclude each other"),
    ("secure_multiplication", ["--ot_half"], b"--ot_half needs --use_ot --ot_matrix"),
    ("secure_multiplication", ["--use_ot", "--ot_half"], b"--ot_half needs --use_ot --ot_matrix"),
    ("secure_multiplication", ["--ot_matrix", "--ot_half"], b"--ot_half needs --use_ot --ot_matrix"),
])
def test_refused_option_pairs(exe, args, want):
    r = _run(exe, *args)
    assert r.returncode != 0, args
    assert (r.stdout + r.stderr).rstrip().endswith(want), (args, r.stdout[-300:], r.stderr[-300:])
    assert b"finished phase 1" not in r.stdout and b"bytes_sent" not in r.stdout and b"Result" not in r.stdout


def test_help_names_the_option():
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    for exe in ("linreg", "secure_multiplication"):
        r = subprocess.run([os.path.join(HOST, "bin", exe)], capture_output=True, timeout=60)
        assert r.returncode != 0 and b"--ot_half" in r.stderr, exe


# ---- LGC_EINVAL before any device use
def test_einval_precedes_device_use(lgc):
    """no session exists on a machine without a GPU: the arguments are judged before the session is touched, so a block of zeroed
    memory stands in for it"""
    L = lgc.lib()
    buf = (C.c_uint64 * 4)()
    fake = (C.c_uint64 * 1024)()
    p, h = C.cast(buf, C.c_void_p), C.cast(fake, C.c_void_p)

    def refused(rc, want):
        assert rc == -1 and want in L.lgc_last_error().decode(), (rc, L.lgc_last_error())          # LGC_EINVAL

    for args in ((None, p, 1, 1, 1, 64, p), (h, None, 1, 1, 1, 64, p), (h, p, 1, 1, 1, 64, None)):
        refused(L.lgc_ot_gilboa_half_recv_start(*args), "null")
    for args in ((None, p, 1, 1, 1, 64, p, p, p), (h, None, 1, 1, 1, 64, p, p, p), (h, p, 1, 1, 1, 64, None, p, p),
                 (h, p, 1, 1, 1, 64, p, None, p), (h, p, 1, 1, 1, 64, p, p, None)):
        refused(L.lgc_ot_gilboa_half_send(*args), "null")
    for args in ((None, p, p), (h, None, p), (h, p, None)):
        refused(L.lgc_ot_gilboa_half_recv_finish(*args), "null")
    for width in (0, 16, 48, 128):
        refused(L.lgc_ot_gilboa_half_recv_start(h, p, 1, 1, 1, width, p), "width must be 32 or 64")
        refused(L.lgc_ot_gilboa_half_send(h, p, 1, 1, 1, width, p, p, p), "width must be 32 or 64")
        assert L.lgc_ot_gilboa_half_y_bytes(1, 1, 1, width) == 0
    for dims in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        refused(L.lgc_ot_gilboa_half_recv_start(h, p, *dims, 64, p), "empty block")
        refused(L.lgc_ot_gilboa_half_send(h, p, *dims, 32, p, p, p), "empty block")
    refused(L.lgc_ot_gilboa_half_recv_start(h, p, 1 << 20, 1 << 6, 1, 64, p), "2^32 OTs")
    refused(L.lgc_ot_gilboa_half_send(h, p, 1 << 20, 1 << 7, 1, 32, p, p, p), "2^32 OTs")
    # r * nblk = 2^31 slots with few OTs: too wide
    refused(L.lgc_ot_gilboa_half_recv_start(h, p, 1, 1 << 20, 1 << 12, 64, p), "block too wide")
    refused(L.lgc_ot_gilboa_half_send(h, p, 1, 1 << 20, 1 << 12, 64, p, p, p), "block too wide")
    # M = 2^31 OTs and 2^30 slots pass the other bounds, y would be 33 * 2^59 bytes: refused, and the size function says 0, not a wrapped number
    refused(L.lgc_ot_gilboa_half_recv_start(h, p, 1 << 25, 1, 1 << 31, 64, p), "y of 2^63 bytes or more")
    refused(L.lgc_ot_gilboa_half_send(h, p, 1 << 25, 1, 1 << 31, 64, p, p, p), "y of 2^63 bytes or more")
    assert L.lgc_ot_gilboa_half_y_bytes(1 << 25, 1, 1 << 31, 64) == 0 and L.lgc_ot_gilboa_half_y_bytes(1 << 40, 1 << 40, 1, 32) == 0
    assert L.lgc_ot_gilboa_half_y_bytes(1 << 25, 1, 1 << 28, 64) == 33 << 56
    assert not any(fake) and not any(buf)
    assert L.lgc_ot_gilboa_half_y_bytes(3, 5, 7, 64) == 3 * 5 * 33 * 7 * 8 and L.lgc_ot_gilboa_half_y_bytes(3, 5, 7, 32) == 3 * 5 * 17 * 7 * 4


# ---- the two payload forms are one path in the library: the same refusals, sizes in the ratio (W / 2 + 1) : W
BLOCK_ARGS = [      # (rows, r, s, width) and what both forms say to it (None: both accept), in the precedence of the checks
    ((1, 1, 1, 0), "width must be 32 or 64"), ((3, 5, 7, 48), "width must be 32 or 64"), ((0, 1, 1, 16), "width must be 32 or 64"),
    ((0, 1, 1, 64), "empty block"), ((1, 0, 1, 32), "empty block"), ((1, 1, 0, 64), "empty block"), ((0, 1 << 32, 1, 64), "empty block"),
    ((1 << 20, 1 << 6, 1, 64), "2^32 OTs"), ((1 << 20, 1 << 7, 1, 32), "2^32 OTs"), ((1 << 32, 1, 1, 64), "2^32 OTs"),
    ((1 << 26, 1 << 6, 1 << 31, 64), "2^32 OTs"),                              # (also too wide, and y too large)
    ((1, 1 << 20, 1 << 12, 64), "block too wide"), ((1 << 5, 1 << 20, 1 << 31, 64), "block too wide"),      # (the second: y too large as well)
    ((1 << 25, 1, 1 << 31, 64), "y of 2^63 bytes or more"),                    # both products leave 64 bits
    ((1 << 26, 1, 1 << 31, 32), "y of 2^63 bytes or more"),                    # the matrix y is 2^64, the half y 17 * 2^59: within 64 bits, not 63
    ((1, 1, 1, 64), None), ((1, 1, 1, 32), None), ((3, 5, 7, 64), None), ((3, 5, 7, 32), None), ((10000, 51, 50, 64), None),
    ((1 << 25, 1, 1 << 28, 64), None),                                         # y of 2^62 and of 33 * 2^56 bytes
]


@pytest.mark.parametrize("dims,want", BLOCK_ARGS)
def test_both_forms_refuse_alike_and_size_in_ratio(lgc, dims, want):
    """what folding the matrix and the half-payload entry points into one path rests on: on one list of arguments both forms give
    the same status and the same message from recv_start and from send, a null pointer is refused before anything else, and
    where they accept (which no call can show without a device: only the size functions are called then) the sizes of y are
    rows r W s W / 8 and (W / 2 + 1) / W of it.  As test_einval_precedes_device_use, zeroed memory stands in for the sessions"""
    L = lgc.lib()
    buf, fake = (C.c_uint64 * 4)(), (C.c_uint64 * 1024)()
    p, h = C.cast(buf, C.c_void_p), C.cast(fake, C.c_void_p)
    rows, r, s, w = dims
    said = []
    for form in ("matrix", "half"):
        start, send, size = (getattr(L, "lgc_ot_gilboa_%s_%s" % (form, op)) for op in ("recv_start", "send", "y_bytes"))
        out = [(start(None, p, *dims, p), L.lgc_last_error()), (send(h, p, *dims, p, None, p), L.lgc_last_error())]
        assert all(rc == -1 and b"null" in msg for rc, msg in out), (form, out)
        if want is not None:
            out += [(start(h, p, *dims, p), L.lgc_last_error()), (send(h, p, *dims, p, p, p), L.lgc_last_error())]
            assert all(rc == -1 and want in msg.decode() for rc, msg in out[2:]), (form, out)
        said.append((out, size(*dims)))
    assert said[0][0] == said[1][0]
    assert not any(fake) and not any(buf)
    # the size functions judge the width and the 63 bits alone: each form's own words per (row, receiver column, sender column)
    size = lambda words: (lambda v: v if w in (32, 64) and v < 1 << 63 else 0)(rows * r * words * s * w // 8)
    assert (said[0][1], said[1][1]) == (size(w), size(w // 2 + 1))
    if want is None:
        assert said[0][1] and said[1][1] * w == said[0][1] * (w // 2 + 1)


def test_forms_differ_only_where_their_own_y_ends():
    """the one argument range on which the forms part: each form's limit is on its OWN y, so a block whose matrix y reaches 2^63 bytes
    while its half y does not is a matrix refusal and a half-payload block (the models' sizes; the library's are pinned to them
    above and in test_einval_precedes_device_use)"""
    rows, r, s, w = 1 << 25, 1, 1 << 29, 64
    assert om.ots(rows, r, w) < 1 << 32 and r * om.nblk(s, w) < 1 << 31
    assert rows * r * w * s * w // 8 == 1 << 63 and hm.y_bytes(rows, r, s, w) == 33 << 57 < 1 << 63
