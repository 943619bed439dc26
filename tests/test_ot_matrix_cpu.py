"""Gilboa with one vector OT per operand bit (include/linreg_gc_ot_matrix.h) without a GPU: the numpy / OpenSSL model of the
protocol (tests/ot_matrix_model.py) recombines to Xr^T Xs at both widths, tail shapes included; the header's names are
exported and documented; bin/linreg and bin/secure_multiplication refuse the option pairs before connecting; LGC_EINVAL
precedes device use; the batch rule of the model and of the host (host/ot_matrix_plan.c, under the sanitizers in a program of its own)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ot_matrix_model as om
from test_ot import _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "linreg-mpc_amd", "host")
NAMES = {"lgc_ot_gilboa_matrix_y_bytes", "lgc_ot_gilboa_matrix_recv_start", "lgc_ot_gilboa_matrix_send", "lgc_ot_gilboa_matrix_recv_finish"}


def _full(rng, shape, w):
    v = rng.integers(0, 2 ** 63, size=shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=shape, dtype=np.uint64)
    return v & np.uint64((1 << w) - 1)


# ---- the model
@pytest.mark.parametrize("w,rows,r,s", [
    (64, 1, 1, 1), (64, 3, 3, 2), (64, 5, 3, 5), (64, 2, 13, 11),      # half a block, an exact block, nblk = 3 with a half tail, nblk = 6
    (32, 1, 3, 3), (32, 7, 2, 4), (32, 9, 5, 9), (32, 2, 1, 6),        # a 96-bit tail, an exact block, one word / two words in the tail
])
def test_model_shares_sum_to_the_product(w, rows, r, s):
    """share_s + share_r = Xr^T Xs mod 2^W, the product once in wrapping uint64 and once in Python integers; from a counter and a
    tweak that are not zero; y and the shares stay within W bits; the counters advance by ceil(M / 128) and M nblk"""
    rng = np.random.default_rng(100 * w + 10 * rows + s)
    seeds0, seeds1, delta, _ = _setup(rng)
    xr, xs = _full(rng, (rows, r), w), _full(rng, (rows, s), w)
    e = om.run(seeds0, seeds1, delta, xr, xs, w, 5, 12345)
    m = rows * r * w
    with np.errstate(over="ignore"):
        total = (e["share_s"] + e["share_r"]) & om.mask(w)
    assert np.array_equal(total, om.product(xr, xs, w)) and np.array_equal(total, om.product_int(xr, xs, w))
    assert e["y"].shape == (m, s) and e["y"].dtype == (np.uint32 if w == 32 else np.uint64) and e["y"].nbytes == m * s * w // 8
    assert e["share_s"].shape == (r, s) and e["share_r"].shape == (r, s)
    assert not (e["share_s"] >> np.uint64(w - 1) >> np.uint64(1)).any() and not (e["share_r"] >> np.uint64(w - 1) >> np.uint64(1)).any()
    assert len(e["u"]) == (m + 127) // 128 * 128 * 16
    assert e["ctr"] == 5 + (m + 127) // 128 and e["tweak"] == 12345 + m * ((s * w + 127) // 128)


def test_model_pads_follow_the_definition():
    """block c of OT i under tweak0 + i nblk + c, word e of block c for column c (128 / W) + e, little-endian, the rest dropped"""
    from helpers import openssl_gate_hash
    rng = np.random.default_rng(9)
    rows128 = rng.integers(0, 256, size=(3, 16), dtype=np.uint8)
    for w, s in ((64, 3), (32, 5)):
        nb, wpb = om.nblk(s, w), 128 // w
        got = om.pads(rows128, s, w, 1000)
        for i in range(3):
            for j in range(s):
                c, e = divmod(j, wpb)
                h = openssl_gate_hash(rows128[i:i + 1], [1000 + i * nb + c])[0]
                assert int(got[i, j]) == int.from_bytes(h[e * w // 8:(e + 1) * w // 8].tobytes(), "little"), (w, i, j)


def test_model_batch_rule():
    """as many whole rows as keep M <= 2^24 and y <= 256 MiB, and at least one"""
    assert om.batch_rows(10, 3, 2, 64) == [10]
    assert om.batch_rows(10000, 50, 50, 64) == [209] * 47 + [177]                  # y binds: 256 MiB / (50 * 64 * 50 * 8)
    assert om.batch_rows(10000, 50, 50, 32) == [838] * 11 + [782]                  # y binds: 256 MiB / (50 * 32 * 50 * 4)
    assert om.batch_rows(100000, 8, 1, 64) == [32768, 32768, 32768, 1696]          # M binds: 2^24 / (8 * 64)
    assert om.batch_rows(3, 1 << 20, 4, 64) == [1, 1, 1]                           # at least one row
    for n, r, s, w in ((10000, 50, 50, 64), (100000, 8, 1, 64), (777, 5, 3, 32)):
        b = om.batch_rows(n, r, s, w)
        assert sum(b) == n and all(x * r * w <= 1 << 24 and x * r * w * s * w // 8 <= 256 << 20 for x in b)


def test_host_batch_rule_equals_the_model_under_sanitizers(tmp_path):
    """host/ot_matrix_plan.c compiled with ASan + UBSan into a program of its own (tests/tools/asan_ot_matrix.c) and run: the rows
    of a batch are the model's for shapes on both sides of both bounds; nothing is loaded into python"""
    import shutil
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    shapes = [(3, 2, 64), (50, 50, 64), (50, 51, 64), (50, 50, 32), (8, 1, 64), (1, 1, 32), (1 << 20, 4, 64), (4096, 64, 64), (4097, 3, 32)]
    exe = str(tmp_path / "asan_ot_matrix")
    cc = subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", HOST,
                         os.path.join(ROOT, "tests", "tools", "asan_ot_matrix.c"), os.path.join(HOST, "ot_matrix_plan.c"), "-o", exe],
                        capture_output=True, text=True)
    if cc.returncode != 0 and "cannot find" in cc.stderr and "san" in cc.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert cc.returncode == 0, cc.stderr[-2000:]
    run = subprocess.run([exe] + [str(v) for sh in shapes for v in sh], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("all ok"), (run.stdout[-1500:], run.stderr[-3000:])
    got = [int(x) for x in run.stdout.split()[:-2]]
    assert got == [om.rows_per_batch(r, s, w) for r, s, w in shapes]


# ---- the header, the exports, the documents
def test_header_is_exported_and_documented(lgc):
    hdr = open(os.path.join(ROOT, "include", "linreg_gc_ot_matrix.h")).read()
    names = set(re.findall(r"^[a-z][^\n(]*?\b(lgc_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    assert names == NAMES
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for nme in names:
        assert hasattr(lgc.lib(), nme), nme
        assert nme in doc, nme
    assert "linreg_gc_ot_matrix.h" in doc and "### 1.18" in doc and "--ot_matrix" in doc.split("### 1.18", 1)[1]
    assert "ot_gilboa_matrix_send_kernel" in design and "ot_gilboa_matrix_recv_kernel" in design and "--ot_matrix" in design
    assert "--ot_matrix" in readme
    for m in ("gilboa_matrix_start", "gilboa_matrix_finish", "gilboa_matrix_start_ptr", "gilboa_matrix_finish_ptr"):
        assert hasattr(lgc.OtReceiver, m), m
    for m in ("gilboa_matrix", "gilboa_matrix_ptr"):
        assert hasattr(lgc.OtSender, m), m
    # linreg_gc.h keeps its entry points: the new ones live in the new header alone
    assert "gilboa_matrix" not in open(os.path.join(ROOT, "include", "linreg_gc.h")).read()


# ---- the option pairs refused before any connection
def _run(exe, *args):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    inp = os.path.join(ROOT, "tests", "golden", "readme_example.in")             # n = 10, d = 5
    return subprocess.run([os.path.join(HOST, "bin", exe), inp, "56", "3"] + list(args), capture_output=True, timeout=60)


@pytest.mark.parametrize("exe,args,want", [
    ("linreg", ["cgd", "10", "0.001", "--ot_matrix"], b"--ot_matrix needs --use_ot"),
    ("linreg", ["cgd", "10", "0.001", "--use_ot", "--ot_matrix", "--ot_ring"], b"--ot_matrix and --ot_ring exclude each other"),
    ("linreg", ["cgd", "10", "0.001", "--ot_ring", "--ot_matrix"], b"--ot_matrix and --ot_ring exclude each other"),
    ("linreg", ["cholesky", "0", "0.001", "--scan=2", "--use_ot", "--ot_matrix"], b"--ot_matrix and --scan exclude each other"),
    ("linreg", ["cholesky", "0", "0.001", "--ot_matrix", "--use_ot", "--scan=2"], b"--ot_matrix and --scan exclude each other"),
    ("secure_multiplication", ["--ot_matrix"], b"--ot_matrix needs --use_ot"),
])
def test_refused_option_pairs(exe, args, want):
    r = _run(exe, *args)
    assert r.returncode != 0, args
    assert (r.stdout + r.stderr).rstrip().endswith(want + (b" (it is a mode of the OT-based phase 1)" if b"needs" in want else b"")), (args, r.stdout[-300:], r.stderr[-300:])
    assert b"finished phase 1" not in r.stdout and b"bytes_sent" not in r.stdout and b"Result" not in r.stdout


def test_help_names_the_option():
    for exe in ("linreg", "secure_multiplication"):
        r = subprocess.run([os.path.join(HOST, "bin", exe)], capture_output=True, timeout=60)
        assert r.returncode != 0 and b"--ot_matrix" in r.stderr, exe


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
        refused(L.lgc_ot_gilboa_matrix_recv_start(*args), "null")
    for args in ((None, p, 1, 1, 1, 64, p, p, p), (h, None, 1, 1, 1, 64, p, p, p), (h, p, 1, 1, 1, 64, None, p, p),
                 (h, p, 1, 1, 1, 64, p, None, p), (h, p, 1, 1, 1, 64, p, p, None)):
        refused(L.lgc_ot_gilboa_matrix_send(*args), "null")
    for args in ((None, p, p), (h, None, p), (h, p, None)):
        refused(L.lgc_ot_gilboa_matrix_recv_finish(*args), "null")
    for width in (0, 16, 48, 128):
        refused(L.lgc_ot_gilboa_matrix_recv_start(h, p, 1, 1, 1, width, p), "width must be 32 or 64")
        refused(L.lgc_ot_gilboa_matrix_send(h, p, 1, 1, 1, width, p, p, p), "width must be 32 or 64")
        assert L.lgc_ot_gilboa_matrix_y_bytes(1, 1, 1, width) == 0
    for dims in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        refused(L.lgc_ot_gilboa_matrix_recv_start(h, p, *dims, 64, p), "empty block")
        refused(L.lgc_ot_gilboa_matrix_send(h, p, *dims, 32, p, p, p), "empty block")
    refused(L.lgc_ot_gilboa_matrix_recv_start(h, p, 1 << 20, 1 << 6, 1, 64, p), "2^32 OTs")
    # M = 2^31 OTs and 2^30 slots pass the other bounds, y would be 2^65 bytes: refused, and the size function says 0, not a wrapped number
    refused(L.lgc_ot_gilboa_matrix_recv_start(h, p, 1 << 25, 1, 1 << 31, 64, p), "y of 2^63 bytes or more")
    refused(L.lgc_ot_gilboa_matrix_send(h, p, 1 << 25, 1, 1 << 31, 64, p, p, p), "y of 2^63 bytes or more")
    assert L.lgc_ot_gilboa_matrix_y_bytes(1 << 25, 1, 1 << 31, 64) == 0 and L.lgc_ot_gilboa_matrix_y_bytes(1 << 40, 1 << 40, 1, 32) == 0
    assert L.lgc_ot_gilboa_matrix_y_bytes(1 << 25, 1, 1 << 28, 64) == 1 << 62
    assert not any(fake) and not any(buf)
    assert L.lgc_ot_gilboa_matrix_y_bytes(3, 5, 7, 64) == 3 * 5 * 64 * 7 * 8 and L.lgc_ot_gilboa_matrix_y_bytes(3, 5, 7, 32) == 3 * 5 * 32 * 7 * 4
