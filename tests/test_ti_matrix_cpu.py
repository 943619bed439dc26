"""The matrix-triple mode of phase 1 (include/linreg_gc_p1_matrix.h) without a GPU: the numpy model of the protocol
(tests/ti_matrix_model.py) against the integer Gram block, the seed derivation pinned and held against the library's, the
header's exports and documents, the option pairs bin/linreg and bin/secure_multiplication refuse before connecting, and the
LGC_EINVAL cases that precede device use.  Every comparison is word for word."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ti_matrix_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "linreg-mpc_amd", "host")
SEEDS = (bytes(range(16)), bytes(range(16, 32)), bytes(range(32, 48)))


def data(rng, n, d, w):
    """quantised-looking words: signed values that use the whole width, sign-extended to 64 bits as phase 1 stores them"""
    lo, hi = -(1 << (w - 1)), (1 << (w - 1))
    return rng.integers(lo, hi, size=(n, d), dtype=np.int64), rng.integers(lo, hi, size=n, dtype=np.int64)


# ---- the model
@pytest.mark.parametrize("w", [32, 64])
@pytest.mark.parametrize("n,cols_a,cols_b", [(1, [6], [0]), (7, [4, 5, 6], [0, 2]), (33, [5, 2, 6], [4, 0, 1, 3])])
def test_model_shares_sum_to_the_gram_block(w, n, cols_a, cols_b):
    """share_a + share_b = X_a^T X_b mod 2^W with y (column d) among A's columns, the products once in wrapping uint64 and
    once in Python integers"""
    d = 6
    rng = np.random.default_rng(1000 * w + n)
    Xq, yq = data(rng, n, d, w)
    assert d in cols_a
    Xa, Xb = tm.columns(Xq, yq, cols_a), tm.columns(Xq, yq, cols_b)
    want = [[sum(int(Xq[k, i] if i < d else yq[k]) * int(Xq[k, j]) for k in range(n)) & tm.mask(w) for j in cols_b] for i in cols_a]
    for mul in (tm.tmul, tm.tmul_int):
        r = tm.run(Xa, Xb, *SEEDS, w, mul=mul)
        with np.errstate(over="ignore"):
            total = (r["share_a"] + r["share_b"]) & np.uint64(tm.mask(w))
        assert total.tolist() == want
        assert np.array_equal(total, tm.gram_block(Xa, Xb, w, mul=mul))
        for k in ("E", "F", "T", "share_a", "share_b"):
            assert not (r[k] >> np.uint64(w - 1) >> np.uint64(1)).any(), k
        assert r["E"].shape == (n, len(cols_a)) and r["F"].shape == (n, len(cols_b)) and r["T"].shape == (len(cols_a), len(cols_b))
    a, b = tm.run(Xa, Xb, *SEEDS, w), tm.run(Xa, Xb, *SEEDS, w, mul=tm.tmul_int)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_model_streams_are_row_major_words_from_block_zero():
    ks = tm.openssl_aes_ctr(SEEDS[0], 0, 3).tobytes()
    assert tm.stream(SEEDS[0], 2, 3, 64).tolist() == [[int.from_bytes(ks[8 * (3 * k + i):8 * (3 * k + i) + 8], "little") for i in range(3)] for k in range(2)]
    assert tm.stream(SEEDS[0], 3, 2, 32).tolist() == [[int.from_bytes(ks[4 * (2 * k + i):4 * (2 * k + i) + 4], "little") for i in range(2)] for k in range(3)]


# ---- the seed derivation
PINNED = [
    (bytes(range(16)), 0, ("c6a13b37878f5b826f4f8162a1c8d879", "e37cd363dd7c87a09aff0e3e60e09c82", "fb8ae31ba5db9cad97364d8722d47326")),
    (bytes(range(16))[::-1], 5, ("84fd42fa6e626114623c491b85166ae5", "1a52f454d4ccfd9d44f6757efdc114f0", "2a3b32cb2c73f29476f3277a05888ea0")),
]


@pytest.mark.parametrize("master,u,want", PINNED)
def test_seed_derivation_is_pinned(master, u, want):
    """blocks 3u, 3u + 1, 3u + 2 of AES-128-CTR under the master seed; the first value is FIPS-197's key 00..0f on the zero block"""
    assert tuple(s.hex() for s in tm.seeds(master, u)) == want


@pytest.mark.parametrize("master,u,want", PINNED + [(b"\xa5" * 16, (1 << 32) + 7, None), (b"\x00" * 16, 123456789, None)])
def test_library_seeds_equal_the_model(lgc, master, u, want):
    got = lgc.ti_matrix_seeds(master, u)
    assert got == tm.seeds(master, u)
    assert want is None or tuple(s.hex() for s in got) == want


# ---- the header, the exports, the documents
def test_header_is_exported_and_documented(lgc):
    hdr = open(os.path.join(ROOT, "include", "linreg_gc_p1_matrix.h")).read()
    names = set(re.findall(r"^[a-z][^\n(]*?\b(lgc_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    assert names == {"lgc_p1_matrix_mask", "lgc_p1_matrix_share_a", "lgc_p1_matrix_share_b", "lgc_ti_matrix_generate", "lgc_ti_matrix_seeds"}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for nme in names:
        assert hasattr(lgc.lib(), nme), nme
        assert nme in doc, nme
    assert "linreg_gc_p1_matrix.h" in doc and "### 1.17" in doc and "--ti_matrix" in doc.split("### 1.17", 1)[1]
    assert "p1_cross_kernel" in design and "--ti_matrix" in design and "--ti_matrix" in readme
    for m in ("matrix_mask", "matrix_share_a", "matrix_share_b"):
        assert hasattr(lgc.Phase1, m), m
    assert hasattr(lgc, "ti_matrix_generate") and hasattr(lgc, "ti_matrix_seeds")


# ---- the option pairs refused before any connection
def _run(exe, *args):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    inp = os.path.join(ROOT, "tests", "golden", "readme_example.in")             # n = 10, d = 5
    return subprocess.run([os.path.join(HOST, "bin", exe), inp, "56", "3"] + list(args), capture_output=True, timeout=60)


@pytest.mark.parametrize("exe,args,want", [
    ("linreg", ["cgd", "10", "0.001", "--ti_matrix", "--use_ot"], b"--ti_matrix and --use_ot"),
    ("linreg", ["cgd", "10", "0.001", "--use_ot", "--ti_matrix"], b"--ti_matrix and --use_ot"),
    ("linreg", ["cgd", "10", "0.001", "--ti_matrix", "--ot_ring"], b"--ti_matrix and --ot_ring"),
    ("linreg", ["cgd", "10", "0.001", "--ti_matrix", "--ti_ring"], b"--ti_matrix and --ti_ring"),
    ("linreg", ["cholesky", "0", "0.001", "--scan=2", "--ti_matrix"], b"--ti_matrix and --scan"),
    ("secure_multiplication", ["--ti_matrix", "--use_ot"], b"--ti_matrix and --use_ot"),
])
def test_refused_option_pairs(exe, args, want):
    r = _run(exe, *args)
    assert r.returncode != 0 and want in r.stdout + r.stderr, (args, r.stdout[-300:], r.stderr[-300:])
    assert b"finished phase 1" not in r.stdout and b"bytes_sent" not in r.stdout


def test_help_names_the_option():
    r = subprocess.run([os.path.join(HOST, "bin", "linreg")], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"--ti_matrix" in r.stderr


# ---- LGC_EINVAL before any device use
def test_einval_precedes_device_use(lgc):
    L = lgc.lib()
    buf = (C.c_uint64 * 4)()
    cols = (C.c_uint32 * 1)(0)
    s = bytes(16)
    p = C.cast(buf, C.c_void_p)
    pc = C.cast(cols, C.c_void_p)

    def refused(rc, want):
        assert rc == -1 and want in L.lgc_last_error().decode(), (rc, L.lgc_last_error())          # LGC_EINVAL

    refused(L.lgc_p1_matrix_mask(None, pc, 1, s, p), "null")
    refused(L.lgc_p1_matrix_share_a(None, 1, s, s, p, 1, p), "null")
    refused(L.lgc_p1_matrix_share_b(None, pc, 1, p, 1, p, p), "null")
    for args in ((None, s, s), (s, None, s), (s, s, None)):
        refused(L.lgc_ti_matrix_generate(0, *args, 4, 1, 1, 64, p), "null")
    refused(L.lgc_ti_matrix_generate(0, s, s, s, 4, 1, 1, 64, None), "null")
    for width in (0, 16, 48, 128):
        refused(L.lgc_ti_matrix_generate(0, s, s, s, 4, 1, 1, width, p), "width must be 32 or 64")
    refused(L.lgc_ti_matrix_generate(0, s, s, s, 0, 1, 1, 64, p), "empty data")
    refused(L.lgc_ti_matrix_seeds(None, 0, p, p, p), "null")
    refused(L.lgc_ti_matrix_seeds(s, 0, None, p, p), "null")
    refused(L.lgc_ti_matrix_seeds(s, 0, p, p, None), "null")
    # an empty block launches nothing and needs no device: T is not written
    buf[0] = 77
    assert L.lgc_ti_matrix_generate(0, s, s, s, 4, 0, 3, 64, p) == 0 and L.lgc_ti_matrix_generate(0, s, s, s, 4, 3, 0, 32, p) == 0
    assert buf[0] == 77


# ---- the host-only pieces under the sanitizers, as a stand-alone program
def test_host_pieces_under_address_sanitizer(tmp_path):
    """the seed derivation, the plan of instances, the scatter into share_A / share_b and the initializer's messages compiled with
    ASan + UBSan into a program of their own (tests/tools/asan_ti_matrix.cpp) and run: nothing is loaded into python"""
    import shutil
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no gcc")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    obj, exe = str(tmp_path / "plan.o"), str(tmp_path / "asan_ti_matrix")
    steps = (["gcc", "-std=gnu11"] + san + ["-c", os.path.join(HOST, "ti_matrix_plan.c"), "-o", obj],
             ["g++", "-std=c++17"] + san + ["-I", HOST, "-I", os.path.join(ROOT, "linreg-mpc_amd", "csrc"),
                                            os.path.join(ROOT, "tests", "tools", "asan_ti_matrix.cpp"), obj, "-o", exe])
    for cmd in steps:
        cc = subprocess.run(cmd, capture_output=True, text=True)
        if cc.returncode != 0 and "cannot find" in cc.stderr and "san" in cc.stderr:
            pytest.skip("sanitizer runtime not installed")
        assert cc.returncode == 0, cc.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("all ok"), (run.stdout[-1500:], run.stderr[-3000:])
