"""The two references of the keyed streams agree with each other before either is compared with a kernel (no GPU):
helpers' OpenSSL / numpy restatements (openssl_aes_ctr, openssl_gate_hash_fast, iknp_restatement and its two payload
functions) against the slow per-block OpenSSL forms and against the CPU mirror oracle/gc_cpu.cpp (gccpu), byte for byte.
test_ot_edges_gpu.py and test_ti_stream_gpu.py then hold the HIP kernels against both."""
import numpy as np
import pytest

from helpers import (iknp_gilboa_restatement, iknp_labels_restatement, iknp_restatement, openssl_aes_ctr, openssl_gate_hash,
                     openssl_gate_hash_fast)
from test_ot import _openssl_aes_ctr, _setup


@pytest.mark.parametrize("first_block", [0, 5, 2 ** 32 - 3])          # 2^32 - 3: the carry out of the counter's low 32-bit word
def test_openssl_aes_ctr_matches_per_block_form_and_mirror(gccpu, first_block):
    key = bytes(range(40, 56))
    nblocks = 9
    ks = openssl_aes_ctr(key, first_block, nblocks)
    assert ks.dtype == np.uint8 and ks.shape == (nblocks * 16,)
    assert np.array_equal(ks, _openssl_aes_ctr(key, first_block, nblocks))
    assert np.array_equal(ks, gccpu.aes_ctr(key, first_block, nblocks))
    assert len(set(ks.reshape(nblocks, 16).tobytes()[16 * b:16 * b + 16] for b in range(nblocks))) == nblocks   # no block twice
    assert openssl_aes_ctr(key, first_block, 0).size == 0


def test_openssl_gate_hash_fast_matches_slow_form_and_mirror(gccpu):
    rng = np.random.default_rng(21)
    n = 2000
    labels = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    tweaks = rng.integers(0, 2 ** 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    tweaks[:4] = [0, 1, 2 ** 32 - 1, 2 ** 64 - 1]
    fast = openssl_gate_hash_fast(labels, tweaks)
    assert np.array_equal(fast, openssl_gate_hash(labels, tweaks))
    assert np.array_equal(fast, gccpu.gate_hash(labels, tweaks))


def test_label_restatement_matches_mirror(gccpu):
    rng = np.random.default_rng(31)
    seeds0, seeds1, delta, _ = _setup(rng)
    m, ctr0, tweak0 = 2049 + 77, 9, 1234                              # ragged: 17 blocks of 128, the last holds 78 OTs
    choice = rng.integers(0, 2, size=m, dtype=np.uint8)
    m0 = rng.integers(0, 256, size=(m, 16), dtype=np.uint8); m1 = rng.integers(0, 256, size=(m, 16), dtype=np.uint8)
    packed = np.packbits(choice, bitorder="little")
    U, rows_t, rows_q = iknp_restatement(seeds0, seeds1, delta, packed, m, ctr0)
    cu, rt, rq = gccpu.iknp_extend(seeds0, seeds1, delta.tobytes(), packed, m, ctr0)
    assert np.array_equal(U.reshape(-1), cu)
    assert np.array_equal(rows_t.reshape(-1), rt[:m * 16]) and np.array_equal(rows_q.reshape(-1), rq[:m * 16])
    assert np.array_equal(rows_q, rows_t ^ (delta[None, :] * choice[:, None]))          # the IKNP correlation itself
    e0, e1, out = iknp_labels_restatement(rows_t, rows_q, delta, choice, m0, m1, tweak0)
    ce, cout = gccpu.iknp_labels(rt, rq, delta.tobytes(), choice, m0, m1, tweak0)
    assert np.array_equal(ce.reshape(m, 2, 16)[:, 0], e0) and np.array_equal(ce.reshape(m, 2, 16)[:, 1], e1)
    assert np.array_equal(cout, out)
    assert np.array_equal(out, np.where(choice[:, None] == 1, m1, m0))


@pytest.mark.parametrize("w,npairs,n,ctr0,tweak0", [(64, 3, 17, 11, 4321), (32, 3, 17, 3, 2 ** 32 - 100)])
def test_gilboa_restatement_matches_mirror(gccpu, w, npairs, n, ctr0, tweak0):
    rng = np.random.default_rng(w)
    seeds0, seeds1, delta, _ = _setup(rng)
    mask = (1 << w) - 1
    a = rng.integers(0, 2 ** 63, size=(npairs, n), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(npairs, n), dtype=np.uint64)
    b = rng.integers(0, 2 ** 63, size=(npairs, n), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(npairs, n), dtype=np.uint64)
    a &= np.uint64(mask); b &= np.uint64(mask)
    m = npairs * n * w
    cb = a.view(np.uint8) if w == 64 else a.astype(np.uint32).view(np.uint8)
    U, rows_t, rows_q = iknp_restatement(seeds0, seeds1, delta, cb, m, ctr0)
    cu, rt, rq = gccpu.iknp_extend(seeds0, seeds1, delta.tobytes(), cb, m, ctr0)
    assert np.array_equal(U.reshape(-1), cu)
    assert np.array_equal(rows_t.reshape(-1), rt[:m * 16]) and np.array_equal(rows_q.reshape(-1), rq[:m * 16])
    y, ss, sr = iknp_gilboa_restatement(rows_t, rows_q, delta, a, b, w, tweak0)
    cy, css, csr = gccpu.iknp_gilboa(rt, rq, delta.tobytes(), a, b, w, tweak0)
    assert np.array_equal(y, cy) and np.array_equal(ss, css) and np.array_equal(sr, csr)
    for q in range(npairs):
        assert (int(ss[q]) + int(sr[q])) & mask == sum(int(x) * int(z) for x, z in zip(a[q], b[q])) & mask
