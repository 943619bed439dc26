"""The trusted initializer's AES-128-CTR stream (ti_prg_kernel, ti_unpack_kernel, ti_unpack_scatter_kernel and the p1_dot
kernels that lgc_ti_generate / lgc_ti_generate_scatter run, csrc/phase1.hip) word for word at every stream offset and
second trip.

The stream masks private columns, and every party derives the same words from the same seed: a batch that resumes at the
wrong offset, or a grid-stride trip that restarts at the first trip's position, reuses keystream without any share-level
check noticing.  Every comparison here is np.array_equal against two references: the CPU mirror's AES-NI stream
(gccpu.ti_stream_words) and the same words cut from OpenSSL's (helpers.openssl_aes_ctr).  xy_minus_r is recomputed in
Python integers.

Word t of pair q is stream word q (2n + 1) + t (x, then y, then r), w / 8 bytes each, in 16-byte counter blocks.  Launch
geometry of ti_generate (phase1.hip), named by the shapes below:
    512 x 1024    ti_prg_kernel: 524 288 blocks per trip
    1024 x 256    ti_unpack_kernel: 262 144 words per trip
    64 x 256      p1_dot_kernel: gx = min(ceil(n / 256), 64), 16 384 elements per trip
    128 x 256     ti_unpack_scatter_kernel: gx = min(ceil((2n + 1) / 256), 128), 32 768 words of a pair per trip"""
import ctypes as C

import numpy as np
import pytest

from helpers import openssl_aes_ctr

pytestmark = pytest.mark.gpu

SEED = bytes(range(101, 117))


def _openssl_words(seed, first_word, nwords, w):
    """words [first_word, first_word + nwords) of the stream, cut from OpenSSL's keystream (own arithmetic: byte offsets)"""
    wb = w // 8
    byte0, byte1 = first_word * wb, (first_word + nwords) * wb
    blk0 = byte0 // 16
    ks = openssl_aes_ctr(seed, blk0, (byte1 + 15) // 16 - blk0)
    raw = ks[byte0 - 16 * blk0:byte1 - 16 * blk0]
    return np.frombuffer(raw.tobytes(), dtype="<u8" if w == 64 else "<u4").astype(np.uint64)


def _xy_minus_r(x, y, r, w):
    mask = (1 << w) - 1
    return [(sum(a * b for a, b in zip(xq, yq)) - rq) & mask for xq, yq, rq in zip(x.tolist(), y.tolist(), r.tolist())]


@pytest.mark.parametrize("w,first_pair,npairs,n", [
    (64, 1, 1, 1),             # byte0 = 24: skip = 8 inside the first counter block
    (32, 3, 2, 5),             # byte0 = 3 * 11 * 4 = 132: skip = 4
    (32, 1, 1, 1),             # byte0 = 12: skip = 12
    (32, 7, 5, 257),           # n one past the 256-lane workgroup of p1_dot_kernel; skip = 4
    # 33 * 32 771 = 1 081 443 words = 540 722 blocks > 512 x 1024: a second ti_prg_kernel trip; five trips of
    # ti_unpack_kernel (1024 x 256); n = 16 385 = 64 x 256 + 1: a second p1_dot_kernel trip with a lone element
    (64, 7, 33, 16385),
    (32, 9, 17, 16385),        # the same n at w = 32: 557 107 words, three ti_unpack_kernel trips, skip = 12
])
def test_ti_generate_matches_both_streams(lgc, gccpu, w, first_pair, npairs, n):
    per = 2 * n + 1
    x, y, r, xyr = lgc.ti_generate(SEED, first_pair, npairs, n, w)
    for words in (gccpu.ti_stream_words(SEED, first_pair * per, npairs * per, w), _openssl_words(SEED, first_pair * per, npairs * per, w)):
        words = words.reshape(npairs, per)
        assert np.array_equal(x, words[:, :n])
        assert np.array_equal(y, words[:, n:2 * n])
        assert np.array_equal(r, words[:, 2 * n])
    assert xyr.tolist() == _xy_minus_r(x, y, r, w)


def test_ti_batches_tile_the_stream(lgc):
    """generate(0, a) then generate(a, b) equals generate(0, a + b) word for word: batches neither overlap nor leave a gap.
    w = 32 and odd a, n: the second batch starts at byte 3 * 11 * 4 = 132, inside a counter block"""
    w, n, a, b = 32, 5, 3, 4
    whole = lgc.ti_generate(SEED, 0, a + b, n, w)
    head = lgc.ti_generate(SEED, 0, a, n, w)
    tail = lgc.ti_generate(SEED, a, b, n, w)
    for full, h, t in zip(whole, head, tail):
        assert np.array_equal(np.concatenate([h, t]), full)
    # and the whole is the stream itself: x, y, r of consecutive pairs are consecutive words
    stream = np.concatenate([np.concatenate([whole[0][q], whole[1][q], whole[2][q:q + 1]]) for q in range(a + b)])
    assert np.array_equal(stream, _openssl_words(SEED, 0, (a + b) * (2 * n + 1), w))


@pytest.mark.parametrize("w,first_pair,npairs,n", [
    (64, 2, 3, 5),
    (32, 4, 3, 6),             # even first_pair: the batch's byte offset 4 * 13 * 4 = 208 is a multiple of 16
    (64, 1, 3, 16400),         # 2n + 1 = 32 801 > 128 x 256: a second trip of ti_unpack_scatter_kernel; n > 64 x 256: of p1_dot_ptr_kernel
])
def test_ti_generate_scatter_matches_generate(lgc, w, first_pair, npairs, n):
    """lgc_ti_generate_scatter (x[q] / y[q] written to per-pair device buffers, the --ti_ring path of the host) against
    lgc_ti_generate for the same arguments"""
    L = lgc.lib()
    for f, a in (("lgc_dev_alloc", [C.c_int, C.c_size_t, C.POINTER(C.c_void_p), C.c_void_p]), ("lgc_dev_upload", [C.c_void_p, C.c_void_p, C.c_size_t]),
                 ("lgc_dev_download", [C.c_void_p, C.c_void_p, C.c_size_t]),
                 ("lgc_ti_generate_scatter", [C.c_int, C.c_char_p, C.c_uint64, C.c_size_t, C.c_size_t, C.c_int] + [C.c_void_p] * 4)):
        getattr(L, f).argtypes = a; getattr(L, f).restype = C.c_int
    L.lgc_dev_free.argtypes = [C.c_void_p]; L.lgc_dev_free.restype = None
    x, y, r, xyr = lgc.ti_generate(SEED, first_pair, npairs, n, w)
    bufs = []
    try:
        for _ in range(2 * npairs):
            ptr = C.c_void_p()
            assert L.lgc_dev_alloc(0, n * 8, C.byref(ptr), None) == 0
            bufs.append(ptr)
        xdst = (C.c_void_p * npairs)(*[p.value for p in bufs[:npairs]])
        ydst = (C.c_void_p * npairs)(*[p.value for p in bufs[npairs:]])
        gr = np.zeros(npairs, dtype=np.uint64); gxyr = np.zeros(npairs, dtype=np.uint64)
        assert L.lgc_ti_generate_scatter(0, SEED, first_pair, npairs, n, w, xdst, ydst, gr.ctypes.data_as(C.c_void_p),
                                         gxyr.ctypes.data_as(C.c_void_p)) == 0, L.lgc_last_error()
        gx = np.zeros((npairs, n), dtype=np.uint64); gy = np.zeros((npairs, n), dtype=np.uint64)
        for q in range(npairs):
            assert L.lgc_dev_download(gx[q].ctypes.data_as(C.c_void_p), bufs[q], n * 8) == 0
            assert L.lgc_dev_download(gy[q].ctypes.data_as(C.c_void_p), bufs[npairs + q], n * 8) == 0
    finally:
        for ptr in bufs:
            L.lgc_dev_free(ptr)
    assert np.array_equal(gx, x) and np.array_equal(gy, y)
    assert np.array_equal(gr, r) and np.array_equal(gxyr, xyr)
    assert xyr.tolist() == _xy_minus_r(x, y, r, w)
