"""Gilboa on a whole block with one vector OT per operand bit (include/linreg_gc_ot_matrix.h), restated from the header's
definitions on helpers.iknp_restatement and helpers.openssl_gate_hash_fast: OpenSSL and numpy, nothing of the product.

    OT i = (k r + ir) W + bit, c_i = bit `bit` of Xr[k][ir], M = rows r W
    nblk = ceil(s W / 128); block c of OT i is H(row_i, tweak0 + i nblk + c); its 16 bytes are 128 / W little-endian words,
    word e of block c is sender column j = c (128 / W) + e, words with j >= s are dropped
    y[i][j] = x0 + (Xs[k][j] << bit) - x1,  share_s[ir][j] = -sum x0,  share_r[ir][j] = sum pad(t_i)[j] + c_i y[i][j]   (mod 2^W)

All arithmetic is numpy uint64, which wraps mod 2^64; the mask brings it to W bits."""
import numpy as np

from helpers import iknp_restatement, openssl_gate_hash_fast


def mask(w):
    return np.uint64((1 << w) - 1)


def nblk(s, w):
    return (s * w + 127) // 128


def ots(rows, r, w):
    return rows * r * w


def choice_bytes(xr, w):
    """the M choice bits packed LSB-first: the dense rows x r block, W bits per word"""
    xr = np.ascontiguousarray(xr, dtype=np.uint64)
    return xr.view(np.uint8).ravel() if w == 64 else xr.astype(np.uint32).view(np.uint8).ravel()


def pads(rows128, s, w, tweak0):
    """(M, s) uint64: the pad words of every OT row (M, 16) uint8"""
    m, nb = len(rows128), nblk(s, w)
    tweaks = (np.uint64(tweak0) + np.arange(m, dtype=np.uint64)[:, None] * np.uint64(nb) + np.arange(nb, dtype=np.uint64)[None, :]).ravel()
    h = openssl_gate_hash_fast(np.repeat(np.ascontiguousarray(rows128, dtype=np.uint8), nb, axis=0), tweaks)     # (M nblk, 16)
    words = np.ascontiguousarray(h).view("<u8" if w == 64 else "<u4").reshape(m, nb * (128 // w))
    return words[:, :s].astype(np.uint64)


def payload(rows_t, rows_q, delta, xr, xs, w, tweak0):
    """the payload on given OT rows.  Returns (y (M, s) uint32 / uint64, share_s (r, s) uint64, share_r (r, s) uint64)"""
    xr = np.ascontiguousarray(xr, dtype=np.uint64); xs = np.ascontiguousarray(xs, dtype=np.uint64)
    (rows, r), s = xr.shape, xs.shape[1]
    assert xs.shape[0] == rows
    m = ots(rows, r, w)
    delta = np.frombuffer(bytes(delta), dtype=np.uint8)
    x0 = pads(rows_q[:m], s, w, tweak0)
    x1 = pads(rows_q[:m] ^ delta[None, :], s, w, tweak0)
    pt = pads(rows_t[:m], s, w, tweak0)
    bit = np.tile(np.arange(w, dtype=np.uint64), rows * r)                                  # bit of OT i
    k = np.repeat(np.arange(rows), r * w)                                                   # row of OT i
    with np.errstate(over="ignore"):
        y = (x0 + (xs[k, :] << bit[:, None]) - x1) & mask(w)
        c = ((np.repeat(xr.ravel(), w) >> bit) & np.uint64(1))[:, None]
        # sum over (k, bit) for every ir: OT i is [k][ir][bit]
        ss = (np.uint64(0) - x0.reshape(rows, r, w, s).sum(axis=(0, 2), dtype=np.uint64)) & mask(w)
        sr = (pt + c * y).reshape(rows, r, w, s).sum(axis=(0, 2), dtype=np.uint64) & mask(w)
    return y.astype(np.uint32 if w == 32 else np.uint64), ss, sr


def run(seeds0, seeds1, delta, xr, xs, w, ctr0, tweak0):
    """one batch from the base-OT seeds.  Returns a dict with u (bytes, flat), y, share_s, share_r and the counters after it"""
    rows, r = np.shape(xr)
    s = np.shape(xs)[1]
    m = ots(rows, r, w)
    U, rows_t, rows_q = iknp_restatement(seeds0, seeds1, delta, choice_bytes(xr, w), m, ctr0)
    y, ss, sr = payload(rows_t, rows_q, delta, xr, xs, w, tweak0)
    return {"u": U.reshape(-1), "y": y, "share_s": ss, "share_r": sr, "ctr": ctr0 + (m + 127) // 128, "tweak": tweak0 + m * nblk(s, w)}


def product(xr, xs, w):
    """(Xr^T Xs) mod 2^W in wrapping uint64"""
    with np.errstate(over="ignore"):
        return (np.ascontiguousarray(xr, dtype=np.uint64).T @ np.ascontiguousarray(xs, dtype=np.uint64)) & mask(w)


def product_int(xr, xs, w):
    """(Xr^T Xs) mod 2^W in Python integers"""
    xr = np.asarray(xr, dtype=np.uint64).tolist(); xs = np.asarray(xs, dtype=np.uint64).tolist()
    r, s = len(xr[0]), len(xs[0])
    return np.array([[sum(a[i] * b[j] for a, b in zip(xr, xs)) & ((1 << w) - 1) for j in range(s)] for i in range(r)], dtype=np.uint64)


def rows_per_batch(r, s, w):
    """as many whole rows as keep M <= 2^24 OTs and y <= 256 MiB, and at least one (host/ot_matrix_plan.c, otm_batch_rows)"""
    return max(min((1 << 24) // (r * w), (256 << 20) // (r * w * s * (w // 8))), 1)


def batch_rows(n, r, s, w):
    """rows of every batch of an n-row block, as the host cuts them"""
    per = rows_per_batch(r, s, w)
    return [min(per, n - k) for k in range(0, n, per)]
