"""The half-payload form of the matrix Gilboa product (include/linreg_gc_ot_half.h), restated from the header's definitions on
helpers.iknp_restatement and ot_matrix_model.pads: OpenSSL and numpy, nothing of the product.

    OT i = (k r + ir) W + bit, c_i = bit `bit` of Xr[k][ir], M = rows r W; choice bits, extension and pads are the matrix mode's
    n_b = W - bit, m_b = 2^(n_b) - 1
    y'[i][j] = (x0 + Xs[k][j] - x1) & m_b,  share_s[ir][j] -= (x0 & m_b) << bit,
    share_r[ir][j] += ((pad(t_i)[j] + c_i y'[i][j]) & m_b) << bit                                       (sums mod 2^W)
    wire: H = W / 2 + 1 words per (k, ir, j): word 0 = y' of bit 0; word p (1 <= p < W / 2) = y' of bit p | y' of bit W - p << (W - p);
    word W / 2 = y' of bit W / 2; word ((k r + ir) H + p) s + j

All arithmetic is numpy uint64, which wraps mod 2^64; the masks bring it to the field widths."""
import numpy as np

import ot_matrix_model as om
from helpers import iknp_restatement


def words(w):
    """H: words of W bits per (k, ir, j)"""
    return w // 2 + 1


def y_bytes(rows, r, s, w):
    return rows * r * words(w) * s * w // 8


def field_masks(w):
    """(W,) uint64: m_b = 2^(W - bit) - 1 in Python integers, so no shift by W"""
    return np.array([(1 << (w - b)) - 1 for b in range(w)], dtype=np.uint64)


def pack(yp, w):
    """fields (G, W, s) uint64, yp[g, bit, j] < 2^(W - bit)  ->  words (G, H, s) uint32 / uint64"""
    yp = np.ascontiguousarray(yp, dtype=np.uint64)
    g, _, s = yp.shape
    out = np.zeros((g, words(w), s), dtype=np.uint64)
    out[:, 0] = yp[:, 0]
    for p in range(1, w // 2):
        out[:, p] = yp[:, p] | (yp[:, w - p] << np.uint64(w - p))
    out[:, w // 2] = yp[:, w // 2]
    return out.astype(np.uint32 if w == 32 else np.uint64)


def unpack(y, w):
    """words (G, H, s)  ->  fields (G, W, s) uint64"""
    y = np.ascontiguousarray(y).astype(np.uint64)
    g, _, s = y.shape
    m = field_masks(w)
    out = np.zeros((g, w, s), dtype=np.uint64)
    out[:, 0] = y[:, 0]
    for p in range(1, w // 2):
        out[:, p] = y[:, p] & m[p]
        out[:, w - p] = y[:, p] >> np.uint64(w - p)
    out[:, w // 2] = y[:, w // 2] & m[w // 2]
    return out


def payload(rows_t, rows_q, delta, xr, xs, w, tweak0):
    """the payload on given OT rows.  Returns (y (rows r H, s) uint32 / uint64, share_s (r, s) uint64, share_r (r, s) uint64)"""
    xr = np.ascontiguousarray(xr, dtype=np.uint64); xs = np.ascontiguousarray(xs, dtype=np.uint64)
    (rows, r), s = xr.shape, xs.shape[1]
    assert xs.shape[0] == rows
    m = om.ots(rows, r, w)
    delta = np.frombuffer(bytes(delta), dtype=np.uint8)
    x0 = om.pads(rows_q[:m], s, w, tweak0)
    x1 = om.pads(rows_q[:m] ^ delta[None, :], s, w, tweak0)
    pt = om.pads(rows_t[:m], s, w, tweak0)
    bit = np.tile(np.arange(w, dtype=np.uint64), rows * r)[:, None]                         # bit of OT i
    mb = np.tile(field_masks(w), rows * r)[:, None]                                         # m_b of OT i
    k = np.repeat(np.arange(rows), r * w)                                                   # row of OT i
    with np.errstate(over="ignore"):
        yp = (x0 + xs[k, :] - x1) & mb
        c = ((np.repeat(xr.ravel(), w)[:, None] >> bit) & np.uint64(1))
        ss = (np.uint64(0) - ((x0 & mb) << bit).reshape(rows, r, w, s).sum(axis=(0, 2), dtype=np.uint64)) & om.mask(w)
        sr = (((pt + c * yp) & mb) << bit).reshape(rows, r, w, s).sum(axis=(0, 2), dtype=np.uint64) & om.mask(w)
    return pack(yp.reshape(rows * r, w, s), w).reshape(rows * r * words(w), s), ss, sr


def run(seeds0, seeds1, delta, xr, xs, w, ctr0, tweak0):
    """one batch from the base-OT seeds.  Returns a dict with u (bytes, flat), y (packed), share_s, share_r and the counters after it"""
    rows, r = np.shape(xr)
    s = np.shape(xs)[1]
    m = om.ots(rows, r, w)
    U, rows_t, rows_q = iknp_restatement(seeds0, seeds1, delta, om.choice_bytes(xr, w), m, ctr0)
    y, ss, sr = payload(rows_t, rows_q, delta, xr, xs, w, tweak0)
    return {"u": U.reshape(-1), "y": y, "share_s": ss, "share_r": sr, "ctr": ctr0 + (m + 127) // 128, "tweak": tweak0 + m * om.nblk(s, w)}


def rows_per_batch(r, s, w):
    """as many whole rows as keep M <= 2^24 OTs and the half y <= 256 MiB, and at least one (host/ot_matrix_plan.c, otm_half_batch_rows)"""
    return max(min((1 << 24) // (r * w), (256 << 20) // y_bytes(1, r, s, w)), 1)


def batch_rows(n, r, s, w):
    """rows of every batch of an n-row block, as the host cuts them"""
    per = rows_per_batch(r, s, w)
    return [min(per, n - k) for k in range(0, n, per)]
