"""The matrix-triple protocol of include/linreg_gc_p1_matrix.h restated in numpy uint64 and Python integers: nothing of the
product.  Keystreams come from helpers.openssl_aes_ctr (OpenSSL), matrices are row-major, a wire word is W bits little-endian.

  R_a (n x a) <- seed_a, R_b (n x b) <- seed_b, S (a x b) <- seed_s: word k * cols + i of a stream is entry [k][i]
  T = (R_a^T R_b - S) & m         E = (X_a - R_a) & m         F = (X_b - R_b) & m
  share_a = (R_a^T F + S) & m     share_b = (E^T X_b + T) & m
  share_a + share_b = X_a^T X_b mod 2^W
"""
import numpy as np

from helpers import openssl_aes_ctr


def mask(w):
    return (1 << w) - 1


def stream(seed, rows, cols, w):
    """rows x cols keystream words of W bits (uint64), from block 0 of AES-128-CTR under `seed`"""
    nbytes = rows * cols * (w // 8)
    ks = openssl_aes_ctr(seed, 0, (nbytes + 15) // 16)[:nbytes]
    return np.frombuffer(ks.tobytes(), dtype="<u4" if w == 32 else "<u8").astype(np.uint64).reshape(rows, cols)


def seeds(master, u):
    """(seed_a, seed_b, seed_s) of instance u: blocks 3u, 3u + 1, 3u + 2 of the master seed's keystream"""
    ks = openssl_aes_ctr(master, 3 * u, 3).tobytes()
    return ks[0:16], ks[16:32], ks[32:48]


def tmul_int(P, Q, w):
    """P^T Q mod 2^W in Python integers: no wrap-around is relied upon"""
    r = np.array(P.astype(object).T @ Q.astype(object), dtype=object) & mask(w)
    return np.array(r, dtype=object).astype(np.uint64)


def tmul(P, Q, w):
    """P^T Q mod 2^W in numpy uint64, whose products and sums wrap mod 2^64 (tests/test_ti_matrix_cpu.py holds it against
    tmul_int)"""
    with np.errstate(over="ignore"):
        return (P.astype(np.uint64).T @ Q.astype(np.uint64)) & np.uint64(mask(w))


def columns(Xq, yq, cols):
    """the n x len(cols) block of [X | y] as words mod 2^64 (column d is y)"""
    full = np.column_stack([Xq, yq]) if yq is not None else Xq
    return np.ascontiguousarray(full[:, list(cols)]).astype(np.int64).view(np.uint64)


def run(Xa, Xb, seed_a, seed_b, seed_s, w, mul=tmul):
    """every message and both shares for the blocks Xa (n x a) and Xb (n x b), given as uint64 words; mul: tmul or tmul_int.
    Returns a dict of uint64 arrays: Ra, Rb, S, T, E, F, share_a, share_b"""
    n, a = Xa.shape
    b = Xb.shape[1]
    m = np.uint64(mask(w))
    Ra, Rb, S = stream(seed_a, n, a, w), stream(seed_b, n, b, w), stream(seed_s, a, b, w)
    with np.errstate(over="ignore"):
        T = (mul(Ra, Rb, w) - S) & m
        E = (Xa - Ra) & m
        F = (Xb - Rb) & m
        share_a = (mul(Ra, F, w) + S) & m
        share_b = (mul(E, Xb & m, w) + T) & m
    return dict(Ra=Ra, Rb=Rb, S=S, T=T, E=E, F=F, share_a=share_a, share_b=share_b)


def gram_block(Xa, Xb, w, mul=tmul):
    """X_a^T X_b mod 2^W, the integer Gram block the shares must sum to"""
    return mul(Xa, Xb, w)
