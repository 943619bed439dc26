"""The inputs of test_p1_diag_gpu.py and their reference words, shared with test_p1_model_cpu.py, which proves on a CPU what the
GPU tests rely on: the w = 64 in-range words depend on the order of the additions, no in-range word is the saturated word, and
every word of the saturating inputs is.  A matrix depends on (n, d, w) alone, and every reference is computed once per process."""
import functools

import numpy as np

import p1_model

WIDTHS = [(64, 56), (32, 28)]
PREC = dict(WIDTHS)
SEED = 1

# c0 = 1, own = 17, d = 19: a column before and one behind the block, two workgroups of p1_diag_kernel (16 columns + 1)
C0, OWN, D = 1, 17, 19
# 59, 60, 61: the loader's row phase r0 + 60 u; 599, 600, 601: a full chunk of 600 rows, a second chunk of one row;
# 1200, 1201: two full chunks, a third of one row in the LDS buffer the first one used; 1801: a fourth, in the second one's
ROWS = [1, 59, 60, 61, 599, 600, 601, 1200, 1201, 1801]
# at n = 601: 16 and 17 cross the 16 columns of a workgroup, 33 makes a third one
OWNS = [1, 15, 16, 17, 33]
OWNS_N = 601
# K = 2 folds of 1201 rows are rows [0, 600) and [600, 1201)
FOLDS_N, FOLDS = 1201, [(0, 600), (600, 1201)]
# the divisor cases: at w = 32 the sum of n squares below 2^24 stays below 2^31 undivided while n < 128
DIVISORS_N = 61
SAT_N = 601

# n = 1, divisor 1: the word is x^2 while that is below 2^(w-1).  (width, x, word)
BOUNDARY = [
    (32, 46340, 0x7ffea810), (32, 46341, 0x80000000), (32, -46341, 0x80000000),
    (64, 3037000499, 0x7ffffffe9ea1dc00), (64, 3037000500, 0x8000000000000000),
]


@functools.lru_cache(maxsize=None)
def in_range(n, d, w):
    """|x| < 2^27 at w = 64 (p = 56): a square has up to 54 bits and the running sum more, so every addition rounds;
    |x| < 2^12 at w = 32 (p = 28)"""
    b = 1 << (27 if w == 64 else 12)
    X = np.random.default_rng([SEED, n, d, w]).integers(-b + 1, b, (n, d), dtype=np.int64)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def full_range(n, d, w):
    """every word of the width, sign-extended: a sum of squares over the divisor is far beyond 2^(w-1)"""
    X = np.random.default_rng([SEED + 1, n, d, w]).integers(-(1 << (w - 1)), 1 << (w - 1), (n, d), dtype=np.int64)
    X.setflags(write=False)
    return X


def boundary(w):
    """(the 1 x k matrix of the boundary inputs of width w, their words)"""
    rows = [(x, word) for ww, x, word in BOUNDARY if ww == w]
    return np.array([[x for x, _ in rows]], dtype=np.int64), [word for _, word in rows]


@functools.lru_cache(maxsize=None)
def words(kind, n, d, w, c0, c1, divisor, r0=0, r1=None):
    """the reference words of columns [c0, c1) over rows [r0, r1) of in_range / full_range (n, d, w)"""
    X = {"in_range": in_range, "full_range": full_range}[kind](n, d, w)
    return tuple(p1_model.diag_words(X[r0:r1], c0, c1, PREC[w], w, divisor))


def in_range_cases():
    """every (n, d, w, c0, c1, divisor, r0, r1) whose in-range reference words test_p1_diag_gpu.py asks for"""
    out = []
    for w, _ in WIDTHS:
        out += [(n, D, w, C0, C0 + OWN, D, 0, n) for n in ROWS]
        out += [(OWNS_N, own + 2, w, C0, C0 + own, own + 2, 0, OWNS_N) for own in OWNS]
        out += [(FOLDS_N, D, w, C0, C0 + OWN, D, r0, r1) for r0, r1 in FOLDS]
        out += [(DIVISORS_N, D, w, C0, C0 + OWN, v, 0, DIVISORS_N) for v in (1, 7, D)]
    return out
