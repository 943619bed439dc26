"""Several target columns in one solve (include/linreg_gc_targets.h), on the CPU: the program of k right-hand sides is run
record by record on the CPU checker and every beta_t is compared with the oracle's single-target solve on (A, b_t).
No GPU needed."""
import zlib

import numpy as np
import pytest

from helpers import oracle_solve, split_shares, sx

OP_MAC, OP_DIV, OP_MACK = 1, 13, 20      # gc_exec.h


def _plain(gccpu, prog, sysm, shares):
    info = prog.info
    words = np.zeros(info.n_words, dtype=np.uint64)
    words[info.in_base:info.in_base + shares.size] = shares.ravel() & np.uint64((1 << sysm.width) - 1)
    dec = np.zeros(info.n_reveal + 1, dtype=np.uint64)
    steps, gates = gccpu.plain_run(prog.records(), info.n_records, sysm.width, sysm.precision, words, dec)
    assert steps == info.total_steps and gates == info.total_gates
    return dec


def _targets_system(oracle, rng, n, d, k, w, p):
    """one feature matrix, k outcomes: A (shared) and b_0 .. b_{k-1}, aggregated by the oracle"""
    X = rng.standard_normal((n, d)); X /= np.abs(X).max(axis=0)
    Xq = oracle.quantize(X, p, n, w)
    A0, bs = None, []
    for t in range(k):
        y = X @ rng.random(d) + 0.1 * rng.standard_normal(n)
        if t == k - 1 and k > 1:
            y = y[rng.permutation(n)]                       # a permuted copy, as a null-model target would be
        A, b = oracle.aggregate(Xq, oracle.quantize(y, p, n, w), n, d, p, w)
        if A0 is None:
            A0 = A
        assert np.array_equal(A, A0)
        bs.append(b)
    return A0, bs


def _same_program(a, b, lgc):
    assert a.records().tobytes() == b.records().tobytes()
    assert a.launches() == b.launches()
    for f, _ in lgc.ProgramInfo._fields_:
        assert getattr(a.info, f) == getattr(b.info, f), f


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 28)])
@pytest.mark.parametrize("alg", ["cgd", "cholesky", "ldlt"])
def test_every_target_matches_its_own_oracle_solve(lgc, gccpu, oracle, alg, w, p, normalize, k):
    rng = np.random.default_rng(zlib.crc32(("%s %d %d %d" % (alg, w, normalize, k)).encode()))
    d, n, iters, lam = 6, 40, 4, 0.001
    A, bs = _targets_system(oracle, rng, n, d, k, w, p)
    shares = split_shares(rng, A, np.concatenate(bs), 2, w)
    sysm = lgc.make_system(d, w, p, alg, iters, lam, 2, normalize, 1, 0)
    prog = lgc.Program(sysm, targets=k)
    info = prog.info
    T = d * (d + 1) // 2
    assert info.n_reveal >= T + k * d + k * d
    dec = _plain(gccpu, prog, sysm, shares)
    inputs = sx(dec[info.rv_inputs:info.rv_inputs + T + k * d], w)
    for t in range(k):
        exp, a, bb = oracle_solve(oracle, A, bs[t], d, w, p, alg, iters, lam, normalize)
        got = sx(dec[info.rv_beta + t * d:info.rv_beta + (t + 1) * d], w)
        assert got.tolist() == np.asarray(exp).tolist(), (alg, t)
        # reveal_inputs: A, then b_0 .. b_{k-1}
        assert inputs[:T].tolist() == sx(a, w).tolist()
        assert inputs[T + t * d:T + (t + 1) * d].tolist() == sx(bb, w).tolist()


@pytest.mark.parametrize("alg,d,w,normalize,reveal,trace", [
    ("cgd", 5, 64, 1, 1, 1), ("cgd", 100, 64, 1, 0, 0), ("cgd", 40, 32, 0, 1, 0),
    ("cholesky", 7, 32, 1, 1, 0), ("cholesky", 184, 64, 1, 0, 0), ("cholesky", 30, 64, 0, 0, 0),
    ("ldlt", 9, 64, 0, 1, 0), ("ldlt", 184, 64, 1, 0, 0), ("ldlt", 50, 32, 1, 0, 0),
])
def test_one_target_is_todays_program(lgc, alg, d, w, normalize, reveal, trace):
    """k = 1 lowers to the records, launches and info of lgc_program_build, byte for byte (Karatsuba sizes included)"""
    sysm = lgc.make_system(d, w, w - 8, alg, 3, 0.001, 2, normalize, reveal, trace)
    _same_program(lgc.Program(sysm), lgc.Program(sysm, targets=1), lgc)


@pytest.mark.parametrize("alg", ["cholesky", "ldlt"])
def test_factorisation_is_shared(lgc, gccpu, alg):
    """A is factored once: eight targets take the launches of one, and every added target costs the AND gates of its own
    substitutions and divisions (d (d - 1) products, 2d or d divisions) plus a few per cent for merging partial sums.
    (The whole program at d = 60 is 1.52 - 1.58 x the single one -- a target's own operations are 7 - 8 % of a solve that
    small; at d = 100 it is below 1.4 x.)"""
    mac = gccpu.rec_cost(OP_MAC, 1, 64, 56)[1]
    div = gccpu.rec_cost(OP_DIV, 1, 64, 56)[1]
    for d in (60, 100):
        sysm = lgc.make_system(d, 64, 56, alg, 0, 0.001, 2, 1, 0, 0)
        one, eight = lgc.Program(sysm), lgc.Program(sysm, targets=8)
        assert eight.info.n_launches == one.info.n_launches
        own = d * (d - 1) * mac + (2 * d if alg == "cholesky" else d) * div
        extra = (eight.info.total_gates - one.info.total_gates) / 7
        assert own <= extra < 1.05 * own, (d, extra / own)
        if d == 100:
            assert eight.info.total_gates < 1.5 * one.info.total_gates


def test_cholesky_karatsuba_size_matches_oracle(lgc, gccpu, oracle):
    """d = 184: the factorisation's dot products go through the Karatsuba circuit, whose shadow words now cover every y_t"""
    rng = np.random.default_rng(184)
    d, n, k, w, p = 184, 400, 2, 64, 56
    A, bs = _targets_system(oracle, rng, n, d, k, w, p)
    shares = split_shares(rng, A, np.concatenate(bs), 2, w)
    sysm = lgc.make_system(d, w, p, "cholesky", 0, 0.001, 2, 1, 0, 0)
    prog = lgc.Program(sysm, targets=k)
    recs = np.frombuffer(prog.records().tobytes(), dtype=np.uint32).reshape(-1, 10)
    assert (recs[:, 0] == OP_MACK).any()
    dec = _plain(gccpu, prog, sysm, shares)
    for t in range(k):
        exp, _, _ = oracle_solve(oracle, A, bs[t], d, w, p, "cholesky", 0, 0.001, 1)
        assert sx(dec[prog.info.rv_beta + t * d:prog.info.rv_beta + (t + 1) * d], w).tolist() == np.asarray(exp).tolist(), t


def test_rejections(lgc):
    sysm = lgc.make_system(4, 64, 56, "cgd", 2, 0.001, 2, 1, 0, 1)
    with pytest.raises(lgc.LgcError) as e:
        lgc.Program(sysm, targets=2)                                     # trace has one x per iteration
    assert e.value.code == -1
    lgc.Program(sysm, targets=1).close()                                 # ... which a single target still has
    plain = lgc.make_system(4, 64, 56, "cholesky", 0, 0.001, 2, 1, 0, 0)
    for k in (0, 257):
        with pytest.raises(lgc.LgcError) as e:
            lgc.Program(plain, targets=k)
        assert e.value.code == -1
    lgc.Program(plain, targets=256).close()
    with pytest.raises(lgc.LgcError) as e:
        lgc.Program(plain, lambdas=[0.1, 0.2], targets=2)
    assert e.value.code == -1
    with pytest.raises(lgc.LgcError) as e:                               # (the solver refuses before it looks for a GPU)
        lgc.Solver(plain, lambdas=[0.1, 0.2], targets=2)
    assert e.value.code == -1


def test_targets_header_is_exported_and_documented(lgc):
    import os
    import re
    root = os.path.join(os.path.dirname(__file__), "..")
    hdr = open(os.path.join(root, "include", "linreg_gc_targets.h")).read()
    names = set(re.findall(r"^[a-z][^\n(]*?\b(lgc_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    assert len(names) == 8, sorted(names)
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    for nme in names:
        assert hasattr(lgc.lib(), nme), nme
        assert nme in doc, nme
    base = open(os.path.join(root, "include", "linreg_gc.h")).read()
    assert not [n for n in names if n in base]                           # the drop-in header is unchanged
