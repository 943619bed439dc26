"""In-circuit model selection of a lasso path on a hold-out (include/linreg_gc_lasso_select.h) on the CPU: the lowered program,
run record by record by the CPU checker and garbled + evaluated by its CPU backends, against the independent model of
tests/lasso_select_model.py; beta* against the plain path program; inputs whose selection is not trivial; the three record
variants alone on edge operands; the structure of the lowering; the rejections.  No GPU needed."""
import ctypes as C
import math
import os
import re
import zlib

import numpy as np
import pytest

import lasso_select_model as lsm
import linreg_gc
import op_corpus as oc
import word_model as wm
from helpers import split_shares, sx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OP_SUM, OP_MAX, OP_REVEAL, OP_MACK, OP_HDIFF, OP_EQ, OP_PROX = 2, 12, 18, 20, 21, 22, 26          # gc_exec.h
INF = math.inf
INDEX, SCORES = lsm.REVEAL_INDEX, lsm.REVEAL_SCORES
FLAGS = (0, INDEX, INDEX | SCORES)
# L values each, listed out of order so that the best one is not at an end; ratios of lambda_max lie in [0, 2]
VALUES = {lsm.ABSOLUTE: [0.3, 0.05, 0.0005, 0.01, 0.1, 0.002, 0.02, 0.2, 0.005],
          lsm.RATIO: [1.5, 0.5, 0.01, 0.1, 0.8, 0.03, 0.2, 1.0, 0.05]}


def _recs(prog):
    return np.frombuffer(prog.records().tobytes(), dtype=np.uint32).reshape(-1, 10)


def two_systems(oracle, rng, d, w, p, n=None, n_val=None, sigma=0.1, scale_v=1.0):
    """(A, b, A_v, b_v) as words: a training and a validation system from rows of ONE planted model, A = X^T X / (n d) packed
    as the lower triangle row by row, b = X^T y / (n d) (positive semi-definite as the circuit reads it, entries well inside
    the range at either width); scale_v scales the validation targets"""
    n = n or 3 * d + 20
    n_val = n_val or 2 * d + 10
    beta = rng.random(d) * (rng.random(d) < 0.6)
    m = (1 << w) - 1
    out = []
    for rows, s in ((n, 1.0), (n_val, scale_v)):
        X = rng.standard_normal((rows, d)); X /= np.abs(X).max(axis=0)
        y = (X @ beta + sigma * rng.standard_normal(rows)) * s
        M, v = X.T @ X / (rows * d), X.T @ y / (rows * d)
        out.append(np.array([int(M[i][j] * 2.0 ** p) & m for i in range(d) for j in range(i + 1)], dtype=np.uint64))
        out.append(np.array([int(x * 2.0 ** p) & m for x in v], dtype=np.uint64))
    return out


def joined_shares(rng, A, b, Av, bv, nshares, w):
    """shares of [A, b, A_v, b_v]: (nshares, 2 (T + d)); returns them with the training and the validation halves"""
    tr, va = split_shares(rng, A, b, nshares, w), split_shares(rng, Av, bv, nshares, w)
    return np.ascontiguousarray(np.hstack([tr, va])), tr, va


def train_inputs(oracle, A, b, d, w, p, lam, normalize):
    a = oracle.sum_shares(np.asarray(A, dtype=np.uint64)[None, :], w)
    bb = oracle.sum_shares(np.asarray(b, dtype=np.uint64)[None, :], w)
    if normalize:
        a, bb = oracle.circuit_input(a, bb, d, lam, p, w)
    return sx(a, w).tolist(), sx(bb, w).tolist()


def plain(gccpu, prog, w, p, shares):
    info = prog.info
    words = np.zeros(info.n_words, dtype=np.uint64)
    words[info.in_base:info.in_base + shares.size] = shares.ravel() & np.uint64((1 << w) - 1)
    dec = np.zeros(info.n_reveal + 1, dtype=np.uint64)
    steps, gates = gccpu.plain_run(prog.records(), info.n_records, w, p, words, dec)
    assert steps == info.total_steps and gates == info.total_gates
    return dec


def shown(prog, dec, w, flags, L):
    """the words the program reveals from rv_beta: beta*, [l*], [scores]"""
    n = prog.system.d + (1 if flags & INDEX else 0) + (L if flags & SCORES else 0)
    assert prog.info.n_reveal == prog.info.rv_beta + n
    return sx(dec[prog.info.rv_beta:prog.info.rv_beta + n], w).tolist()


def options(d):
    kinds = [(-INF, INF), (0.0, INF), (-INF, 0.3), (-0.02, 0.4)]
    return dict(penalty_factors=[(1.0, 0.5, 2.0, 0.0)[i % 4] for i in range(d)], lower=[kinds[i % 4][0] for i in range(d)],
                upper=[kinds[i % 4][1] for i in range(d)])


def program(lgc, sysm, values, mode, flags, **kw):
    key = "l1" if mode == lsm.ABSOLUTE else "l1_ratios"
    return lgc.Program(sysm, validation=True, reveal_index=bool(flags & INDEX), reveal_scores=bool(flags & SCORES),
                       **dict(kw, **{key: list(values)}))


@pytest.mark.parametrize("L", [1, 2, 3, 9])
@pytest.mark.parametrize("d", [1, 5, 12])
@pytest.mark.parametrize("mode", [lsm.ABSOLUTE, lsm.RATIO])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_program_reveals_the_model(lgc, gccpu, oracle, w, p, normalize, mode, d, L):
    """every revealed word of the lowered program, run record by record, is the model's: both widths, both input paths, both
    modes, with and without factors / bounds, the three reveal combinations"""
    rng = np.random.default_rng(zlib.crc32(("select %d %d %d %d %d" % (w, normalize, mode, d, L)).encode()))
    N, lam = 8, 0.05
    A, b, Av, bv = two_systems(oracle, rng, d, w, p)
    shares, _, va = joined_shares(rng, A, b, Av, bv, 2, w)
    values = VALUES[mode][:L]
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, normalize, 0, 0)
    a, bb = train_inputs(oracle, A, b, d, w, p, lam, normalize)
    for k, flags in enumerate(FLAGS):
        kw = options(d) if (k + d + L) % 2 else {}
        prog = program(lgc, sysm, values, mode, flags, **kw)
        best, idx, scores, _ = lsm.lasso_select(a, bb, va, d, w, p, N, values, mode, normalize, kw.get("penalty_factors"),
                                                kw.get("lower"), kw.get("upper"))
        assert shown(prog, plain(gccpu, prog, w, p, shares), w, flags, L) == lsm.revealed(best, idx, scores, flags)
    # scores alone
    prog = program(lgc, sysm, values, mode, SCORES)
    best, idx, scores, _ = lsm.lasso_select(a, bb, va, d, w, p, N, values, mode, normalize)
    assert shown(prog, plain(gccpu, prog, w, p, shares), w, SCORES, L) == lsm.revealed(best, idx, scores, SCORES)


@pytest.mark.parametrize("d,L", [(1, 2), (5, 3), (5, 9)])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_cpu_garble_evaluate_gives_the_model(lgc, gccpu, oracle, w, p, d, L):
    rng = np.random.default_rng(zlib.crc32(("select ge %d %d %d" % (w, d, L)).encode()))
    N, lam, flags = 4, 0.05, INDEX | SCORES
    A, b, Av, bv = two_systems(oracle, rng, d, w, p)
    shares, _, va = joined_shares(rng, A, b, Av, bv, 2, w)
    values = VALUES[lsm.RATIO][:L]
    kw = options(d)
    prog = program(lgc, lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0), values, lsm.RATIO, flags, **kw)
    dec, gates, _ = gccpu.garble_eval(prog, shares)
    assert gates == prog.info.total_gates
    a, bb = train_inputs(oracle, A, b, d, w, p, lam, 1)
    best, idx, scores, _ = lsm.lasso_select(a, bb, va, d, w, p, N, values, lsm.RATIO, 1, kw["penalty_factors"], kw["lower"], kw["upper"])
    assert shown(prog, dec, w, flags, L) == lsm.revealed(best, idx, scores, flags)


@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_beta_star_is_a_row_of_the_plain_path(lgc, gccpu, oracle, w, p):
    """beta* is row l* of the existing path program's beta on the training inputs alone, bit for bit, and l* is the first
    argmin (signed) of the revealed scores"""
    d, L, N, lam = 7, 6, 8, 0.05
    rng = np.random.default_rng(zlib.crc32(("row %d" % w).encode()))
    A, b, Av, bv = two_systems(oracle, rng, d, w, p)
    shares, tr, _ = joined_shares(rng, A, b, Av, bv, 2, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0)
    values = VALUES[lsm.RATIO][:L]
    sel = program(lgc, sysm, values, lsm.RATIO, INDEX | SCORES)
    got = shown(sel, plain(gccpu, sel, w, p, shares), w, INDEX | SCORES, L)
    path = lgc.Program(sysm, l1_ratios=values)
    rows = sx(plain(gccpu, path, w, p, tr)[path.info.rv_beta:path.info.rv_beta + L * d], w).reshape(L, d).tolist()
    idx, scores = got[d], got[d + 1:]
    assert idx == lsm.argmin_first(scores) and got[:d] == rows[idx]
    assert len({tuple(r) for r in rows}) >= 4 and any(rows[idx])   # (the models differ: picking a row means something)


def test_interior_winner_and_negative_scores(lgc, gccpu, oracle):
    """a validation system of the training rows' model: the scores are negative and the best value is the small lambda1
    listed in the middle"""
    w, p, d, N, lam = 64, 56, 6, 8, 0.01
    rng = np.random.default_rng(77)
    A, b, Av, bv = two_systems(oracle, rng, d, w, p, n=200, n_val=150)
    shares, _, va = joined_shares(rng, A, b, Av, bv, 2, w)
    values = [0.9, 0.01, 0.4]                                  # ratios of lambda_max
    prog = program(lgc, lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0), values, lsm.RATIO, INDEX | SCORES)
    a, bb = train_inputs(oracle, A, b, d, w, p, lam, 1)
    best, idx, scores, betas = lsm.lasso_select(a, bb, va, d, w, p, N, values, lsm.RATIO, 1)
    assert idx == 1 and min(scores) < 0 and len(set(scores)) == 3
    assert shown(prog, plain(gccpu, prog, w, p, shares), w, INDEX | SCORES, 3) == lsm.revealed(best, idx, scores, INDEX | SCORES)


@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_zero_b_v_gives_scores_of_the_other_sign(lgc, gccpu, oracle, w, p):
    """b_v = 0: score_l = beta^T M_v beta >= 0, so the most shrunk model wins; with the targets of the validation rows
    scaled by 8 instead the scores are negative and large"""
    d, N, lam = 5, 8, 0.05
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, 0, 0, 0)
    for case in ("zero", "large"):
        values = [0.1, 1.5, 0.01, 0.5] if case == "zero" else [0.1, 0.05, 0.01, 0.3]   # ratios (large: no model is all zero)
        rng = np.random.default_rng(zlib.crc32(("sign %d" % w).encode()))
        A, b, Av, bv = two_systems(oracle, rng, d, w, p, scale_v=1.0 if case == "zero" else 8.0)
        if case == "zero":
            bv = np.zeros_like(bv)
        shares, _, va = joined_shares(rng, A, b, Av, bv, 2, w)
        prog = program(lgc, sysm, values, lsm.RATIO, INDEX | SCORES)
        a, bb = train_inputs(oracle, A, b, d, w, p, lam, 0)
        best, idx, scores, _ = lsm.lasso_select(a, bb, va, d, w, p, N, values, lsm.RATIO, 0)
        assert shown(prog, plain(gccpu, prog, w, p, shares), w, INDEX | SCORES, 4) == lsm.revealed(best, idx, scores, INDEX | SCORES)
        if case == "zero":
            assert min(scores) == scores[1] == 0 and max(scores) > 0 and idx == scores.index(0) and not any(best)
        else:
            assert max(scores) < 0 and len(set(scores)) == 4


@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_ties_go_to_the_first_value(lgc, gccpu, oracle, w, p):
    """an all-zero validation system makes every score 0: l* = 0; a value listed twice ties with itself: the first wins"""
    d, N, lam = 5, 8, 0.05
    rng = np.random.default_rng(zlib.crc32(("ties %d" % w).encode()))
    A, b, Av, bv = two_systems(oracle, rng, d, w, p)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0)
    a, bb = train_inputs(oracle, A, b, d, w, p, lam, 1)
    for values, zero, want in (([0.1, 0.002, 0.02], True, 0), ([0.3, 0.002, 0.002, 0.1, 0.002], False, 1)):
        L = len(values)
        shares, _, va = joined_shares(rng, A, b, np.zeros_like(Av) if zero else Av, np.zeros_like(bv) if zero else bv, 2, w)
        prog = program(lgc, sysm, values, lsm.ABSOLUTE, INDEX | SCORES)
        best, idx, scores, _ = lsm.lasso_select(a, bb, va, d, w, p, N, values, lsm.ABSOLUTE, 1)
        assert idx == want and scores.count(min(scores)) >= 3 and (not zero or scores == [0] * L)
        assert shown(prog, plain(gccpu, prog, w, p, shares), w, INDEX | SCORES, L) == lsm.revealed(best, idx, scores, INDEX | SCORES)
        dec, gates, _ = gccpu.garble_eval(prog, shares)
        assert gates == prog.info.total_gates and shown(prog, dec, w, INDEX | SCORES, L) == lsm.revealed(best, idx, scores, INDEX | SCORES)


# ---- the three record variants alone
def _mismatches(C, got, want):
    m = wm.mask(C.w)
    return ["word %d (%s): got 0x%x, expected 0x%x" % (i, C.desc.get(i, "input"), int(got[i]) & m, want[i])
            for i in range(len(want)) if int(got[i]) & m != want[i]][:8]


@pytest.mark.parametrize("w", [64, 32])
def test_variants_plain(gccpu, w):
    for p in (1, w - 8):
        Cp = lsm.select_corpus(w, p, np.random.default_rng([w, p]))
        prog = Cp.program(linreg_gc, lambda kind: ("auto", "auto"))
        bad = _mismatches(Cp, oc.plain_words(gccpu, prog, Cp), lsm.corpus_words(Cp))
        assert not bad, (w, p, bad)


@pytest.mark.parametrize("w", [64, 32])
def test_variants_garbled(gccpu, w):
    """garble + evaluate of the whole corpus, cnt = 256 included: the index wiring for k >= 128, the one-hot chain over 256
    candidates and a 256-way gated select, with the gate count of the lowered records"""
    Cp = lsm.select_corpus(w, w - 8, np.random.default_rng([w, 1]))
    assert {r[1] for r in Cp.launches[1][1]} == set(lsm.CNTS) and any(lsm.corpus_words(Cp)[r[5]] >= 128 for r in Cp.launches[1][1])
    prog = Cp.program(linreg_gc, lambda kind: ("auto", "auto"))
    got, gates, _ = gccpu.garble_eval(prog, np.array(Cp.inputs, dtype=np.uint64))
    assert gates == prog.info.total_gates
    bad = _mismatches(Cp, got, lsm.corpus_words(Cp))
    assert not bad, bad


def test_corpus_reaches_the_edges():
    """the minimum is each of -2^(w-1), -1, 0, 2^(w-1) - 1; it sits first, in the middle, last and at several places"""
    w = 64
    Cp = lsm.select_corpus(w, 56, np.random.default_rng(3))
    W = lsm.corpus_words(Cp)
    mins = {wm.s(W[r[2]], w) for r in Cp.launches[0][1]}
    assert {-(1 << 63), -1, 0, (1 << 63) - 1} <= mins
    where, several = set(), 0
    for r in Cp.launches[1][1]:
        cnt, hot, iv, ref, idx, sa = r[1], r[2], r[3], r[4], r[5], r[6]
        hits = [k for k in range(cnt) if W[iv + k * sa] == W[ref]]
        assert [W[hot + k] for k in range(cnt)] == [wm.mask(w) if hits and k == hits[0] else 0 for k in range(cnt)]
        if hits:
            where.add("first" if hits[0] == 0 else "last" if hits[0] == cnt - 1 else "middle")
            several += len(hits) > 1
    assert where == {"first", "middle", "last"} and several >= 6
    assert {r[1] for r in Cp.launches[2][1]} == set(lsm.CNTS)


@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_variant_costs(w, p):
    """a signed minimum costs what a maximum does; the one-hot one comparison per candidate and one gate per candidate but
    the first; the gated select one AND step of w gates per candidate"""
    def cost(rec):
        info = linreg_gc.RecordProgram(w, p, [rec], [1], n_inputs=0, n_words=600).info
        return info.total_steps, info.total_gates
    for cnt in (2, 9, 256):
        assert cost((OP_MAX, cnt, 1, 2, 2, 0, 1, 1)) == cost((OP_MAX, cnt, 1, 2, 1, 0, 1, 1))
        eq1 = cost((OP_EQ, 1, 1, 2, 3, 0, 1, 1))
        assert cost((OP_EQ, cnt, 300, 2, 1, 299, 1, 1)) == (cnt * eq1[0] + cnt - 1, cnt * eq1[1] + cnt - 1)
        assert cost((OP_SUM, cnt, 1, 2, 300, 0, 1, 1)) == (cnt, cnt * w)


# ---- structure of the lowering
def _launch_ops(prog):
    ops = _recs(prog)[:, 0]
    return [(Lc, ops[Lc["first_rec"]:Lc["first_rec"] + Lc["nrec"]]) for Lc in prog.launches()]


def test_scoring_runs_as_karatsuba_products_at_d96(lgc):
    """d = 96, w = 64: after the last OP_PROX launch the L d dot products of length d on M_v are OP_MACK records, d^2 + L d
    OP_HDIFF records form the shadow of M_v and of every beta_l, and the iteration marks are the path's"""
    d, L, N = 96, 3, 3
    sysm = lgc.make_system(d, 64, 56, "lasso", N, 0.01, 2, 1, 0, 0)
    values = VALUES[lsm.RATIO][:L]
    sel, path = program(lgc, sysm, values, lsm.RATIO, 0), lgc.Program(sysm, l1_ratios=values)
    recs, lo = _recs(sel), _launch_ops(sel)
    last_prox = max(i for i, (_, ops) in enumerate(lo) if (ops == OP_PROX).any())
    tail = recs[lo[last_prox + 1][0]["first_rec"]:]
    mack = tail[tail[:, 0] == OP_MACK]
    assert mack[:, 1].sum() == L * d * d and tail[tail[:, 0] == 1, 1].sum() == L * d      # plain products: the L score jobs only
    assert (tail[:, 0] == OP_HDIFF).sum() == d * d + L * d
    assert (tail[:, 0] == OP_REVEAL).sum() == d
    psel = [i for i, (_, ops) in enumerate(lo) if (ops == OP_PROX).any()]
    ppath = [i for i, (_, ops) in enumerate(_launch_ops(path)) if (ops == OP_PROX).any()]
    assert len(psel) == len(ppath) == N and [lo[i][0]["nrec"] for i in psel] == [L * d] * N


def test_selection_launches_do_not_grow_with_L(lgc):
    """the selection is the minimum tree (one launch per level of fan-in 8), one first-minimum record, one launch of d gated
    selects and the reveal: L = 2 .. 8 lower to the same number of launches, 9 .. 64 to one more, 65 .. 256 to two more"""
    d, N = 4, 2
    sysm = lgc.make_system(d, 64, 56, "lasso", N, 0.01, 2, 1, 0, 0)
    counts = {}
    for L in (2, 8, 9, 64, 65, 256):
        prog = program(lgc, sysm, [0.001 * (k + 1) for k in range(L)], lsm.ABSOLUTE, INDEX)
        lo = _launch_ops(prog)
        depth = 1 if L <= 8 else 2 if L <= 64 else 3
        tail = lo[-(depth + 3):]
        assert [sorted(set(ops.tolist())) for _, ops in tail] == [[OP_MAX]] * depth + [[OP_EQ], [OP_SUM], [OP_REVEAL]], L
        assert OP_MAX not in lo[-(depth + 4)][1]
        assert [Lc["nrec"] for Lc, _ in tail[depth:]] == [1, d, d + 1]
        r = _recs(prog)
        assert (r[:, 0] == OP_MAX).sum() - (r[(r[:, 0] == OP_MAX), 4] == 2).sum() == (_recs(lgc.Program(sysm, l1=[0.001]))[:, 0] == OP_MAX).sum()
        counts[L] = prog.info.n_launches
    assert counts[2] == counts[8] and counts[9] == counts[64] == counts[8] + 1 and counts[65] == counts[256] == counts[8] + 2


@pytest.mark.parametrize("d,w,p", [(5, 64, 56), (100, 64, 56), (17, 32, 24)])
def test_one_value_selects_nothing(lgc, d, w, p):
    """one value with validation: no variant record, beta_0 and the constant zero revealed, the path's OP_PROX records.
    (That programs WITHOUT validation lower as before is pinned by tests/test_program_digests.py: the binding's
    validation=False is the very call it made before, so comparing the two here would compare a program with itself.)"""
    sysm = lgc.make_system(d, w, p, "lasso", 4, 0.01, 2, 1, 0, 0)
    one = program(lgc, sysm, [0.003], lsm.ABSOLUTE, INDEX)
    r = _recs(one)
    assert not ((r[:, 0] == OP_MAX) & (r[:, 4] == 2)).any() and not ((r[:, 0] == OP_EQ) & (r[:, 1] > 1)).any()
    assert not ((r[:, 0] == OP_SUM) & (r[:, 4] != 0)).any()
    assert one.info.n_reveal == d + 1 and (r[:, 0] == OP_PROX).sum() == (_recs(lgc.Program(sysm, l1=[0.003]))[:, 0] == OP_PROX).sum()
    rv = r[r[:, 0] == OP_REVEAL]
    assert rv[-1, 3] == 0                                       # l* is read from word 0, the constant zero


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_reveal_inputs_gives_both_systems(lgc, gccpu, oracle, w, p, normalize):
    """reveal_inputs = 1 on a selection: 2 (T + d) words laid out as a share is -- a, b as every solver reveals them, then
    a_v (packed lower triangle of M_v) and b_v, which are the model's validation system"""
    d, L, N, lam = 5, 3, 3, 0.05
    T = d * (d + 1) // 2
    rng = np.random.default_rng(zlib.crc32(("reveal inputs %d %d" % (w, normalize)).encode()))
    A, b, Av, bv = two_systems(oracle, rng, d, w, p)
    shares, _, va = joined_shares(rng, A, b, Av, bv, 2, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, normalize, 1, 0)
    prog = program(lgc, sysm, VALUES[lsm.RATIO][:L], lsm.RATIO, INDEX)
    dec = plain(gccpu, prog, w, p, shares)
    got = sx(dec[prog.info.rv_inputs:prog.info.rv_inputs + 2 * (T + d)], w).tolist()
    a, bb = train_inputs(oracle, A, b, d, w, p, lam, normalize)
    Mv, bvv = lsm.validation_system(va, d, w, normalize)
    assert got == a + bb + [Mv[i][j] for i in range(d) for j in range(i + 1)] + bvv
    assert prog.info.rv_beta == prog.info.rv_inputs + 2 * (T + d)
    # ... and beta*, l* behind them are still the model's
    best, idx, scores, _ = lsm.lasso_select(a, bb, va, d, w, p, N, VALUES[lsm.RATIO][:L], lsm.RATIO, normalize)
    assert sx(dec[prog.info.rv_beta:prog.info.rv_beta + d + 1], w).tolist() == lsm.revealed(best, idx, scores, INDEX)


def test_karatsuba_scoring_matches_the_model(lgc, gccpu, oracle):
    """d = 96, w = 64, N = 2: the scoring products run as OP_MACK records on the half-difference shadow of M_v and of every
    beta_l; every revealed word is the integer model's (which knows nothing of Karatsuba products)"""
    w, p, d, L, N, lam, flags = 64, 56, 96, 2, 2, 0.01, INDEX | SCORES
    rng = np.random.default_rng(9601)
    A, b, Av, bv = two_systems(oracle, rng, d, w, p)
    shares, _, va = joined_shares(rng, A, b, Av, bv, 2, w)
    values = [0.5, 0.05]
    prog = program(lgc, lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0), values, lsm.RATIO, flags)
    r = _recs(prog)
    last_prox = np.nonzero(r[:, 0] == OP_PROX)[0][-1]
    assert r[last_prox:][r[last_prox:, 0] == OP_MACK, 1].sum() == L * d * d
    a, bb = train_inputs(oracle, A, b, d, w, p, lam, 1)
    best, idx, scores, _ = lsm.lasso_select(a, bb, va, d, w, p, N, values, lsm.RATIO, 1)
    assert any(best) and len(set(scores)) == L
    assert shown(prog, plain(gccpu, prog, w, p, shares), w, flags, L) == lsm.revealed(best, idx, scores, flags)


# ---- rejections
def test_rejections(lgc):
    d = 4
    sysm = lgc.make_system(d, 64, 56, "lasso", 5, 0.01, 2, 1, 0, 0)
    L = lgc.lib()

    def bad(want, *a, **k):
        with pytest.raises(lgc.LgcError) as e:
            lgc.Program(*a, validation=True, **k)
        assert e.value.code == -1 and want in str(e.value), str(e.value)

    # everything a path rejects, and the options' own
    bad("1..256 values", sysm, l1=[])
    bad("1..256 values", sysm, l1=[0.1] * 257)
    bad("must be finite and >= 0", sysm, l1=[0.1, -0.2])
    bad("[0, 2]", sysm, l1_ratios=[0.5, 2.5])
    bad("LGC_ALG_LASSO", lgc.make_system(d, 64, 56, "cgd", 5, 0.01, 2, 1, 0, 0), l1=[0.1, 0.2])
    bad("penalty factor 1", sysm, l1=[0.1], penalty_factors=[1, -1, 1, 1])
    bad("above its upper bound", sysm, l1=[0.1], lower=[0.5, 0, 0, 0], upper=[0.4, 1, 1, 1])
    bad("need", sysm)
    bad("sweep", sysm, l1=[0.1], lambdas=[0.1, 0.2])
    bad("targets", sysm, l1=[0.1], targets=2)
    # trace, for one value too
    tr = lgc.make_system(d, 64, 56, "lasso", 5, 0.01, 2, 1, 0, 1)
    bad("trace", tr, l1=0.1)
    bad("trace", tr, l1=[0.1, 0.2])
    with pytest.raises(lgc.LgcError) as e:
        lgc.Program(sysm, l1=[0.1], reveal_index=True)
    assert "validation=True" in str(e.value)
    # the C calls: unknown flag bits, a null opts
    vals = (C.c_double * 2)(0.1, 0.2)
    o = lgc.LassoOpts(2, C.cast(vals, C.c_void_p), 0, None, None, None)
    out = C.c_void_p()
    for flags in (4, 8 | 1, -1):
        assert L.lgc_program_build_lasso_select(C.byref(out), C.byref(sysm), C.byref(o), flags) == -1
        assert b"unknown reveal flags" in L.lgc_last_error()
    assert L.lgc_program_build_lasso_select(C.byref(out), C.byref(sysm), None, 0) == -1 and b"null opts" in L.lgc_last_error()
    assert L.lgc_program_build_lasso_select(C.byref(out), C.byref(sysm), C.byref(o), 3) == 0
    L.lgc_program_destroy(out)
    assert L.lgc_solver_selected_index(None) == -1 and L.lgc_party_selected_index(None) == -1
    # (refused before a GPU is looked for)
    with pytest.raises(lgc.LgcError) as e:
        lgc.Solver(tr, l1=[0.1], validation=True)
    assert "trace" in str(e.value)
    with pytest.raises(lgc.LgcError) as e:
        lgc.Party(sysm, lgc.GARBLER, seed=bytes(16), l1_ratios=[3.0], validation=True)
    assert "[0, 2]" in str(e.value)


def test_footprint_violations_are_refused(lgc):
    """the test-program hook runs every record on a machine that notes the words it touches: each variant's reads and writes
    beyond n_words are refused"""
    n = 40
    ok = [(OP_MAX, 9, 1, 10, 2, 0, 1, 1), (OP_EQ, 9, 20, 10, 1, 39, 1, 1), (OP_SUM, 9, 1, 10, 20, 0, 1, 1)]
    lgc.RecordProgram(64, 56, ok, [3], n_inputs=0, n_words=n).close()
    for rec in ((OP_MAX, 9, 1, 32, 2, 0, 1, 1),              # the last candidate
                (OP_EQ, 9, 32, 10, 1, 2, 1, 1),              # the last one-hot word
                (OP_EQ, 9, 20, 32, 1, 2, 1, 1),              # the last candidate
                (OP_EQ, 9, 20, 10, 40, 2, 1, 1),             # the reference word
                (OP_EQ, 9, 20, 10, 1, 40, 1, 1),             # the index word
                (OP_SUM, 9, 1, 10, 32, 0, 1, 1),             # the last gate word
                (OP_SUM, 9, 1, 10, 20, 0, 1, 3),             # ... through the stride
                (OP_SUM, 9, 1, 32, 20, 0, 1, 1)):            # the last value word
        with pytest.raises(lgc.LgcError) as e:
            lgc.RecordProgram(64, 56, [rec], [1], n_inputs=0, n_words=n)
        assert "outside n_words" in str(e.value), (rec, str(e.value))


def test_header_is_exported_and_documented(lgc):
    hdr = open(os.path.join(ROOT, "include", "linreg_gc_lasso_select.h")).read()
    names = set(re.findall(r"^[a-z][^\n(]*?\b(lgc_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    assert names == {"lgc_program_build_lasso_select", "lgc_solver_create_lasso_select", "lgc_party_create_lasso_select",
                     "lgc_solver_selected_index", "lgc_party_selected_index"}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for nme in names:
        assert hasattr(lgc.lib(), nme), nme
        assert nme in doc, nme
    for word in ("LGC_SELECT_REVEAL_INDEX", "LGC_SELECT_REVEAL_SCORES", "2 (T + d)", "lgc_p1_"):
        assert word in hdr, word
    assert "linreg_gc_lasso_select.h" in doc and "validation" in design and "K-fold" in design
    assert "validation=True" in open(os.path.join(ROOT, "README.md")).read()
