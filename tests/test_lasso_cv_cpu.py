"""In-circuit K-fold cross-validation of a lasso path (include/linreg_gc_lasso_cv.h) on the CPU: the lowered program, run
record by record by the CPU checker and garbled + evaluated by its CPU backends, against the independent model of
tests/lasso_cv_model.py; the fold fits and beta* against plain path programs of the existing entry points; a float64
restatement; the structure of the lowering; that programs differ with K and from a single hold-out's (the parties'
fingerprint itself needs a device: tests/test_lasso_cv_gpu.py); the rejections.  No GPU needed."""
import ctypes as C
import os
import re
import zlib

import numpy as np
import pytest

import lasso_cv_model as lcm
import lasso_model as lm
import test_lasso_select_cpu as sel
from helpers import split_shares, sx

ROOT = sel.ROOT
INDEX, SCORES = lcm.REVEAL_INDEX, lcm.REVEAL_SCORES
OP_IDIVC, OP_PROX, OP_MACK, OP_STEPEXP = 15, sel.OP_PROX, sel.OP_MACK, 25     # gc_exec.h
VALUES = sel.VALUES


def fold_words(rng, d, K, w, p, rows=None, sigma=0.1, density=0.6, beta=None):
    """[(A_k, b_k)] as words: K folds of rows of ONE planted model, A_k = X_k^T X_k / (n_k d) packed as the lower triangle row by
    row, b_k = X_k^T y_k / (n_k d)"""
    rows = rows or 2 * d + 10
    beta = rng.random(d) * (rng.random(d) < density) if beta is None else beta
    m = (1 << w) - 1
    out = []
    for _ in range(K):
        X = rng.standard_normal((rows, d)); X /= np.abs(X).max(axis=0)
        y = X @ beta + sigma * rng.standard_normal(rows)
        M, v = X.T @ X / (rows * d), X.T @ y / (rows * d)
        out.append((np.array([int(M[i][j] * 2.0 ** p) & m for i in range(d) for j in range(i + 1)], dtype=np.uint64),
                    np.array([int(x * 2.0 ** p) & m for x in v], dtype=np.uint64)))
    return out


def fold_shares(rng, folds, nshares, w):
    """(shares (nshares, K (T + d)), [the (nshares, T + d) rows of fold k])"""
    per = [split_shares(rng, A, b, nshares, w) for A, b in folds]
    return np.ascontiguousarray(np.hstack(per)), per


def program(lgc, sysm, K, values, mode, flags, **kw):
    key = "l1" if mode == lcm.ABSOLUTE else "l1_ratios"
    return lgc.Program(sysm, folds=K, reveal_index=bool(flags & INDEX), reveal_scores=bool(flags & SCORES), **dict(kw, **{key: list(values)}))


def run_plain(gccpu, prog, w, p, shares):
    """(decode slots, word file) of the program run record by record"""
    info = prog.info
    words = np.zeros(info.n_words, dtype=np.uint64)
    words[info.in_base:info.in_base + shares.size] = shares.ravel() & np.uint64((1 << w) - 1)
    dec = np.zeros(info.n_reveal + 1, dtype=np.uint64)
    steps, gates = gccpu.plain_run(prog.records(), info.n_records, w, p, words, dec)
    assert steps == info.total_steps and gates == info.total_gates
    return dec, words


def model(per, d, w, p, N, values, mode, normalize, lam, kw):
    return lcm.lasso_cv(per, d, w, p, N, values, mode, normalize, lam, kw.get("penalty_factors"), kw.get("lower"), kw.get("upper"))


GRID = [(d, K, L) for d in (1, 5) for K in (2, 3, 5) for L in (1, 2, 5)]


@pytest.mark.parametrize("d,K,L", GRID)
@pytest.mark.parametrize("mode", [lcm.ABSOLUTE, lcm.RATIO])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_program_reveals_the_model(lgc, gccpu, w, p, normalize, mode, d, K, L):
    """every revealed word of the lowered program, run record by record, is the model's: with and without factors / bounds,
    the reveal combinations"""
    rng = np.random.default_rng(zlib.crc32(("cv %d %d %d %d %d %d" % (w, normalize, mode, d, K, L)).encode()))
    N, lam = 6, 0.05
    shares, per = fold_shares(rng, fold_words(rng, d, K, w, p), 2, w)
    values = VALUES[mode][:L]
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, normalize, 0, 0)
    for kw in ({}, sel.options(d)):
        best, idx, cv, _ = model(per, d, w, p, N, values, mode, normalize, lam, kw)
        for flags in ((INDEX | SCORES, 0) if kw else (INDEX | SCORES, INDEX, SCORES)):
            prog = program(lgc, sysm, K, values, mode, flags, **kw)
            assert sel.shown(prog, run_plain(gccpu, prog, w, p, shares)[0], w, flags, L) == lcm.revealed(best, idx, cv, flags)


@pytest.mark.parametrize("d,K,L", GRID)
@pytest.mark.parametrize("mode", [lcm.ABSOLUTE, lcm.RATIO])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_cpu_garble_evaluate_gives_the_model(lgc, gccpu, w, p, normalize, mode, d, K, L):
    """the same grid garbled and evaluated on the CPU, with and without factors / bounds (N = 3; all three reveals without
    options, beta* alone with them)"""
    rng = np.random.default_rng(zlib.crc32(("cv ge %d %d %d %d %d %d" % (w, normalize, mode, d, K, L)).encode()))
    N, lam = 3, 0.05
    shares, per = fold_shares(rng, fold_words(rng, d, K, w, p), 2, w)
    values = VALUES[mode][:L]
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, normalize, 0, 0)
    for kw, flag_sets in (({}, (INDEX | SCORES,)), (sel.options(d), (INDEX | SCORES, 0))):
        best, idx, cv, _ = model(per, d, w, p, N, values, mode, normalize, lam, kw)
        for flags in flag_sets:
            prog = program(lgc, sysm, K, values, mode, flags, **kw)
            dec, gates, _ = gccpu.garble_eval(prog, shares)
            assert gates == prog.info.total_gates
            assert sel.shown(prog, dec, w, flags, L) == lcm.revealed(best, idx, cv, flags)


def _fits_from_words(prog, words, w, NF, L, d):
    """x_{f,l} of the word file: the OP_PROX records of the last iteration name them, fit-major then value-major"""
    r = sel._recs(prog)
    prox = r[r[:, 0] == OP_PROX]
    last = prox[-NF * L * d:]
    return sx(words[last[:, 2]], w).reshape(NF, L, d).tolist()


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_fits_are_plain_paths_of_existing_entry_points(lgc, gccpu, w, p, K):
    """every fold fit beta_{k,l}, read from the word file of a plaintext run, is the plain lasso path
    (lgc_program_build_lasso_path) on that fold's training system, and beta* is row l* of the plain path on the full system:
    absolute mode for the folds (a plain path's lambda_max would be the fold's own), ratio mode for the refit"""
    d, L, N, lam = 6, 4, 8, 0.05
    rng = np.random.default_rng(zlib.crc32(("cv rows %d %d" % (w, K)).encode()))
    shares, per = fold_shares(rng, fold_words(rng, d, K, w, p), 2, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0)
    systems = lcm.training_systems(lcm.fold_systems(per, d, w, 1), d, w, lm.to_fixed(lam, p, w))
    one = lgc.make_system(d, w, p, "lasso", N, 0.0, 1, 0, 0, 0)         # one share, nothing added: the system as given
    m = (1 << w) - 1

    def path_rows(s, **kw):
        path = lgc.Program(one, **kw)
        sh = np.array([[int(v) & m for v in systems[s][0] + systems[s][1]]], dtype=np.uint64)
        dec = run_plain(gccpu, path, w, p, sh)[0]
        return sx(dec[path.info.rv_beta:path.info.rv_beta + L * d], w).reshape(L, d).tolist()

    values = [0.001, 0.0002, 0.00002, 0.0005]
    prog = program(lgc, sysm, K, values, lcm.ABSOLUTE, INDEX)
    dec, words = run_plain(gccpu, prog, w, p, shares)
    fits = _fits_from_words(prog, words, w, K + 1, L, d)
    for s in range(K + 1):
        assert fits[s] == path_rows(s, l1=values), s
    assert len({tuple(r) for f in fits for r in f if any(r)}) >= 3 * (K + 1)    # (the fits differ between systems and values)
    got = sel.shown(prog, dec, w, INDEX, L)
    assert got[:d] == fits[K][got[d]]
    ratios = VALUES[lcm.RATIO][:L]
    prog = program(lgc, sysm, K, ratios, lcm.RATIO, INDEX)
    got = sel.shown(prog, run_plain(gccpu, prog, w, p, shares)[0], w, INDEX, L)
    assert got[:d] == path_rows(K, l1_ratios=ratios)[got[d]] and any(got[:d])


# ---- float64 restatement
def _float_cv(folds, d, p, N, ratios, lam):
    """the K-fold procedure in float64 numpy on the fold systems [(M_k, b_k)] (floats, normalised as the circuit's are)"""
    K = len(folds)
    totM, totb = sum(M for M, _ in folds), sum(b for _, b in folds)
    train = [((totM - M) / (K - 1) + lam * np.eye(d), (totb - b) / (K - 1)) for M, b in folds] + [(totM / K + lam * np.eye(d), totb / K)]
    lmax = np.abs(train[K][1]).max()
    s = max(0, (d - 1).bit_length())

    def fit(M, b, theta1):
        ell = s + int(np.floor(np.abs(M) * 2.0 ** p / 2.0 ** s).sum(axis=1).max()).bit_length()
        step = 2.0 ** (p - ell)
        x, y, t = np.zeros(d), np.zeros(d), 1.0
        for _ in range(N):
            z = y - step * (M @ y - b)
            xn = np.sign(z) * np.maximum(np.abs(z) - step * theta1, 0.0)
            tn = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
            y, x, t = xn + (t - 1.0) / tn * (xn - x), xn, tn
        return x
    cv = []
    for r in ratios:
        fits = [fit(M, b, r * lmax) for M, b in train[:K]]
        cv.append(sum(f @ Mv @ f - 2.0 * bv @ f for f, (Mv, bv) in zip(fits, folds)))
    return np.array(cv)


# largest |integer - float| cross-validation score over the 20 systems below, as measured: 3.886e-16 (the scores are of order
# 1e-2 and a word's last place is 2^-56 = 1.4e-17: a few hundred truncations and the rounding of float64 itself), and the
# tolerance on the gap between the two best float scores: ten times that, for seeds not seen.  The smallest gap among the 20
# is 2.1e-5, so none falls under it
CV_MEASURED = 3.886e-16
CV_TOLERANCE = 10 * CV_MEASURED
FLOAT_SEEDS = list(range(20))


def test_float_restatement_agrees_on_the_selected_index(lgc, gccpu):
    """W = 64, p = 56, 20 planted-sparse systems: the integer l* is the float arg-min wherever the float gap between the two
    best cv scores exceeds CV_TOLERANCE; at most 2 systems fall under it; one at least selects an interior index"""
    w, p, d, K, N, lam = 64, 56, 6, 4, 40, 0.001
    ratios = [1.2, 0.6, 0.3, 0.15, 0.07, 0.03, 0.01, 0.003]
    L = len(ratios)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, 0, 0, 0)
    prog = program(lgc, sysm, K, ratios, lcm.RATIO, INDEX | SCORES)
    worst, under, interior = 0.0, 0, 0
    for seed in FLOAT_SEEDS:
        rng = np.random.default_rng(1000 + seed)
        beta = np.zeros(d); beta[rng.choice(d, 2, replace=False)] = rng.uniform(0.5, 1.5, 2)
        folds = fold_words(rng, d, K, w, p, rows=12, sigma=0.5, beta=beta)
        shares, _ = fold_shares(rng, folds, 2, w)
        got = sel.shown(prog, run_plain(gccpu, prog, w, p, shares)[0], w, INDEX | SCORES, L)
        idx, cv_int = got[d], np.array(got[d + 1:], dtype=np.float64) / 2.0 ** p
        fl = []
        for A, b in folds:
            M = np.array(lm.full_matrix(A, d, w), dtype=np.float64) / 2.0 ** p
            fl.append((M, sx(b, w).astype(np.float64) / 2.0 ** p))
        cv = _float_cv(fl, d, p, N, ratios, float(lm.to_fixed(lam, p, w)) / 2.0 ** p)
        worst = max(worst, float(np.abs(cv_int - cv).max()))
        order = np.sort(cv)
        print("seed %d: l* = %d, float arg-min %d, gap %.3e, max |int - float| %.3e" % (seed, idx, int(cv.argmin()), order[1] - order[0], np.abs(cv_int - cv).max()))
        if order[1] - order[0] > CV_TOLERANCE:
            assert idx == int(cv.argmin()), seed
        else:
            under += 1
        interior += 0 < idx < L - 1
    print("largest |integer - float| cv score: %.3e" % worst)
    assert worst <= CV_TOLERANCE and under <= 2 and interior >= 1


# ---- structure of the lowering
def test_structure_of_the_lowering(lgc):
    """K = 3, L = 4, d = 5 with options: (K + 1) L d OP_PROX records per iteration in ONE launch, K + 1 times the plain path's
    OP_STEPEXP groups, divisions by K - 1 and K; K = 2 divides by d and by K only; one value fits the full system alone"""
    d, L, N = 5, 4, 3
    sysm = lgc.make_system(d, 64, 56, "lasso", N, 0.01, 2, 1, 0, 0)
    T = d * (d + 1) // 2
    values = VALUES[lcm.RATIO][:L]
    kw = sel.options(d)
    base = sel._recs(lgc.Program(sysm, l1_ratios=values, **kw))
    for K in (2, 3):
        prog = program(lgc, sysm, K, values, lcm.RATIO, 0, **kw)
        r = sel._recs(prog)
        per_launch = [int((ops == OP_PROX).sum()) for _, ops in sel._launch_ops(prog) if (ops == OP_PROX).any()]
        assert per_launch == [(K + 1) * L * d] * N
        assert (r[:, 0] == OP_STEPEXP).sum() == (K + 1) * (base[:, 0] == OP_STEPEXP).sum()
        div = r[r[:, 0] == OP_IDIVC]
        want = {d: K * T, K: T + d}                      # by d: the off-diagonals and b of every fold
        if K > 2:
            want[K - 1] = K * (T + d)
        assert {int(c): int((div[:, 5] == c).sum()) for c in set(div[:, 5].tolist())} == want
        assert prog.info.n_reveal == d
        one = program(lgc, sysm, K, values[:1], lcm.RATIO, INDEX | SCORES)
        r1 = sel._recs(one)
        assert (r1[:, 0] == OP_PROX).sum() == N * d and one.info.n_reveal == d + 2
        rv = r1[r1[:, 0] == sel.OP_REVEAL]
        assert rv[-1, 3] == 0 and rv[-2, 3] == 0            # l* and cv_0 are read from word 0, the constant zero


def test_programs_differ_with_the_folds_and_from_a_hold_out(lgc):
    """the record bytes and word counts of K = 2, K = 3 and a single hold-out differ pairwise.  (This is not
    lgc_party_program_fingerprint, which needs a party and hence a device: tests/test_lasso_cv_gpu.py compares it.)"""
    d = 4
    sysm = lgc.make_system(d, 64, 56, "lasso", 3, 0.01, 2, 1, 0, 0)
    values = VALUES[lcm.RATIO][:3]
    progs = [program(lgc, sysm, K, values, lcm.RATIO, INDEX) for K in (2, 3)] + [sel.program(lgc, sysm, values, lcm.RATIO, INDEX)]
    digests = {zlib.crc32(pr.records().tobytes()) for pr in progs}
    assert len(digests) == 3 and len({pr.info.n_words for pr in progs}) == 3


# ---- rejections and the interface
def test_rejections(lgc):
    d = 4
    sysm = lgc.make_system(d, 64, 56, "lasso", 5, 0.01, 2, 1, 0, 0)
    Lb = lgc.lib()

    def bad(want, *a, **k):
        with pytest.raises(lgc.LgcError) as e:
            lgc.Program(*a, **dict(dict(folds=3), **k))
        assert e.value.code == -1 and want in str(e.value), str(e.value)

    for K in (0, 1, 17, 1000):
        bad("2..16 folds", sysm, l1=[0.1, 0.2], folds=K)
    tr = lgc.make_system(d, 64, 56, "lasso", 5, 0.01, 2, 1, 0, 1)
    bad("trace", tr, l1=[0.1, 0.2])
    bad("trace", tr, l1=0.1)
    bad("exclude each other", sysm, l1=[0.1], validation=True)
    bad("needs l1 or l1_ratios", sysm)
    # everything the options and a path reject
    bad("1..256 values", sysm, l1=[])
    bad("1..256 values", sysm, l1=[0.1] * 257)
    bad("must be finite and >= 0", sysm, l1=[0.1, -0.2])
    bad("[0, 2]", sysm, l1_ratios=[0.5, 2.5])
    bad("LGC_ALG_LASSO", lgc.make_system(d, 64, 56, "cgd", 5, 0.01, 2, 1, 0, 0), l1=[0.1, 0.2])
    bad("penalty factor 1", sysm, l1=[0.1], penalty_factors=[1, -1, 1, 1])
    bad("above its upper bound", sysm, l1=[0.1], lower=[0.5, 0, 0, 0], upper=[0.4, 1, 1, 1])
    bad("sweep", sysm, l1=[0.1], lambdas=[0.1, 0.2])
    bad("targets", sysm, l1=[0.1], targets=2)
    # a program whose word ids would not fit: refused before it is lowered
    bad("too large", lgc.make_system(100, 64, 56, "lasso", 5, 0.01, 1 << 20, 1, 0, 0), l1=[0.1, 0.2], folds=16)
    bad("too large", lgc.make_system(4096, 64, 56, "lasso", 5, 0.01, 2, 1, 0, 0), l1=[0.1] * 256, folds=16)
    with pytest.raises(lgc.LgcError) as e:
        lgc.Program(sysm, l1=[0.1], reveal_index=True)
    assert "folds=K" in str(e.value)
    # the C calls: unknown flag bits, a null opts
    vals = (C.c_double * 2)(0.1, 0.2)
    o = lgc.LassoOpts(2, C.cast(vals, C.c_void_p), 0, None, None, None)
    out = C.c_void_p()
    for flags in (4, 8 | 1, -1):
        assert Lb.lgc_program_build_lasso_cv(C.byref(out), C.byref(sysm), C.byref(o), 3, flags) == -1
        assert b"unknown reveal flags" in Lb.lgc_last_error()
    assert Lb.lgc_program_build_lasso_cv(C.byref(out), C.byref(sysm), None, 3, 0) == -1 and b"null opts" in Lb.lgc_last_error()
    assert Lb.lgc_program_build_lasso_cv(C.byref(out), C.byref(sysm), C.byref(o), 16, 3) == 0
    Lb.lgc_program_destroy(out)
    assert Lb.lgc_solver_num_folds(None) == 0 and Lb.lgc_party_num_folds(None) == 0
    # (refused before a GPU is looked for)
    with pytest.raises(lgc.LgcError) as e:
        lgc.Solver(tr, l1=[0.1], folds=2)
    assert "trace" in str(e.value)
    with pytest.raises(lgc.LgcError) as e:
        lgc.Party(sysm, lgc.GARBLER, seed=bytes(16), l1_ratios=[0.3], folds=17)
    assert "2..16 folds" in str(e.value)


@pytest.mark.parametrize("normalize", [0, 1])
def test_reveal_inputs_gives_the_folds(lgc, gccpu, normalize):
    """reveal_inputs = 1: K (T + d) words laid out as a share is, the folds as the model assembles them"""
    w, p, d, K, L, N, lam = 64, 56, 4, 3, 2, 2, 0.05
    rng = np.random.default_rng(31 + normalize)
    shares, per = fold_shares(rng, fold_words(rng, d, K, w, p), 2, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, normalize, 1, 0)
    prog = program(lgc, sysm, K, VALUES[lcm.RATIO][:L], lcm.RATIO, INDEX)
    dec = run_plain(gccpu, prog, w, p, shares)[0]
    n = K * (d * (d + 1) // 2 + d)
    want = [v for M, b in lcm.fold_systems(per, d, w, normalize) for v in lcm.packed(M, d) + list(b)]
    assert sx(dec[prog.info.rv_inputs:prog.info.rv_inputs + n], w).tolist() == want and prog.info.rv_beta == prog.info.rv_inputs + n


def test_header_is_exported_and_documented(lgc):
    hdr = open(os.path.join(ROOT, "include", "linreg_gc_lasso_cv.h")).read()
    names = set(re.findall(r"^[a-z][^\n(]*?\b(lgc_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    assert names == {"lgc_program_build_lasso_cv", "lgc_solver_create_lasso_cv", "lgc_party_create_lasso_cv",
                     "lgc_solver_num_folds", "lgc_party_num_folds"}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for nme in names:
        assert hasattr(lgc.lib(), nme), nme
        assert nme in doc, nme
    for word in ("LGC_MAX_FOLDS 16", "K (T + d)", "lgc_p1_", "BOTH input paths", "equal in size to within one row"):
        assert word in hdr, word
    assert "linreg_gc_lasso_cv.h" in doc and "folds" in design and "one-standard-error" in design
    assert "folds=" in open(os.path.join(ROOT, "README.md")).read()
