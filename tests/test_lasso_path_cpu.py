"""The lasso path (include/linreg_gc_lasso_path.h) on the CPU: the lowered program, run record by record by the CPU checker and
garbled + evaluated by its CPU backends, against the independent model of tests/lasso_path_model.py and against single lasso
solves; the ratio mode's semantics; the shared setup and the merged launches at d = 100; the OP_STEPEXP cnt = 2 variant on
edge operands; the rejections, bin/linreg's options and the header.  No GPU needed."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import lasso_model as lm
import lasso_path_model as lpm
import linreg_gc
import op_corpus as oc
import word_model as wm
from helpers import split_shares, sx, synth_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OP_ABSSUM, OP_STEPEXP, OP_PROX, OP_HDIFF = 24, 25, 26, 21        # gc_exec.h
ABS_VALUES = [0.0, 0.0005, 0.001, 0.002, 0.003, 0.005, 0.008, 0.02]
RATIOS = [0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 1.0, 1.0625]


def _recs(prog):
    return np.frombuffer(prog.records().tobytes(), dtype=np.uint32).reshape(-1, 10)


def _inputs(oracle, A, b, d, w, p, lam, normalize):
    a = oracle.sum_shares(np.asarray(A, dtype=np.uint64)[None, :], w)
    bb = oracle.sum_shares(np.asarray(b, dtype=np.uint64)[None, :], w)
    if normalize:
        a, bb = oracle.circuit_input(a, bb, d, lam, p, w)
    return sx(a, w).tolist(), sx(bb, w).tolist()


def _plain(gccpu, prog, w, p, shares):
    info = prog.info
    words = np.zeros(info.n_words, dtype=np.uint64)
    words[info.in_base:info.in_base + shares.size] = shares.ravel() & np.uint64((1 << w) - 1)
    dec = np.zeros(info.n_reveal + 1, dtype=np.uint64)
    steps, gates = gccpu.plain_run(prog.records(), info.n_records, w, p, words, dec)
    assert steps == info.total_steps and gates == info.total_gates
    return dec


def _beta(prog, dec, w, rows):
    info = prog.info
    return sx(dec[info.rv_beta:info.rv_beta + rows * prog.system.d], w).reshape(rows, prog.system.d).tolist()


def _values(mode, L):
    vals = ABS_VALUES if mode == lpm.ABSOLUTE else RATIOS
    return [vals[(3 * i + 1) % len(vals)] for i in range(L)] if L < len(vals) else vals[:L]


def _program(lgc, sysm, mode, values):
    return lgc.Program(sysm, l1=values) if mode == lpm.ABSOLUTE else lgc.Program(sysm, l1_ratios=values)


def _case(oracle, rng, d, w, p):
    return synth_system(oracle, rng, 3 * d + 20, d, w, p)


@pytest.mark.parametrize("L", [1, 3, 8])
@pytest.mark.parametrize("mode", [lpm.ABSOLUTE, lpm.RATIO])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 28)])
def test_path_reveals_the_model(lgc, gccpu, oracle, w, p, normalize, mode, L):
    """every beta_l of the lowered path, run record by record, is the model's"""
    d, N, lam = 5, 6, 0.05
    rng = np.random.default_rng(zlib.crc32(("path %d %d %d %d" % (w, normalize, mode, L)).encode()))
    A, b = _case(oracle, rng, d, w, p)
    shares = split_shares(rng, A, b, 2, w)
    values = _values(mode, L)
    prog = _program(lgc, lgc.make_system(d, w, p, "lasso", N, lam, 2, normalize, 0, 0), mode, values)
    dec = _plain(gccpu, prog, w, p, shares)
    a, bb = _inputs(oracle, A, b, d, w, p, lam, normalize)
    betas, _, th = lpm.lasso_path(a, bb, d, w, p, N, values, mode)
    assert _beta(prog, dec, w, L) == betas
    if L == 8:
        assert len(set(th)) > 2 and len(set(map(tuple, betas))) > 2       # the values reach the result


@pytest.mark.parametrize("mode", [lpm.ABSOLUTE, lpm.RATIO])
def test_karatsuba_size_matches_the_model(lgc, gccpu, oracle, mode):
    """d = 96: the L d dot products run through OP_MACK on the hdiff(y_l) words of every value's OP_PROX records"""
    rng = np.random.default_rng(96 + mode)
    w, p, d, N, lam, L = 64, 56, 96, 3, 0.01, 3
    A, b = _case(oracle, rng, d, w, p)
    shares = split_shares(rng, A, b, 2, w)
    values = [0.0002, 0.0005, 0.002] if mode == lpm.ABSOLUTE else [0.05, 0.2, 0.6]
    prog = _program(lgc, lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0), mode, values)
    recs = _recs(prog)
    assert (recs[:, 0] == 20).any() and (recs[recs[:, 0] == OP_PROX, 7] != 0).all()
    dec = _plain(gccpu, prog, w, p, shares)
    a, bb = _inputs(oracle, A, b, d, w, p, lam, 1)
    assert _beta(prog, dec, w, L) == lpm.lasso_path(a, bb, d, w, p, N, values, mode)[0]


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 28)])
def test_absolute_path_is_single_solves(lgc, gccpu, oracle, w, p, normalize):
    """beta_l of an absolute path is bit for bit the beta of lgc_program_build_lasso with lambda1 = values[l]"""
    d, N, lam = 7, 5, 0.02
    rng = np.random.default_rng(zlib.crc32(("single %d %d" % (w, normalize)).encode()))
    A, b = _case(oracle, rng, d, w, p)
    shares = split_shares(rng, A, b, 2, w)
    sysm = lgc.make_system(d, w, p, "lasso", N, lam, 2, normalize, 0, 0)
    values = [0.004, 0.0, 0.001]
    path = lgc.Program(sysm, l1=values)
    got = _beta(path, _plain(gccpu, path, w, p, shares), w, 3)
    for l, v in enumerate(values):
        one = lgc.Program(sysm, l1=v)
        assert got[l] == _beta(one, _plain(gccpu, one, w, p, shares), w, 1)[0], l


@pytest.mark.parametrize("mode", [lpm.ABSOLUTE, lpm.RATIO])
@pytest.mark.parametrize("w,p", [(64, 56), (32, 28)])
def test_cpu_garble_evaluate_gives_the_model(lgc, gccpu, oracle, w, p, mode):
    d, N, lam, L = 4, 3, 0.05, 3
    rng = np.random.default_rng(zlib.crc32(("ge %d %d" % (w, mode)).encode()))
    A, b = _case(oracle, rng, d, w, p)
    shares = split_shares(rng, A, b, 2, w)
    values = _values(mode, L)
    prog = _program(lgc, lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0), mode, values)
    dec, gates, _ = gccpu.garble_eval(prog, shares)
    assert gates == prog.info.total_gates
    a, bb = _inputs(oracle, A, b, d, w, p, lam, 1)
    assert _beta(prog, dec, w, L) == lpm.lasso_path(a, bb, d, w, p, N, values, mode)[0]


@pytest.mark.parametrize("d,w,p", [(5, 64, 56), (100, 64, 56), (17, 32, 28)])
def test_one_value_is_the_single_program(lgc, d, w, p):
    """an absolute path with L = 1 is the single lasso program: records, launches and every lgc_program_info field"""
    for normalize in (0, 1):
        sysm = lgc.make_system(d, w, p, "lasso", 4, 0.01, 2, normalize, 0, 0)
        a, b = lgc.Program(sysm, l1=0.003), lgc.Program(sysm, l1=[0.003])
        assert a.records().tobytes() == b.records().tobytes()
        assert a.launches() == b.launches()
        assert [getattr(a.info, f) for f, _ in lgc.ProgramInfo._fields_] == [getattr(b.info, f) for f, _ in lgc.ProgramInfo._fields_]
        assert b.path == 1 and a.path is None


def _planted(oracle, rng, w, p, d, n):
    X = rng.standard_normal((n, d)); X /= np.abs(X).max(axis=0)
    beta_true = np.zeros(d); beta_true[[1, 4, 9]] = [0.9, -0.7, 0.5]
    y = X @ beta_true + 0.01 * rng.standard_normal(n)
    return oracle.aggregate(oracle.quantize(X, p, n, w), oracle.quantize(y, p, n, w), n, d, p, w)


def test_ratio_semantics(lgc, gccpu, oracle):
    """ratio 1.0625 of lambda_max gives beta = 0 exactly; smaller ratios agree with float64 FISTA (same step, same c_k,
    lambda1 = r lambda_max) on the support wherever |z| has a margin over theta"""
    rng = np.random.default_rng(77)
    w, p, d, n, N, lam = 64, 56, 12, 400, 60, 0.01
    A, b = _planted(oracle, rng, w, p, d, n)
    shares = split_shares(rng, A, b, 2, w)
    ratios = [1.0625, 0.5, 0.2, 0.05]
    prog = lgc.Program(lgc.make_system(d, w, p, "lasso", N, lam, 2, 1, 0, 0), l1_ratios=ratios)
    got = np.array(_beta(prog, _plain(gccpu, prog, w, p, shares), w, len(ratios)))
    a, bb = _inputs(oracle, A, b, d, w, p, lam, 1)
    M = lm.full_matrix(a, d, w)
    ell = lm.step_exponent(M, d, w)
    lmax = lpm.lambda_max(bb, w)
    assert lmax >= 2 ** (ell - p + 5)                                     # the fixture's condition
    betas = lpm.lasso_path(a, bb, d, w, p, N, ratios, lpm.RATIO)[0]
    assert got.tolist() == betas
    assert (got[0] == 0).all()
    Mf = np.array(M, dtype=float) / 2.0 ** p
    bf = np.array(bb, dtype=float) / 2.0 ** p
    c = [ck / 2.0 ** p for ck in lm.coefficients(N, w, p)]
    alpha = 2.0 ** (p - ell)
    for l, r in enumerate(ratios[1:], 1):
        theta = alpha * r * lmax / 2.0 ** p
        x = np.zeros(d); y = np.zeros(d); z = np.zeros(d)
        for ck in c:
            z = y - alpha * (Mf @ y - bf)
            xn = np.sign(z) * np.maximum(np.abs(z) - theta, 0.0)
            y = xn + ck * (xn - x)
            x = xn
        sure = np.abs(np.abs(z) - theta) > 1e-6
        assert sure.sum() >= d - 1, (l, sure)
        assert ((got[l] != 0) == (np.abs(z) > theta))[sure].all(), (l, got[l], z, theta)
    assert (got[3] != 0).sum() > (got[1] != 0).sum()                     # a smaller ratio keeps more coordinates


def test_structure_at_d100(lgc):
    """d = 100, N = 15, L = 8: the launches of a single solve; hdiff(M) and the row sums of M once; L N d OP_PROX records in
    exactly N launches; fewer than 8 x the single solve's AND gates"""
    d, N, L = 100, 15, 8
    sysm = lgc.make_system(d, 64, 56, "lasso", N, 0.001, 2, 1, 0, 0)
    one = lgc.Program(sysm, l1=0.001)
    r1 = _recs(one)
    s = 7                                                                # ceil(log2 100): the shift of M's row sums
    for mode, values in ((lpm.ABSOLUTE, ABS_VALUES), (lpm.RATIO, RATIOS)):
        path = _program(lgc, sysm, mode, values)
        rp = _recs(path)
        assert path.info.n_launches == one.info.n_launches, mode
        for op in (OP_HDIFF,):
            assert (rp[:, 0] == op).sum() == (r1[:, 0] == op).sum(), (mode, op)
        m_abs = lambda r: ((r[:, 0] == OP_ABSSUM) & (r[:, 5] == s)).sum()
        assert m_abs(rp) == m_abs(r1) > 0
        assert ((rp[:, 0] == OP_ABSSUM).sum() - m_abs(rp)) == (d if mode == lpm.RATIO else 0)
        assert (rp[:, 0] == OP_STEPEXP).sum() == L and set(rp[rp[:, 0] == OP_STEPEXP, 1]) == ({2} if mode else {1})
        ops = rp[:, 0]
        prox = [Lc for Lc in path.launches() if (ops[Lc["first_rec"]:Lc["first_rec"] + Lc["nrec"]] == OP_PROX).any()]
        assert len(prox) == N and all(Lc["nrec"] == L * d for Lc in prox)
        assert (ops == OP_PROX).sum() == L * N * d
        assert path.info.total_gates < 8 * one.info.total_gates, (mode, path.info.total_gates / one.info.total_gates)


# ---- the OP_STEPEXP cnt = 2 variant against the integer model
def _s32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def ratio_corpus(w, p, rng):
    """OP_STEPEXP cnt = 2 records on edge operands: m of every bit length, lambda_max 0, 1, random and near the top, r in
    {0, 1.0, 2^-p, 2.0, popcount-heavy}; returns (corpus, [(out word, m, lambda, r, s)])"""
    ms = [0] + [(1 << k) - 1 for k in range(1, w + 1)] + [1 << k for k in range(w)]
    ms = [x & wm.mask(w) for x in ms]
    lams = [0, 1, (1 << (w - 2)) - 1] + [int(x) & ((1 << (w - 2)) - 1) for x in rng.integers(0, 1 << 62, 5, dtype=np.uint64)]
    heavy = 0x5555555555555555 & wm.mask(w - 1) | 1
    rs = [0, 1, (1 << p) & wm.mask(w), (2 << p) & wm.mask(w), heavy, wm.mask(w - 1), (1 << p) + 0x0F0F & wm.mask(w)]
    def once(n_inputs):
        C = oc.Corpus(w, p, n_inputs)
        im, il = C.inp(ms), C.inp(lams)
        recs, cases = [], []
        for k, m in enumerate(ms):
            for j, r in enumerate(rs):
                li = (k + 3 * j) % len(lams)
                s = (k + j) % 3 * 4
                o = C.out(3)
                recs.append((OP_STEPEXP, 2, o, im + k, il + li, s, _s32(r), _s32(r >> 32)))
                cases.append((o, m, lams[li], r, s))
        C.launch("gen", recs)
        return C, cases
    C0, _ = once(None)
    return once(len(C0.inputs))


def _ratio_expect(C, cases):
    w, p = C.w, C.p
    want = {}
    for o, m, lam, r, s in cases:
        _, th, nth = lpm.stepexp_ratio(m, lam, r, s, w, p)
        ell = s + m.bit_length()
        want[o] = wm.Model(None, w, p).step_word(ell)
        want[o + 1], want[o + 2] = th & wm.mask(w), nth & wm.mask(w)
    return want


@pytest.mark.parametrize("w", [64, 32])
def test_stepexp_ratio_variant_plain(gccpu, w):
    for p in (1, w - 8, w - 1):
        C, cases = ratio_corpus(w, p, np.random.default_rng([w, p]))
        prog = C.program(linreg_gc, lambda kind: ("auto", "auto"))
        got = oc.plain_words(gccpu, prog, C)
        want = _ratio_expect(C, cases)
        bad = [(o, hex(got[o]), hex(v)) for o, v in want.items() if got[o] != v]
        assert not bad, (w, p, bad[:6])


@pytest.mark.parametrize("w", [64, 32])
def test_stepexp_ratio_variant_garbled(gccpu, w):
    p = w - 8
    C, cases = ratio_corpus(w, p, np.random.default_rng([w, p, 1]))
    prog = C.program(linreg_gc, lambda kind: ("auto", "auto"))
    got, gates, _ = gccpu.garble_eval(prog, np.array(C.inputs, dtype=np.uint64))
    assert gates == prog.info.total_gates
    want = _ratio_expect(C, cases)
    bad = [o for o, v in want.items() if int(got[o]) & wm.mask(w) != v]
    assert not bad, bad[:6]


def test_stepexp_cost_follows_the_ratio():
    """the cost of an OP_STEPEXP cnt = 2 record is keyed on r: a popcount-heavy ratio costs more than a power of two"""
    def gates(r):
        rec = (OP_STEPEXP, 2, 3, 1, 2, 4, _s32(r), _s32(r >> 32))
        return linreg_gc.RecordProgram(64, 56, [rec, rec], [2], n_inputs=2, n_words=6).info.total_gates
    assert gates(1 << 56) < gates(0x5555555555555555) and gates(0) < gates(1 << 56)
    one = (OP_STEPEXP, 1, 3, 1, 2, 4, 1, 1)
    assert linreg_gc.RecordProgram(64, 56, [one], [1], n_inputs=2, n_words=6).info.total_gates < gates(1 << 56) / 2


# ---- rejections, bin/linreg, the header
def test_rejections(lgc):
    sysm = lgc.make_system(4, 64, 56, "lasso", 5, 0.01, 2, 1, 0, 0)
    L = lgc.lib()

    def bad(want, *a, **k):
        with pytest.raises(lgc.LgcError) as e:
            lgc.Program(*a, **k)
        assert e.value.code == -1 and want in str(e.value), str(e.value)

    bad("1..256", sysm, l1=[])
    bad("1..256", sysm, l1=[0.1] * 257)
    bad("1..256", sysm, l1_ratios=[])
    for v in (-0.1, float("nan"), float("inf")):
        bad("finite", sysm, l1=[0.1, v])
        bad("finite", sysm, l1_ratios=[v])
    bad("[0, 2]", sysm, l1_ratios=[0.5, 2.5])
    bad("precision", lgc.make_system(4, 32, 31, "lasso", 5, 0.01, 2, 1, 0, 0), l1_ratios=[1.0])
    bad("LGC_ALG_LASSO", lgc.make_system(4, 64, 56, "cgd", 5, 0.01, 2, 1, 0, 0), l1_ratios=[0.5])
    bad("trace", lgc.make_system(4, 64, 56, "lasso", 5, 0.01, 2, 1, 0, 1), l1=[0.1, 0.2])
    bad("exclude", sysm, l1=[0.1], l1_ratios=[0.5])
    lgc.Program(lgc.make_system(4, 64, 56, "lasso", 5, 0.01, 2, 1, 0, 1), l1=[0.1]).close()   # trace with one value
    import ctypes as C
    out = C.c_void_p()
    vals = (C.c_double * 2)(0.1, 0.2)
    assert L.lgc_program_build_lasso_path(C.byref(out), C.byref(sysm), 2, vals, 7) == -1 and b"mode" in L.lgc_last_error()
    assert L.lgc_program_build_lasso_path(C.byref(out), C.byref(sysm), 2, None, 0) == -1 and b"null" in L.lgc_last_error()
    for nm in ("lgc_solver_create_lasso_path", "lgc_party_create_lasso_path"):        # (refused before a GPU is looked for)
        with pytest.raises(lgc.LgcError) as e:
            if nm.startswith("lgc_solver"):
                lgc.Solver(sysm, l1_ratios=[3.0])
            else:
                lgc.Party(sysm, lgc.GARBLER, seed=bytes(16), l1_ratios=[3.0])
        assert "[0, 2]" in str(e.value)
    L.lgc_solver_path_length.restype = C.c_size_t
    assert L.lgc_solver_path_length(None) == 0 and L.lgc_party_path_length(None) == 0
    # the existing lasso rejections keep their wording
    bad("sweep", sysm, lambdas=[0.1, 0.2])
    bad("target", sysm, targets=2)


def _linreg(*args):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "linreg-mpc_amd", "host")], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "linreg-mpc_amd", "host", "bin", "linreg")
    inp = os.path.join(ROOT, "tests", "golden", "readme_example.in")
    return subprocess.run([exe, inp, "56", "3"] + list(args), capture_output=True, timeout=60)


def test_bin_linreg_options():
    """--l1 and --l1_ratios exclude each other; lasso still needs one of them (the message names --l1); lists are numbers"""
    for args, want in ((["lasso", "10", "0.001"], b"--l1"),
                       (["lasso", "10", "0.001", "--l1=0.1", "--l1_ratios=0.5"], b"exclude"),
                       (["lasso", "10", "0.001", "--l1_ratios=0.5,x"], b"--l1_ratios"),
                       (["lasso", "10", "0.001", "--l1=0.1,,0.2"], b"--l1"),
                       (["cgd", "10", "0.001", "--l1_ratios=0.5"], b"--l1_ratios"),
                       (["lasso", "10", "0.001", "--l1_ratios=0.5,2.5"], b"[0, 2]")):
        r = _linreg(*args)
        assert r.returncode != 0 and want in r.stdout + r.stderr, (args, r.stdout[-300:], r.stderr[-300:])


def test_lasso_path_header_is_exported_and_documented(lgc):
    hdr = open(os.path.join(ROOT, "include", "linreg_gc_lasso_path.h")).read()
    names = set(re.findall(r"^[a-z][^\n(]*?\b(lgc_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    assert names == {"lgc_program_build_lasso_path", "lgc_solver_create_lasso_path", "lgc_party_create_lasso_path",
                     "lgc_solver_path_length", "lgc_party_path_length"}
    assert re.search(r"#define LGC_L1_ABSOLUTE 0\b", hdr) and re.search(r"#define LGC_L1_RATIO 1\b", hdr)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for nme in names:
        assert hasattr(lgc.lib(), nme), nme
        assert nme in doc, nme
    assert "linreg_gc_lasso_path.h" in doc and "1.8" in doc and "lambda_max" in design.replace("λ_max", "lambda_max")
    assert "--l1_ratios" in open(os.path.join(ROOT, "README.md")).read()
    assert "lasso_path" not in open(os.path.join(ROOT, "include", "linreg_gc_lasso.h")).read()
