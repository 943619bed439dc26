"""Every record op on every record kernel that can run it, on the GPU, against the plaintext machine (the numbers the
kernels must produce) and the integer model (word_model.py), at the edge operands of helpers.edge_operands; the launch
geometry of each kernel at the record counts where it changes; launches of different kernels chained.  Test programs
(lgc_test_program_create) force the kernel of each launch and end with a launch that reveals every word."""
import numpy as np
import pytest

import op_corpus as oc
import word_model as wm

pytestmark = pytest.mark.gpu

OP = wm.OP
SEED = bytes(range(31, 47))
GENERIC = ("split", "quad2", "wide")


def _run(lgc, C, modes):
    prog = C.program(lgc, modes)
    s = lgc.RecordSolver(prog, seed=SEED)
    s.set_inputs(np.array(C.inputs, dtype=np.uint64))
    s.run()
    got = [int(v) for v in s.reveal()]
    s.close()
    return prog, got


def _check(lgc, gccpu, oracle, C, modes, what):
    prog, got = _run(lgc, C, modes)
    # the forced kernels are the kernels the solver ran
    mg, me = prog.modes()
    for i, (kind, _) in enumerate(C.launches):
        g, e = modes(kind)
        if g != "auto":
            assert mg[i] == lgc.LM[g] and me[i] == lgc.LM[e], (what, i, mg[i], me[i])
    plain = oc.plain_words(gccpu, prog, C)
    bad = oc.mismatches(C, got, plain)
    assert not bad, "%s, kernel against the plaintext machine:\n%s" % (what, "\n".join(bad))
    dec, cs, opaque = oc.model_words(oracle, C)
    bad = oc.mismatches(C, got, dec, cs, opaque)
    assert not bad, "%s, kernel against the model:\n%s" % (what, "\n".join(bad))


def _precs(w):
    return (1, w - 8, w - 1)


@pytest.mark.parametrize("w", [32, 64])
@pytest.mark.parametrize("kernel", GENERIC)
def test_every_op_on_generic_kernels(lgc, gccpu, oracle, w, kernel):
    """all ops valid at w, MAC records included, in one launch per op group on the forced kernel, both roles"""
    for p in _precs(w):
        C = oc.build(w, p, n_rand=24)
        _check(lgc, gccpu, oracle, C, lambda kind: (kernel, kernel), "w=%d p=%d kernel=%s" % (w, p, kernel))


@pytest.mark.parametrize("w", [32, 64])
def test_mac_ops_on_mac_kernels(lgc, gccpu, oracle, w):
    """OP_MAC / OP_MAC2 in the MAC kernel, OP_MACK (hdiff words made by an OP_HDIFF launch before it) in the MACK kernel"""
    for p in _precs(w):
        C = oc.build(w, p, sections=("mac", "mac2"))
        _check(lgc, gccpu, oracle, C, lambda kind: ("mac", "mac") if kind == "mac" else ("auto", "auto"),
               "w=%d p=%d kernel=MAC" % (w, p))
        if w == 64:
            C = oc.build(w, p, sections=("mack",))
            _check(lgc, gccpu, oracle, C, lambda kind: ("mack", "mack") if kind == "mack" else ("auto", "auto"),
                   "w=%d p=%d kernel=MACK" % (w, p))


@pytest.mark.parametrize("w", [32, 64])
@pytest.mark.parametrize("g,e", [("split", "quad2"), ("quad2", "split")])
def test_cross_role_pairs(lgc, gccpu, oracle, w, g, e):
    """a garbler on one latency kernel, the evaluator on the other: the divider, the square root, PROX and EQ"""
    C = oc.build(w, w - 8, n_rand=8, sections=("binary", "unary", "lasso"))
    _check(lgc, gccpu, oracle, C, lambda kind: (g, e), "w=%d garbler=%s evaluator=%s" % (w, g, e))


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _geometry_corpus(w, p, op, sizes, rng):
    """one launch per size of cheap records with distinct inputs, each record with outputs of its own"""
    n_in = sum(2 * n for n in sizes)
    C = oc.Corpus(w, p, n_in)
    m = wm.mask(w)
    lay = []
    for n in sizes:
        a = [(i * 0x9E3779B97F4A7C15 + 7) & m for i in range(n)]
        b = [int(x) & m for x in rng.integers(0, 1 << 62, n, dtype=np.uint64)]
        lay.append((C.inp(a), C.inp(b), n))
    for ia, ib, n in lay:
        if op == "ADD":
            o = C.out(n)
            C.launch("gen", [(OP["ADD"], 1, o + i, ia + i, ib + i, 0, 1, 1) for i in range(n)], ["record %d of %d" % (i, n) for i in range(n)])
        elif op == "MAC":
            o = C.out(2 * n)
            C.launch("mac", [(OP["MAC"], 1, o + 2 * i, ia + i, ib + i, 0, 1, 1) for i in range(n)], ["record %d of %d" % (i, n) for i in range(n)])
        else:   # OP_MACK with cnt = 2: products (a_i, b_i) and (a_i+1, b_i+1), the hdiff words made first
            hd = C.out(2 * n)
            C.launch("gen", [(OP["HDIFF"], 1, hd + i, ia + i, 0, 0, 1, 1) for i in range(n)] +
                     [(OP["HDIFF"], 1, hd + n + i, ib + i, 0, 0, 1, 1) for i in range(n)])
            o = C.out(2 * (n - 1))
            C.launch("mack", [(OP["MACK"], 2, o + 2 * i, ia + i, ib + i, hd - ia, 1, 1) for i in range(n - 1)],
                     ["record %d of %d" % (i, n - 1) for i in range(n - 1)])
    return C


def _expected_mode(lgc, kind, n):
    c = lgc.launch_constants()
    if kind in ("mac", "mack") and n >= c["narrow_mac"]:
        return lgc.LM[kind]
    if n >= c["wide_launch"]:
        return lgc.LM["wide"]
    return lgc.LM["split"] if n <= c["split_max_recs"] else lgc.LM["quad2"]


@pytest.mark.parametrize("op,w", [("ADD", 64), ("MAC", 32), ("MACK", 64)])
def test_launch_geometry(lgc, gccpu, oracle, op, w):
    """launches at the record counts where the kernel or its geometry changes, in automatic mode: every record's own
    output is right (a record skipped or run twice shows), and each launch ran on the kernel its size implies"""
    cus = _cus()
    sizes = [1, 255, 256, 257, 519, 520, 521, 1023, 1024, 1025, 12 * cus - 1, 12 * cus + 1, 16 * cus - 1, 16 * cus + 1]
    if op == "MAC":
        sizes += [3 * 16 * cus + 7, 2 * 16 * cus * 2 + 5]
    if op == "MACK":
        sizes = [n + 1 for n in sizes]          # (n - 1 OP_MACK records from n operand pairs)
    C = _geometry_corpus(w, w - 8, op, sizes, np.random.default_rng(5))
    prog, got = _run(lgc, C, lambda kind: ("auto", "auto"))
    mg, me = prog.modes()
    for i, (kind, rs) in enumerate(C.launches):
        want = _expected_mode(lgc, kind, len(rs))
        assert mg[i] == want and me[i] == want, (op, len(rs), mg[i], me[i], want)
    assert not oc.mismatches(C, got, oc.plain_words(gccpu, prog, C), limit=4), op
    dec, cs, opaque = oc.model_words(oracle, C)
    bad = oc.mismatches(C, got, dec, cs, opaque)
    assert not bad, "%s geometry:\n%s" % (op, "\n".join(bad))


@pytest.mark.parametrize("w", [32, 64])
def test_chained_kernels(lgc, gccpu, oracle, w):
    """SPLIT -> WIDE -> MAC -> QUAD2, words handed from launch to launch: x = a b; y = x - c; (S, C) = sum of three y; z = S + C"""
    p, n = w - 8, 96
    rng = np.random.default_rng(9)
    a, b = oc.edge_operands(rng, w, n)
    C = oc.Corpus(w, p, 3 * n)
    ia, ib, ic = C.inp(a[-n:]), C.inp(b[-n:]), C.inp(a[:n])
    x, y, sc, z = C.out(n), C.out(n), C.out(2 * (n - 2)), C.out(n - 2)
    C.launch("gen", [(OP["MUL"], 1, x + i, ia + i, ib + i, 0, 1, 1) for i in range(n)])
    C.launch("gen2", [(OP["SUB"], 1, y + i, x + i, ic + i, 0, 1, 1) for i in range(n)])
    C.launch("mac", [(OP["MAC"], 3, sc + 2 * i, y + i, x + n - 1 - i, 0, 1, -1) for i in range(n - 2)])
    C.launch("gen3", [(OP["ADD"], 1, z + i, sc + 2 * i, sc + 2 * i + 1, 0, 1, 1) for i in range(n - 2)])
    K = {"gen": "split", "gen2": "wide", "mac": "mac", "gen3": "quad2"}
    _check(lgc, gccpu, oracle, C, lambda kind: (K[kind], K[kind]), "w=%d chain" % w)
