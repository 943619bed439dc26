"""Every record op against the integer model (word_model.py) on the CPU, the rejections of the test-program hook
(lgc_test_program_create) and the launch geometry of every record kernel (lgc_test_launch_shape)."""
import numpy as np
import pytest

import linreg_gc
import op_corpus as oc
import word_model as wm

OP = wm.OP
PRECS = {64: [1, 56, 63], 32: [1, 24, 31]}


@pytest.mark.parametrize("w", [64, 32])
def test_corpus_plain_matches_model(gccpu, oracle, w):
    """the plaintext machine (the circuits) against the model, every op valid at w, bit for bit"""
    for p in PRECS[w]:
        C = oc.build(w, p)
        ops = {r[0] for _, rs in C.launches for r in rs}
        assert ops == set(range(1, len(wm.OPS))) - (wm.ONLY32 if w == 64 else wm.ONLY64) - {OP["REVEAL"]}, sorted(ops)
        prog = C.program(linreg_gc, lambda kind: ("auto", "auto"))
        dec, cs, opaque = oc.model_words(oracle, C)
        bad = oc.mismatches(C, oc.plain_words(gccpu, prog, C), dec, cs, opaque)
        assert not bad, "w=%d p=%d:\n%s" % (w, p, "\n".join(bad))


@pytest.mark.parametrize("w,p", [(64, 56), (32, 24)])
def test_corpus_garble_eval_matches_plain(gccpu, w, p):
    """the CPU garbler + evaluator on a test program (a small corpus) decode what the plaintext machine computes"""
    C = oc.build(w, p, n_rand=4, sections=("binary", "unary", "lasso", "mac", "mac2", "mack"))
    prog = C.program(linreg_gc, lambda kind: ("auto", "auto"))
    got, gates, _ = gccpu.garble_eval(prog, np.array(C.inputs, dtype=np.uint64))
    assert gates == prog.info.total_gates
    m = wm.mask(w)
    bad = oc.mismatches(C, [int(v) & m for v in got[:prog.info.n_reveal]], oc.plain_words(gccpu, prog, C))
    assert not bad, "\n".join(bad)


def test_model_knows_the_op_list():
    """word_model's op numbering is gc_exec.h's: the hook accepts the last op and rejects the next number"""
    rec = (OP["PROX"], 0, 4, 1, 0, 1, 1, 0)
    linreg_gc.RecordProgram(64, 56, [rec], [1], n_inputs=3, n_words=6, n_reveal=0)
    with pytest.raises(linreg_gc.LgcError, match="is not an op"):
        linreg_gc.RecordProgram(64, 56, [(len(wm.OPS),) + rec[1:]], [1], n_inputs=3, n_words=6, n_reveal=0)


def _rejects(msg, *a, **k):
    with pytest.raises(linreg_gc.LgcError, match=msg) as e:
        linreg_gc.RecordProgram(*a, **k)
    assert e.value.code == -1      # LGC_EINVAL


ADD = (OP["ADD"], 1, 3, 1, 2, 0, 1, 1)
MAC = (OP["MAC"], 1, 3, 1, 2, 0, 1, 1)
MACK = (OP["MACK"], 1, 3, 1, 2, 0, 1, 1)


def test_rejections():
    R = _rejects
    R("is not an op", 64, 56, [(99, 1, 3, 1, 2, 0, 1, 1)], [1], n_inputs=2, n_words=5)
    R("OP_MAC2 is a 32-bit op", 64, 56, [(OP["MAC2"], 1, 3, 1, 2, 0, 1, 1)], [1], n_inputs=2, n_words=8)
    for op in ("MACK", "HDIFF", "DIVB"):
        R("is a 64-bit op", 32, 24, [(OP[op], 1, 3, 1, 2, 0, 1, 1)], [1], n_inputs=2, n_words=8)
    # footprints: destinations, operands, strides, side outputs, reveal slots
    R("touches word 5, outside n_words = 5", 64, 56, [(OP["ADD"], 1, 5, 1, 2, 0, 1, 1)], [1], n_inputs=2, n_words=5)
    R("touches word 9, outside", 64, 56, [(OP["SUM"], 4, 3, 0, 0, 0, 3, 1)], [1], n_inputs=2, n_words=9)
    R("touches word 4294967295", 64, 56, [(OP["SUM"], 2, 3, 0, 0, 0, -1, 1)], [1], n_inputs=2, n_words=9)
    R("touches word 4, outside", 64, 56, [MAC], [1], n_inputs=2, n_words=4)
    R("touches word", 64, 56, [(OP["MUL"], 2, 3, 1, 2, 0, 10, 1)], [1], n_inputs=2, n_words=8)
    R("touches word", 64, 56, [(OP["DIV"], 1, 3, 1, 2, 40, 1, 1)], [1], n_inputs=2, n_words=8)
    R("touches word", 64, 56, [(OP["MACK"], 1, 3, 1, 2, 9, 1, 1)], [1], n_inputs=2, n_words=8)
    R("touches word", 64, 56, [(OP["PROX"], 0, 4, 1, 0, 6, 1, 0)], [1], n_inputs=3, n_words=8)
    R("reveals to slot 3, outside n_reveal = 3", 64, 56, [(OP["REVEAL"], 1, 3, 1, 0, 0, 1, 1)], [1], n_inputs=2, n_words=4,
      n_reveal=3)
    # forced kernels
    R("the MAC kernel runs MAC-only launches", 64, 56, [ADD], [1], ["mac"], ["mac"], n_inputs=2, n_words=5)
    R("the MACK kernel runs MAC-only launches", 64, 56, [ADD], [1], ["auto"], ["mack"], n_inputs=2, n_words=5)
    R("the MACK kernel cannot run OP_MAC", 64, 56, [MAC], [1], ["mack"], ["mack"], n_inputs=2, n_words=5)
    R("the MAC kernel cannot run OP_MACK", 64, 56, [MACK], [1], ["mac"], ["mac"], n_inputs=2, n_words=5)
    R("garbler SPLIT and evaluator WIDE number the gate steps differently", 64, 56, [ADD], [1], ["split"], ["wide"],
      n_inputs=2, n_words=5)
    R("garbler MAC and evaluator QUAD2", 64, 56, [MAC], [1], ["mac"], ["quad2"], n_inputs=2, n_words=5)
    R("garbler WIDE and evaluator SPLIT", 64, 56, [ADD], [1], ["wide"], ["auto"], n_inputs=2, n_words=5)
    R("unknown kernel", 64, 56, [ADD], [1], [6], [0], n_inputs=2, n_words=5)
    # launches the lowering would split, and malformed programs
    R("mixes MAC records", 64, 56, [MAC, ADD], [2], n_inputs=2, n_words=6)
    R("mixes MAC records", 64, 56, [MAC, MACK], [2], n_inputs=2, n_words=6)
    R("the launches hold 1 records, not n_records = 2", 64, 56, [ADD, ADD], [1], n_inputs=2, n_words=5)
    R("has no records", 64, 56, [ADD], [1, 0], n_inputs=2, n_words=5)
    R("input words at word 1 do not fit", 64, 56, [ADD], [1], n_inputs=5, n_words=5)
    R("width must be 32 or 64", 48, 20, [ADD], [1], n_inputs=2, n_words=5)
    R("precision must satisfy", 32, 32, [ADD], [1], n_inputs=2, n_words=5)


def test_accepted_pairs_and_modes():
    """SPLIT x QUAD2 both ways (production pairs them when the split kernel is switched off for one role), forced kernels
    are what the solver runs, auto follows the record count"""
    K = linreg_gc.LM
    for g, e in (("split", "quad2"), ("quad2", "split"), ("wide", "wide"), ("mac", "wide"), ("wide", "mac")):
        rec = MAC if "mac" in (g, e) else ADD
        prog = linreg_gc.RecordProgram(64, 56, [rec, rec], [1, 1], [g, "auto"], [e, "auto"], n_inputs=2, n_words=5)
        mg, me = prog.modes()
        assert (mg[0], me[0]) == (K[g], K[e])
        assert mg[1] == me[1] == K["split"]
    c = linreg_gc.launch_constants()
    for n, want in ((1, "split"), (c["split_max_recs"], "split"), (c["split_max_recs"] + 1, "quad2"),
                    (c["wide_launch"] - 1, "quad2"), (c["wide_launch"], "wide")):
        prog = linreg_gc.RecordProgram(32, 24, [ADD] * n, [n], n_inputs=2, n_words=5)
        assert prog.modes() == ([K[want]], [K[want]]), n
    for n, want in ((c["narrow_mac"] - 1, "wide"), (c["narrow_mac"], "mac")):
        prog = linreg_gc.RecordProgram(32, 24, [MAC] * n, [n], n_inputs=2, n_words=5)
        assert prog.modes() == ([K[want]], [K[want]]), n
    prog = linreg_gc.RecordProgram(64, 56, [MACK] * c["narrow_mac"], [c["narrow_mac"]], n_inputs=2, n_words=5)
    assert prog.modes() == ([K["mack"]], [K["mack"]])


def test_program_accounting():
    """step0 / steps / gates of a test program are the lowering's: consecutive records, launches cover them"""
    C = oc.build(64, 56, n_rand=4)
    prog = C.program(linreg_gc, lambda kind: ("auto", "auto"))
    L = prog.launches()
    assert sum(x["nrec"] for x in L) == prog.info.n_records
    for a, b in zip(L, L[1:]):
        assert b["first_rec"] == a["first_rec"] + a["nrec"] and b["step0"] == a["step0"] + a["steps"]
    assert [x["mac_only"] for x in L] == [int(k != "gen") for k, _ in C.launches] + [0]


CUS = [1, 80, 104, 256, 304]


def _nrecs(cus, c):
    n = set(range(1, 20001))
    for waves in range(c["mac_adapt_lo"], 17):
        unit = cus * waves * c["mac_chunk"]
        for k in range(1, 9):
            for d in (-2, -1, 0, 1, 2):
                if k * unit + d > 0:
                    n.add(k * unit + d)
                    n.add(k * unit // 2 + d)
    return np.array(sorted(n), dtype=np.int64)


@pytest.mark.parametrize("cus", CUS)
def test_launch_shape_covers_every_record_once(cus):
    c = linreg_gc.launch_constants()
    for mode in ("mac", "mack", "wide", "split", "quad2"):
        for g in (True, False):
            for n in _nrecs(cus, c):
                grid, threads, per_wg, bound = linreg_gc.launch_shape(mode, g, int(n), cus)
                assert (grid - 1) * per_wg < n <= grid * per_wg, (mode, g, cus, n, grid, per_wg)
                assert threads % 64 == 0 and 64 <= threads <= bound, (mode, g, cus, n, threads, bound)
                if mode in ("mac", "mack"):
                    assert c["mac_adapt_lo"] <= threads // 64 <= bound // 64, (mode, g, cus, n, threads)
                    assert per_wg >= threads // 64 or per_wg == n, (mode, g, cus, n, per_wg, threads)
                elif mode == "wide":
                    assert per_wg == threads // 64
                else:
                    assert per_wg == 1 and grid == n
