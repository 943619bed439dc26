"""The Karatsuba MAC kernel's partial-product rows share AES lookups between the rows of an array (row_hash) and the lanes
of a half wave (hash_lu): the two forms on the device against the plain gate hash at tweaks no small program reaches
(lgc_row_hash_eval), and OP_MACK programs whose arrays straddle the gate steps at which the cached part must be refilled."""
import os

import numpy as np
import pytest

import op_corpus as oc
import word_model as wm
from helpers import edge_operands

pytestmark = pytest.mark.gpu

OP = wm.OP
SEED = bytes(range(31, 47))
# first gate step of an array: row 0 at step s0, row i at s0 + 2 i - 1 (the host tool runs the same cases)
STARTS = [int(l.split()[0]) for l in open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rowhash_starts.txt"))
          if l.strip() and not l.startswith("#")]


def test_row_and_lane_uniform_hashes_on_device(lgc, gccpu):
    rng = np.random.default_rng(21)
    items, labels, tweaks = [], [], []
    for s0 in STARTS:
        for h in (0, 1):
            x = rng.integers(0, 256, size=16, dtype=np.uint8)
            xr = x.reshape(4, 4)[::-1].reshape(16)            # the four 32-bit words in reverse order
            # one row at stride 128, then 32 rows at stride 256: the same label, so the cache lives on
            items.append((x.tobytes(), 128 * s0 + h, 128, 1))
            items.append((x.tobytes(), 128 * (s0 + 1) + h, 256, 32))
            for T in [128 * s0 + h] + [128 * (s0 + 1) + h + 256 * r for r in range(32)]:
                for form in (0, 1):
                    for lane in range(64):
                        labels.append(xr if form == 1 and lane >= 32 else x)
                        tweaks.append(T + 2 * lane)
    got = lgc.row_hash_eval(items).reshape(-1, 16)
    labels = np.array(labels, dtype=np.uint8)
    tweaks = np.array(tweaks, dtype=np.uint64)
    assert len(got) == len(labels) == len(STARTS) * 2 * 33 * 128
    cpu = gccpu.gate_hash(labels, tweaks)
    dev = lgc.gate_hash_eval(labels, tweaks)
    assert np.array_equal(dev, cpu)
    bad = np.flatnonzero((got != cpu).any(axis=1))
    assert bad.size == 0, "first mismatches (row, form, lane): %s" % [(int(i) // 128, int(i) // 64 % 2, int(i) % 64) for i in bad[:8]]


def _mack_corpus(w, p, cnts, rng, pad=0):
    """one launch of OP_MACK records with the given product counts over a vector of 24 edge and random operands; the
    OP_HDIFF launch in front of it (15 gate steps per record) makes the hdiff words, `pad` more records of it write the same differences to words of their own"""
    v = [int(x) for x in edge_operands(rng, w, 520)[0][::26]] + [int(x) for x in rng.integers(0, 1 << 63, 4, dtype=np.uint64) * 2 + 1]
    def once(n_inputs):
        C = oc.Corpus(w, p, n_inputs)
        iv = C.inp(v)
        hd = C.out(len(v))
        extra = C.out(pad)                                   # (a word is written by ONE record of a launch: they run in parallel)
        C.launch("gen", [(OP["HDIFF"], 1, hd + i, iv + i, 0, 0, 1, 1) for i in range(len(v))] +
                 [(OP["HDIFF"], 1, extra + i, iv + i % len(v), 0, 0, 1, 1) for i in range(pad)])
        recs = []
        for i, cnt in enumerate(cnts):
            o = C.out(2)
            recs.append((OP["MACK"], cnt, o, iv + (5 * i) % (len(v) - 3), iv + (7 * i + 1) % (len(v) - 3), hd - iv, 1, 1))
        C.launch("mack", recs, ["record %d cnt=%d" % (i, c) for i, c in enumerate(cnts)])
        return C
    return once(len(once(None).inputs))


def _array_starts(prog, C):
    """first gate step of every 32 x 32 array of the OP_MACK launch: three per pair of products, 63 steps each"""
    recs = np.frombuffer(prog.records(), dtype=np.uint8).reshape(-1, 40)
    step0 = recs[:, 32:40].copy().view(np.uint64).reshape(-1)
    first = len(C.launches[0][1])
    cnts = [r[1] for r in C.launches[1][1]]
    out = []
    for i, cnt in enumerate(cnts):
        pairs = (cnt + 1) // 2
        per_pair = (int(step0[first + i + 1]) - int(step0[first + i])) // pairs
        out += [int(step0[first + i]) + k * per_pair + 63 * t for k in range(pairs) for t in range(3)]
    return out


def _crossed(starts, m):
    """does a row of some array (steps s, s + 1, s + 3, ..., s + 61) follow a multiple of m that its predecessor precedes"""
    return any(s // m != (s + 61) // m for s in starts)


def _cpu_mirror(gccpu, prog, inputs, k):
    """The CPU checker's garbler and evaluator on the program, launch by launch as GcCpu.garble_eval runs them: the
    decoded words, the garbled table of launch k (steps, 2, 64, 16) and both roles' word files (n_words, 64, 16)."""
    info, w, p = prog.info, prog.system.width, prog.system.precision
    recs = prog.records()
    R = gccpu.derive_R(SEED)
    ptr = lambda a: a.ctypes.data
    wordsG = np.zeros(info.n_words * 1024, dtype=np.uint8)
    wordsE = np.zeros(info.n_words * 1024, dtype=np.uint8)
    shares = np.ascontiguousarray(inputs, dtype=np.uint64).ravel()
    gccpu.lib.gcc_input_labels(SEED, ptr(R), ptr(shares), info.in_base, shares.size, w, ptr(wordsG), ptr(wordsE))
    decG = np.zeros(info.n_reveal + 1, dtype=np.uint64)
    decE = np.zeros(info.n_reveal + 1, dtype=np.uint64)
    tab_k = None
    for i, L in enumerate(prog.launches()):
        tab = np.zeros(max(1, L["steps"]) * 2048, dtype=np.uint8)
        sl = recs[L["first_rec"] * 40:(L["first_rec"] + L["nrec"]) * 40]
        g = gccpu.lib.gcc_garble_run(ptr(sl), L["nrec"], w, p, ptr(R), ptr(wordsG), ptr(tab), ptr(decG), L["step0"])
        e = gccpu.lib.gcc_eval_run(ptr(sl), L["nrec"], w, p, ptr(wordsE), ptr(tab), ptr(decE), L["step0"])
        assert g == e == L["gates"]
        if i == k:
            tab_k = tab[:L["steps"] * 2048].reshape(-1, 2, 64, 16)
    return decG ^ decE, tab_k, wordsG.reshape(-1, 64, 16), wordsE.reshape(-1, 64, 16)


def _check(lgc, gccpu, oracle, C, what):
    modes = lambda kind: ("mack", "mack") if kind == "mack" else ("auto", "auto")
    prog = C.program(lgc, modes)
    mg, me = prog.modes()
    assert mg[1] == me[1] == lgc.LM["mack"]
    s = lgc.RecordSolver(prog, seed=SEED)
    s.set_inputs(np.array(C.inputs, dtype=np.uint64))
    s.run()
    got = [int(v) for v in s.reveal()]
    tab = s.tables(1)
    dst = sorted({r[2] + j for r in C.launches[1][1] for j in (0, 1)})         # (S, C) of every OP_MACK record
    lo, n = dst[0], dst[-1] - dst[0] + 1
    assert len(dst) == n
    labG, labE = s.word_labels(True, lo, n), s.word_labels(False, lo, n)
    s.close()
    bad = oc.mismatches(C, got, oc.plain_words(gccpu, prog, C))
    assert not bad, "%s, kernel against the plaintext machine:\n%s" % (what, "\n".join(bad))
    dec, cs, opaque = oc.model_words(oracle, C)
    bad = oc.mismatches(C, got, dec, cs, opaque)
    assert not bad, "%s, kernel against the model:\n%s" % (what, "\n".join(bad))
    # the CPU garbler and evaluator on the same records and seed: the same decoded words, the same garbled table of the
    # OP_MACK launch byte for byte, the same labels of its output words in both roles.  A lane that a gate step leaves
    # inactive is written by neither side (zero in the CPU's fresh buffer, whatever the ring held on the GPU): the rows
    # are compared where the CPU wrote a label, and the activity masks must have made that most of the table.
    cpu, ctab, cG, cE = _cpu_mirror(gccpu, prog, C.inputs, 1)
    assert [int(x) & wm.mask(C.w) for x in cpu[:len(got)]] == got, what
    assert np.array_equal(labG, cG[lo:lo + n]), "%s: garbler's output labels" % what
    assert np.array_equal(labE, cE[lo:lo + n]), "%s: evaluator's output labels" % what
    assert tab.shape == ctab.shape
    written = ctab.any(axis=3)
    assert written.mean() > 0.8, written.mean()
    diff = np.argwhere((tab != ctab).any(axis=3) & written)
    assert diff.size == 0, "%s: table rows differ from the CPU checker's, first (step, TG|TE, lane): %s" % (what, diff[:8].tolist())
    return prog


@pytest.mark.parametrize("p", [1, 56, 63])
def test_mack_records_across_refill_steps(lgc, gccpu, oracle, p):
    """8 records of 1, 2 and 3 products (an odd one pairs with the zero word) in one launch: arrays straddle steps 512 and 1024"""
    C = _mack_corpus(64, p, [1, 2, 3, 1, 2, 3, 3, 2], np.random.default_rng(p), pad=6)
    prog = _check(lgc, gccpu, oracle, C, "8 records, p=%d" % p)
    starts = _array_starts(prog, C)
    assert any(s + 1 < 512 <= s + 61 for s in starts) and any(s + 1 < 1024 <= s + 61 for s in starts), starts


@pytest.mark.parametrize("p", [1, 56, 63])
def test_mack_launch_across_step_2_17(lgc, gccpu, oracle, p):
    """600 records of two products: the launch crosses gate step 2^17, byte 3 of the tweak (about 260 MB of tables; the
    hdiff launch is padded so that it does at p = 1 too, where a pair has fewer steps)"""
    C = _mack_corpus(64, p, [2] * 600, np.random.default_rng(100 + p), pad=400)
    prog = _check(lgc, gccpu, oracle, C, "600 records, p=%d" % p)
    starts = _array_starts(prog, C)
    assert starts[0] < (1 << 17) < starts[-1] and _crossed(starts, 512)
