"""The two-records-per-workgroup form of the column-split kernel (LM_SPLIT2) against the 4-wave kernel (LM_QUAD2), on the GPU:
a launch garbled in either form must be evaluable in the other, and both forms must leave the same bits behind.

For every op and launch size, runs of the same records, inputs and seed with the kernel forced per role -- garbler /
evaluator: new / new, new / old, old / new, old / old, and the 16-wave column-split kernel on both sides -- and the whole word
file of each role and the launch's garbled table are compared with the old / old run bit for bit, no tolerance.

One thing about the table: the 4-wave garbler stores the rows of a step's ACTIVE gates only and leaves the other lanes of the
step as its table ring held them (rings are parked and reused between solvers), while the table pass of a column-split
garbler (gc_tabfill_kernel, the same for the 16-wave and the new form) writes every lane: zeros where the gate is inactive,
and zeros too for the few active gates whose two operands are both the constant-zero label, rows no evaluator ever uses
(its colour bits select neither).  So the new form's table is compared in full, every byte, with the tables of the other
new-form garbler and of the existing 16-wave column-split garbler forced on the same launch -- which fixes the set of rows
that are written at all -- and with the 4-wave garbler's on every gate whose rows it holds."""
import os
import subprocess
import sys

import numpy as np
import pytest

import word_model as wm

pytestmark = pytest.mark.gpu

OP = wm.OP
SEED = bytes(range(7, 23))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# op, width, precision, cnt: whole additions walked by the hash waves (the dividers), posted dual steps (the multiplier),
# a max tree of fan-in 8, a lone addition, and the 32-lane additions of the 32-bit divider
CASES = [("DIVB", 64, 56, 1), ("DIV", 64, 56, 1), ("MUL", 64, 56, 1), ("MAX", 64, 56, 8), ("ADD", 64, 56, 1), ("DIV", 32, 24, 1)]
SIZES = [257, 258, 512]          # an odd last workgroup, a full pair, the upper edge of the mode


def _program(lgc, op, w, p, cnt, n, g, e):
    """n records of `op` in one launch, record i with operands and an output word of its own"""
    rng = np.random.default_rng(1000 * n + 10 * OP[op] + w)
    m = (1 << w) - 1
    a = [int(x) & m for x in rng.integers(0, 1 << 63, n + cnt, dtype=np.uint64) * 2 + rng.integers(0, 2, n + cnt, dtype=np.uint64)]
    b = [int(x) & m for x in rng.integers(0, 1 << 63, n, dtype=np.uint64) * 2 + rng.integers(0, 2, n, dtype=np.uint64)]
    if op == "DIVB":             # the program guarantees |a| <= |b|
        mag = lambda v: abs(wm.s(v, w))
        for i in range(n):
            if mag(a[i]) > mag(b[i]):
                a[i], b[i] = b[i], a[i]
            if b[i] == 0:
                b[i] = 1
    ia, ib = 1, 1 + len(a)
    out = ib + len(b)
    if op == "MAX":
        recs = [(OP[op], cnt, out + i, ia + i, i & 1, 0, 1, 1) for i in range(n)]      # words a_i .. a_i+7, signed / unsigned
    else:
        recs = [(OP[op], cnt, out + i, ia + i, ib + i, 0, 1, 1) for i in range(n)]
    prog = lgc.RecordProgram(w, p, recs, [n], [g], [e], n_inputs=len(a) + len(b), n_words=out + n)
    assert prog.modes() == ([lgc.LM[g]], [lgc.LM[e]])
    return prog, np.array(a + b, dtype=np.uint64)


def _run(lgc, op, w, p, cnt, n, g, e):
    prog, inputs = _program(lgc, op, w, p, cnt, n, g, e)
    s = lgc.RecordSolver(prog, seed=SEED)
    try:
        s.set_inputs(inputs)
        s.run()
        nw = prog.info.n_words
        return prog.launches()[0], s.word_labels(True, 0, nw), s.word_labels(False, 0, nw), s.tables(0)
    finally:
        s.close()


def _gates(tab):
    """(steps, 2, 64, 2) uint64 view of a table: step, TG | TE, lane, label half"""
    return tab.view(np.uint64).reshape(tab.shape[0], 2, 64, 2)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op,w,p,cnt", CASES)
def test_new_and_old_forms_are_interchangeable(lgc, op, w, p, cnt, n):
    L, ref_g, ref_e, ref_tab = _run(lgc, op, w, p, cnt, n, "quad2", "quad2")
    assert L["nrec"] == n and L["steps"] > 0
    # the evaluator holds one of the garbler's two labels on every wire: the reference run did compute something
    assert ref_g.any() and ref_e.any() and not np.array_equal(ref_g, ref_e)
    new_tab = None
    for g, e in (("split2", "split2"), ("split2", "quad2"), ("quad2", "split2"), ("split", "split")):
        what = "%s w=%d n=%d garbler=%s evaluator=%s" % (op, w, n, g, e)
        _, wg, we, tab = _run(lgc, op, w, p, cnt, n, g, e)
        assert np.array_equal(wg, ref_g), what + ": the garbler's word file"
        assert np.array_equal(we, ref_e), what + ": the evaluator's word file"
        if g != "quad2":
            if new_tab is None:
                new_tab = tab
                act = (_gates(new_tab) != 0).any(axis=(1, 3))                       # (steps, 64): the gate's rows are not zero
                # (all active gates but those of two constant operands: a handful per record)
                assert L["gates"] - 8 * n <= int(act.sum()) <= L["gates"], what + ": gates with rows in the table"
                same = (_gates(new_tab) == _gates(ref_tab)).all(axis=(1, 3))
                assert same[act].all(), what + ": table rows of the active gates against the 4-wave garbler's"
            else:
                assert np.array_equal(tab, new_tab), what + ": the table, every byte"
        else:
            same = (_gates(tab) == _gates(ref_tab)).all(axis=(1, 3))
            assert same[act].all(), what + ": table rows of the active gates"
        del tab


def test_small_solve_unchanged(golden_dir, tmp_path):
    """d = 20 CGD-3 through bench.py (every launch has at most 256 records: none reaches the new form): beta is, word for
    word, what the build before this mode dumped (tests/golden/split2_d20_cgd3_*.npy, written by the same command there)"""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--d", "20", "--iters", "3", "--steps", "1",
                        "--warmup", "0", "--dump-outputs", str(out)], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    for name in ("beta", "beta_fixed_hi", "beta_fixed_lo"):
        got = np.load(str(out / (name + ".npy")))
        want = np.load(os.path.join(golden_dir, "split2_d20_cgd3_%s.npy" % name))
        assert got.shape == (20,) and np.array_equal(got, want), name
