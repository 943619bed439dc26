"""The two-records-per-workgroup form of the column-split kernel (LM_SPLIT2): which launches get it by record count, and the
geometry it is dispatched with (lgc_test_launch_shape).  Host only."""
import pytest

import linreg_gc
import word_model as wm

OP = wm.OP
K = linreg_gc.LM
SIZES = [256, 257, 258, 511, 512, 513]


def _prog(op, n, w=64, p=56, cnt=1):
    """one launch of n records of `op`, kernels by record count"""
    return linreg_gc.RecordProgram(w, p, [(OP[op], cnt, 3, 1, 2, 0, 1, 1)] * n, [n], n_inputs=2 + cnt, n_words=8 + cnt)


def _want(n, split_on):
    c = linreg_gc.launch_constants()
    assert (c["split_max_recs"], c["wide_launch"]) == (256, 520)
    if not split_on or n > 2 * c["split_max_recs"]:
        return K["quad2"]
    return K["split"] if n <= c["split_max_recs"] else K["split2"]


@pytest.mark.parametrize("g_on,e_on", [(True, True), (False, True), (True, False), (False, False)])
def test_mode_by_record_count(g_on, e_on):
    """deep records (the 64-bit dividers): 256 -> SPLIT, 257 .. 512 -> SPLIT2, 513 -> QUAD2, per role; a role whose split
    kernels are switched off runs the 4-wave kernel at every one of these sizes"""
    linreg_gc.set_split_kernels(g_on, e_on)
    try:
        for op in ("DIVB", "DIV"):
            for n in SIZES:
                assert _prog(op, n).modes() == ([_want(n, g_on)], [_want(n, e_on)]), (op, n)
    finally:
        linreg_gc.set_split_kernels(True, True)


def test_shallow_and_mac_launches_keep_the_four_wave_kernel():
    """the mode is for deep chains of additions: launches below split2_min_steps gate steps per record, and
    multiply-accumulate launches of any depth, run as before"""
    c = linreg_gc.launch_constants()
    for op, w, p, cnt in (("ADD", 64, 56, 1), ("MUL", 64, 56, 1), ("MAX", 64, 56, 8), ("DIV", 32, 24, 1), ("MAC", 64, 56, 6)):
        for n in (257, 512):
            prog = _prog(op, n, w, p, cnt)
            L = prog.launches()[0]
            assert L["mac_only"] or L["steps"] < c["split2_min_steps"] * n, (op, L)
            assert prog.modes() == ([K["quad2"]], [K["quad2"]]), (op, n)
    for op in ("SQRT", "DIVB", "DIV"):
        L = _prog(op, 257).launches()[0]
        assert not L["mac_only"] and L["steps"] >= c["split2_min_steps"] * 257, (op, L)


@pytest.mark.parametrize("garbler", [True, False])
@pytest.mark.parametrize("cus", [1, 256, 304])
def test_shape(garbler, cus):
    """two records per workgroup of 1024 threads whatever the device; an odd last workgroup holds one record"""
    for n in SIZES + [1, 2, 3, 1536]:
        grid, threads, per_wg, bound = linreg_gc.launch_shape("split2", garbler, n, cus)
        assert (grid, threads, per_wg, bound) == ((n + 1) // 2, 1024, 2, 1024), n
        assert (grid - 1) * per_wg < n <= grid * per_wg
    assert linreg_gc.launch_shape("split2", garbler, 257, cus)[0] == 129          # 128 pairs and one single record
    assert linreg_gc.launch_shape("split", garbler, 256, cus)[:3] == (256, 1024, 1)
    assert linreg_gc.launch_shape("quad2", garbler, 513, cus)[:3] == (513, 256, 1)


def test_forced_mode_is_accepted_and_pairs_with_the_latency_kernels():
    """Launch::force can name the mode per role; it numbers its gate steps as SPLIT and QUAD2 do, not as WIDE does"""
    for g, e in (("split2", "split2"), ("split2", "quad2"), ("quad2", "split2"), ("split2", "split"), ("split", "split2")):
        prog = linreg_gc.RecordProgram(64, 56, [(OP["ADD"], 1, 3, 1, 2, 0, 1, 1)] * 3, [3], [g], [e], n_inputs=2, n_words=5)
        assert prog.modes() == ([K[g]], [K[e]])
    with pytest.raises(linreg_gc.LgcError, match="number the gate steps differently"):
        linreg_gc.RecordProgram(64, 56, [(OP["ADD"], 1, 3, 1, 2, 0, 1, 1)], [1], ["split2"], ["wide"], n_inputs=2, n_words=5)
    with pytest.raises(linreg_gc.LgcError, match="unknown kernel"):
        linreg_gc.RecordProgram(64, 56, [(OP["ADD"], 1, 3, 1, 2, 0, 1, 1)], [1], [16], [0], n_inputs=2, n_words=5)
