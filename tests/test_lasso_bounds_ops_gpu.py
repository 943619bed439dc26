"""The bounded OP_PROX record (bit 31 of cnt) on every generic record kernel, forced, both roles, and with the garbler and the
evaluator on different kernels: against the CPU checker's plaintext machine and the record model of
tests/lasso_bounds_model.py, on the edge operands of its corpus."""
import numpy as np
import pytest

import lasso_bounds_model as lbm
import op_corpus as oc
import test_lasso_bounds_ops_cpu as cpu

pytestmark = pytest.mark.gpu

SEED = bytes(range(41, 57))


def _check(lgc, gccpu, C, g, e, what):
    prog = C.program(lgc, lambda kind: (g, e))
    mg, me = prog.modes()
    assert mg[0] == lgc.LM[g] and me[0] == lgc.LM[e], what
    s = lgc.RecordSolver(prog, seed=SEED)
    s.set_inputs(np.array(C.inputs, dtype=np.uint64))
    s.run()
    got = [int(v) for v in s.reveal()]
    s.close()
    plain = oc.plain_words(gccpu, prog, C)
    assert got[:len(plain)] == plain, what
    bad = cpu._mismatches(C, got, lbm.corpus_words(C))
    assert not bad, (what, bad)


@pytest.mark.parametrize("w", [32, 64])
@pytest.mark.parametrize("kernel", ["split", "quad2", "wide"])
def test_flagged_prox_on_generic_kernels(lgc, gccpu, w, kernel):
    for p in (1, w - 8, w - 1):
        C = lbm.bounds_corpus(w, p, np.random.default_rng([w, p, 3]))
        _check(lgc, gccpu, C, kernel, kernel, "w=%d p=%d kernel=%s" % (w, p, kernel))


@pytest.mark.parametrize("w", [32, 64])
@pytest.mark.parametrize("g,e", [("split", "quad2"), ("quad2", "split")])
def test_flagged_prox_cross_role(lgc, gccpu, w, g, e):
    C = lbm.bounds_corpus(w, w - 8, np.random.default_rng([w, 4]))
    _check(lgc, gccpu, C, g, e, "w=%d garbler=%s evaluator=%s" % (w, g, e))
