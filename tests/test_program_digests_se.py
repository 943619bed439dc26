"""The programs of include/linreg_gc_lasso_cv_se.h and its new rejections, pinned byte for byte
(tests/golden/program_digests_se.json, written by tests/golden/gen_program_digests_se.py): K = 2, 3, 5, the rule on / off, the
curve on / off, both widths, both input paths, record for record.  tests/test_program_digests.py, unchanged, is the proof that
no older program moved.  No GPU needed."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_program_digests_se", os.path.join(GOLDEN, "gen_program_digests_se.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLDEN, "program_digests_se.json")) as f:
        return json.load(f)


def test_lowered_programs_are_pinned(lgc, pinned):
    got = _gen().build_digests(lgc)
    assert sorted(got) == sorted(pinned["programs"]) and len(got) == 4 * (3 * 4 + 1)
    bad = [(name, part) for name in sorted(got) for part in ("records", "launches", "info") if got[name][part] != pinned["programs"][name][part]]
    assert not bad, bad
    assert len({v["records"] for v in got.values()}) == len(got)           # every variant is a program of its own


def test_rejections_are_pinned(lgc, pinned):
    got = _gen().build_rejections(lgc)
    assert got == pinned["rejections"]
    msgs = {m for _, m in got.values()}
    assert any("unknown cross-validation rule" in m for m in msgs) and any("LGC_SELECT_REVEAL_CURVE (4)" in m for m in msgs)
