"""The programs of include/linreg_gc_inference.h, pinned byte for byte (tests/golden/program_digests_inference.json, written by
tests/golden/gen_program_digests_inference.py): both widths, both input paths, the three reveal subsets, d = 1, 5, 65 and 184
(184 reaches the Karatsuba products of the factorisation at width 64).  tests/test_program_digests.py,
tests/test_program_digests_se.py and tests/test_program_digests_ridge_cv.py, unchanged, are the proof that no older program
moved.  No GPU needed."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_program_digests_inference", os.path.join(GOLDEN, "gen_program_digests_inference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLDEN, "program_digests_inference.json")) as f:
        return json.load(f)


def test_lowered_programs_are_pinned(lgc, pinned):
    got = _gen().build_digests(lgc)
    assert sorted(got) == sorted(pinned["programs"]) and len(got) == 2 * 2 * 4 * 3
    bad = [(name, part) for name in sorted(got) for part in ("records", "launches", "info") if got[name][part] != pinned["programs"][name][part]]
    assert not bad, bad
    assert len({v["records"] for v in got.values()}) == len(got)           # every variant is a program of its own
