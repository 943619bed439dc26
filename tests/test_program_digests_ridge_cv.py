"""The programs of include/linreg_gc_ridge_cv.h, pinned byte for byte (tests/golden/program_digests_ridge_cv.json, written by
tests/golden/gen_program_digests_ridge_cv.py): both widths, both input paths, K = 2 and 3, cgd and cholesky, the reveal flags
on / off, and one value.  tests/test_program_digests.py and tests/test_program_digests_se.py, unchanged, are the proof that
no older program moved.  No GPU needed."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_program_digests_ridge_cv", os.path.join(GOLDEN, "gen_program_digests_ridge_cv.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLDEN, "program_digests_ridge_cv.json")) as f:
        return json.load(f)


def test_lowered_programs_are_pinned(lgc, pinned):
    got = _gen().build_digests(lgc)
    assert sorted(got) == sorted(pinned["programs"]) and len(got) == 4 * (2 * 2 * 2 + 1)
    bad = [(name, part) for name in sorted(got) for part in ("records", "launches", "info") if got[name][part] != pinned["programs"][name][part]]
    assert not bad, bad
    assert len({v["records"] for v in got.values()}) == len(got)           # every variant is a program of its own
