"""The programs of include/linreg_gc_scan.h, pinned byte for byte (tests/golden/program_digests_scan.json, written by
tests/golden/gen_program_digests_scan.py): both widths, both input paths, with and without LGC_SCAN_SE, c = 1, 2, 5 covariates
and M = 1, 3, 40 candidates.  tests/test_program_digests.py and its siblings, unchanged, are the proof that no older program
moved.  No GPU needed."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_program_digests_scan", os.path.join(GOLDEN, "gen_program_digests_scan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLDEN, "program_digests_scan.json")) as f:
        return json.load(f)


def test_lowered_programs_are_pinned(lgc, pinned):
    got = _gen().build_digests(lgc)
    assert sorted(got) == sorted(pinned["programs"]) and len(got) == 2 * 2 * 3 * 3 * 2
    bad = [(name, part) for name in sorted(got) for part in ("records", "launches", "info") if got[name][part] != pinned["programs"][name][part]]
    assert not bad, bad
    assert len({v["records"] for v in got.values()}) == len(got)           # every variant is a program of its own
