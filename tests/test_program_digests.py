"""The lowered programs and the build-time rejections, pinned byte for byte (tests/golden/program_digests.json, written by
tests/golden/gen_program_digests.py): records, launch list and program info of a fixed matrix of programs, and the
(code, message) of every invalid create request through Program, Solver and Party.  No GPU needed: every rejection comes
before any device lookup."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_program_digests", os.path.join(GOLDEN, "gen_program_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLDEN, "program_digests.json")) as f:
        return json.load(f)


def test_lowered_programs_are_unchanged(lgc, pinned):
    got, _, _ = _gen().build_digests(lgc)
    assert sorted(got) == sorted(pinned["programs"])
    bad = [(name, part) for name in sorted(got) for part in ("records", "launches", "info")
           if got[name][part] != pinned["programs"][name][part]]
    assert not bad, bad
    # options all at their defaults are no options: the plain path's program, record for record
    gen = _gen()
    defaults = [name for name in got if name.endswith(gen.DEFAULT_OPTS)]
    assert len(defaults) == 4
    for name in defaults:
        assert got[name] == got[name[:-len(gen.DEFAULT_OPTS)] + gen.PLAIN_PATH], name


def test_rejections_are_unchanged(lgc, pinned):
    got = _gen().build_rejections(lgc)
    assert got == pinned["rejections"]
