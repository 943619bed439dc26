"""host/ot_pipe.c, the two-in-flight batch pipeline of phase 1's OT modes, without a GPU and without the rest of the host: compiled
alone into tests/tools/ot_pipe_program.c, once under ThreadSanitizer and once under ASan + UBSan (with LeakSanitizer), and run.
The program's sender and receiver roles are two threads joined by a socketpair; its fake callbacks assert, as they run, that every
callback of a role runs once per batch in order, that send(k) sees the u of start(k) and finish(k) the y of send(k), that start(k)
waits for finish(k - 2), the sender's get of batch k for send(k - 2) and its put of batch k for send(k); nbatch = 1, 2, 3, 5 with a
short last batch.  Then every callback of either side fails once at k = 0, 1 and 2 of 3 batches (a failing put / get shuts the
connection, which is what makes one fail in the host programs): the failing role returns non-zero with all its threads joined
(a thread left behind is ThreadSanitizer's "thread leak"), the other role returns non-zero after the failing side's socket end is
closed -- but for a receiver failing in get(y) or finish at one of the last two batches, when the sender may already have sent its
last y and is then complete -- and nothing is leaked.  A hang ends at the program's alarm of 20 s.  Nothing is loaded into python.

A pthread_create that fails cannot be forced portably; run_role in ot_pipe.c counts the helpers it started, marks the failure, and
joins exactly those before it returns: read, not run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "linreg-mpc_amd", "host")


@pytest.mark.parametrize("name,flags", [("tsan", ["-fsanitize=thread"]),
                                        ("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_pipeline_rules_and_failures_under_sanitizers(tmp_path, name, flags):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / ("ot_pipe_" + name))
    cc = subprocess.run(["gcc", "-std=gnu11", "-O1", "-g"] + flags + ["-I", HOST, os.path.join(ROOT, "tests", "tools", "ot_pipe_program.c"),
                         os.path.join(HOST, "ot_pipe.c"), "-lpthread", "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "cannot find" in cc.stderr and "san" in cc.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert cc.returncode == 0, cc.stderr[-2000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1")
    env.pop("LINREG_TIMING", None)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("all ok"), (run.returncode, run.stdout[-500:], run.stderr[-3000:])
    assert run.stdout.split()[:2] == ["31", "cases"]                 # 4 clean runs, (5 + 4 callbacks) x 3 batches failing
    assert "Sanitizer" not in run.stderr, run.stderr[-3000:]
    # the only words on stderr are the pipeline's four messages
    assert set(run.stderr.splitlines()) <= {"OT: could not send u", "OT: could not receive u", "OT: could not send y", "OT: could not receive y"}
