"""Records what bin/linreg of the PARENT commit says to every line of tests/linreg_cli_corpus.py, into linreg_cli_rules.json.

One-off, on a machine without a GPU; no test runs it.  It checks the given revision (default: HEAD^) out into a scratch worktree,
builds host/bin/linreg there against this tree's liblinreg_gc.so, and keeps the first line of stderr of every run: a line the
rules accept ends in "Could not read config", recorded as "accepted".  The fixture holds the distinct messages once and one index
per corpus line.

    python tests/golden/gen_linreg_cli_rules.py [revision]
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from linreg_cli_corpus import corpus  # noqa: E402

ACCEPTED = "accepted"


def first_line(exe, args):
    run = subprocess.run(["linreg"] + args, executable=exe, capture_output=True, text=True, timeout=120)
    said = run.stderr.split("\n")
    if "Could not read config" in said[:2]:                            # behind config_new's own "fopen: ..." line
        return ACCEPTED                                                # (the device warm-up thread is up by then: any exit status)
    assert run.returncode == 1, (args, run.returncode, run.stderr[-500:])
    return said[0]                                                     # (of the usage text, too, its first line)


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD^"
    tmp = tempfile.mkdtemp(prefix="linreg_parent_")
    tree = os.path.join(tmp, "tree")
    subprocess.check_call(["git", "-C", ROOT, "worktree", "add", "--detach", tree, rev], stdout=subprocess.DEVNULL)
    try:
        so = os.path.join(ROOT, "linreg-mpc_amd", "csrc", "liblinreg_gc.so")
        if os.path.exists(so):                                         # else make builds the parent's own
            shutil.copy2(so, os.path.join(tree, "linreg-mpc_amd", "csrc", "liblinreg_gc.so"))
        host = os.path.join(tree, "linreg-mpc_amd", "host")
        subprocess.check_call(["make", "-C", host, "bin/linreg"], stdout=subprocess.DEVNULL)
        exe = os.path.join(host, "bin", "linreg")
        lines = corpus()
        env_clean = {k: v for k, v in os.environ.items() if not k.startswith("LINREG_")}
        os.environ.clear()
        os.environ.update(env_clean)
        with ThreadPoolExecutor(8) as pool:
            said = list(pool.map(lambda a: first_line(exe, a), lines))
    finally:
        subprocess.call(["git", "-C", ROOT, "worktree", "remove", "--force", tree])
        shutil.rmtree(tmp, ignore_errors=True)
    messages = [ACCEPTED] + sorted(set(said) - {ACCEPTED})
    where = {m: i for i, m in enumerate(messages)}
    out = {"revision": subprocess.check_output(["git", "-C", ROOT, "rev-parse", rev], text=True).strip(),
           "lines": len(lines), "messages": messages, "index": [where[m] for m in said]}
    with open(os.path.join(HERE, "linreg_cli_rules.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("%d lines, %d distinct messages, %.1f %% accepted" % (len(lines), len(messages) - 1, 100.0 * said.count(ACCEPTED) / len(lines)))


if __name__ == "__main__":
    main()
