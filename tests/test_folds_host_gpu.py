"""bin/linreg --folds=K on the MI355X: five processes cross-validate a lasso path end to end.  Phase 1 runs once per row fold
(include/linreg_gc_folds.h), the K share systems enter the pinned phase 2 of include/linreg_gc_lasso_cv.h.  The expected model
comes from the oracle's phase 1 on files that hold one fold's rows each, fed to tests/lasso_cv_model.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import lasso_cv_model as lcm
from helpers import free_ports

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "linreg-mpc_amd", "host")
W, P, N, LAM2, K = 64, 56, 40, 0.001, 2
RATIOS = [1.0, 0.5, 0.1]
ARGS = ["lasso", str(N), str(LAM2), "--l1_ratios=1,0.5,0.1", "--reveal_index"]


def _readme(tmp_path, golden_dir):
    tok = open(os.path.join(golden_dir, "readme_example.in")).read().split("\n")
    n, d, P_ = map(int, tok[0].split())
    ports = free_ports(P_ + 2)
    for i in range(P_ + 2):
        parts = tok[1 + i].split()
        parts[0] = "127.0.0.1:%d" % ports[i]
        tok[1 + i] = " ".join(parts)
    path = str(tmp_path / "readme.in")
    open(path, "w").write("\n".join(tok))
    return path, P_


@pytest.fixture(scope="module")
def expected(lgc, oracle, golden_dir, tmp_path_factory):
    """(fold systems as one (1, K (T + d)) share, beta*, l*) of the README input cut into K folds: each fold's rows go to a file
    of their own, the oracle quantises them with that file's row count and sums phase 1"""
    tok = open(os.path.join(golden_dir, "readme_example.in")).read().split("\n")
    n, d, P_ = map(int, tok[0].split())
    rows, ys = tok[2 + P_ + 2:2 + P_ + 2 + n], tok[2 + P_ + 2 + n + 1].split()
    tmp = tmp_path_factory.mktemp("folds")
    per = []
    for k in range(K):
        r0, r1 = lgc.fold_rows(n, K, k)
        path = str(tmp / ("fold%d.in" % k))
        head = ["%d %d %d" % (r1 - r0, d, P_)] + tok[1:1 + P_ + 2]
        open(path, "w").write("\n".join(head + ["%d %d" % (r1 - r0, d)] + rows[r0:r1] + ["%d" % (r1 - r0), " ".join(ys[r0:r1]), ""]))
        inp = oracle.read_input(path)
        assert (inp["n"], inp["d"]) == (r1 - r0, d)
        A, b = oracle.aggregate(oracle.quantize(inp["X"], P, inp["n"], W), oracle.quantize(inp["y"], P, inp["n"], W), inp["n"], d, P, W)
        per.append(np.concatenate([A, b]).astype(np.uint64)[None, :])
    beta, best, _, _ = lcm.lasso_cv(per, d, W, P, N, RATIOS, lcm.RATIO, 1, LAM2)
    return np.hstack(per), beta, best, d, P_


def _run(path, P_, extra, per_party=None, timeout=240):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = os.path.join(HOST, "bin", "linreg")
    procs = [subprocess.Popen([exe, path, str(P), str(k)] + ARGS + extra + ((per_party or {}).get(k, ["--folds=%d" % K])),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE) for k in range(1, P_ + 3)]
    outs = [q.communicate(timeout=timeout) for q in procs]
    return procs, outs


def _check_output(ev, beta, best):
    lines = ev.strip().splitlines()
    assert lines[-1].startswith("Result:") and sum(l.startswith("Result:") for l in lines) == 1
    assert re.findall("-?[0-9]+\\.[0-9]+", lines[-1]) == ["%.15f" % (v / 2.0 ** P) for v in beta]
    sel = [l for l in lines if l.startswith("Selected index:")]
    assert sel == ["Selected index: %d (L1 ratio: %.17g)" % (best, RATIOS[best])]
    assert "Folds: %d" % K in lines and "Algorithm: lasso" in ev and "A = " not in ev      # the fold systems are not revealed


def test_readme_run_over_the_table_ring(lgc, tmp_path, golden_dir, expected):
    system, beta, best, d, P_ = expected
    path, _ = _readme(tmp_path, golden_dir)
    procs, outs = _run(path, P_, ["--table_ring"])
    assert all(q.returncode == 0 for q in procs), [e.decode()[-400:] for _, e in outs]
    _check_output(outs[1][0].decode(), beta, best)
    assert len(set(beta)) > 1
    # the same fold systems through the co-located solver: the CLI's words are the pinned phase 2's
    sysm = lgc.make_system(d, W, P, "lasso", N, LAM2, 1, 1, 0, 0)
    s = lgc.Solver(sysm, seed=bytes(range(16)), l1_ratios=RATIOS, folds=K, reveal_index=True)
    s.set_shares(system)
    s.run()
    assert (s.beta().tolist(), s.selected_index()) == (beta, best)
    s.close()


def test_readme_run_with_ot_phase1(tmp_path, golden_dir, expected):
    """--use_ot: Gilboa products per fold; sums of shares do not depend on the masks, so the same model is expected"""
    _, beta, best, _, P_ = expected
    path, _ = _readme(tmp_path, golden_dir)
    procs, outs = _run(path, P_, ["--use_ot"])
    assert all(q.returncode == 0 for q in procs), [e.decode()[-400:] for _, e in outs]
    _check_output(outs[1][0].decode(), beta, best)


def test_parties_with_different_folds_refuse(tmp_path, golden_dir, expected):
    """the Evaluator alone is given another K: the program fingerprints differ, both sides say so, nobody hangs"""
    P_ = expected[4]
    path, _ = _readme(tmp_path, golden_dir)
    procs, outs = _run(path, P_, [], per_party={2: ["--folds=3"]}, timeout=120)
    assert procs[0].returncode != 0 and procs[1].returncode != 0
    assert b"built different programs" in outs[0][1] and b"built different programs" in outs[1][1]
    assert b"Result:" not in outs[1][0]
