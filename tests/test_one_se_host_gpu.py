"""bin/linreg --folds=K --one_se --reveal_index --reveal_curve on the MI355X: five processes cross-validate a lasso path end to
end and reveal the one-standard-error model, both indices and the curve: in TI mode over the device-resident table ring,
and once with --use_ot.  The provider that holds y appends the folds' y^T y
(include/linreg_gc_folds_yy.h) to its share.  The expected words come from the oracle's phase 1 on files that hold one fold's
rows each, fed to tests/lasso_cv_se_model.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import lasso_cv_se_model as sem
import test_folds_host_gpu as fh

pytestmark = pytest.mark.gpu

W, P, N, LAM2, K, RATIOS = fh.W, fh.P, fh.N, fh.LAM2, 3, [0.1, 1.0, 0.5]
ARGS = ["lasso", str(N), str(LAM2), "--l1_ratios=0.1,1,0.5", "--folds=%d" % K, "--one_se", "--reveal_index", "--reveal_curve"]
CHILD_TIMEOUT = 180


@pytest.fixture(scope="module")
def expected(lgc, oracle, golden_dir, tmp_path_factory):
    """the model on shares rebuilt from the README input: fold k's rows in a file of their own, quantised with that file's
    row count; yy_k = sum of the squared quantised y of the fold, mod 2^64"""
    tok = open(os.path.join(golden_dir, "readme_example.in")).read().split("\n")
    n, d, P_ = map(int, tok[0].split())
    rows, ys = tok[2 + P_ + 2:2 + P_ + 2 + n], tok[2 + P_ + 2 + n + 1].split()
    tmp = tmp_path_factory.mktemp("folds_se")
    per, yy = [], []
    for k in range(K):
        r0, r1 = lgc.fold_rows(n, K, k)
        path = str(tmp / ("fold%d.in" % k))
        head = ["%d %d %d" % (r1 - r0, d, P_)] + tok[1:1 + P_ + 2]
        open(path, "w").write("\n".join(head + ["%d %d" % (r1 - r0, d)] + rows[r0:r1] + ["%d" % (r1 - r0), " ".join(ys[r0:r1]), ""]))
        inp = oracle.read_input(path)
        Xq, yq = oracle.quantize(inp["X"], P, inp["n"], W), oracle.quantize(inp["y"], P, inp["n"], W)
        A, b = oracle.aggregate(Xq, yq, inp["n"], d, P, W)
        per.append(np.concatenate([A, b]).astype(np.uint64)[None, :])
        yy.append(sum(int(v) * int(v) for v in np.asarray(yq).astype(np.int64).ravel()) & ((1 << W) - 1))
    m = sem.lasso_cv_se(per, [yy], d, W, P, N, RATIOS, sem.RATIO, 1, LAM2)
    return m, d, P_


def _run(path, P_, extra):
    """the P_ + 2 processes; each is waited for under its own time limit, and the first non-zero exit ends the test"""
    subprocess.check_call(["make", "-C", fh.HOST], stdout=subprocess.DEVNULL)
    exe = os.path.join(fh.HOST, "bin", "linreg")
    procs = [subprocess.Popen([exe, path, str(P), str(k)] + ARGS + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE) for k in range(1, P_ + 3)]
    outs = []
    try:
        for k, q in enumerate(procs):
            outs.append(q.communicate(timeout=CHILD_TIMEOUT))
            assert q.returncode == 0, (k + 1, q.returncode, outs[-1][1].decode()[-600:])
    finally:
        for q in procs:
            if q.poll() is None:
                q.kill()
                q.communicate()
    return outs


def _check_output(ev, m, d):
    lines = ev.strip().splitlines()
    num = "-?[0-9]+\\.[0-9]+"
    assert lines[-1].startswith("Result:") and sum(l.startswith("Result:") for l in lines) == 1
    assert re.findall(num, lines[-1]) == ["%.15f" % (v / 2.0 ** P) for v in m["beta"]]
    assert [l for l in lines if l.startswith("Selected index:")] == ["Selected index: %d (L1 ratio: %.17g)" % (m["index"], RATIOS[m["index"]])]
    assert [l for l in lines if l.startswith("Minimum index:")] == ["Minimum index: %d (L1 ratio: %.17g)" % (m["min"], RATIOS[m["min"]])]
    curve = [l for l in lines if l.startswith("CV curve")]
    assert curve == ["CV curve %d (L1 ratio: %.17g): mean %.15f se %.15f" % (l, RATIOS[l], m["mean"][l] / 2.0 ** P, m["se"][l] / 2.0 ** P)
                     for l in range(len(RATIOS))]
    assert "Folds: %d" % K in lines and "A = " not in ev


def test_readme_run_over_the_table_ring(lgc, tmp_path, golden_dir, expected):
    """TI mode, the roles apart (lgc_party_create_lasso_cv_se in parties 1 and 2) with the garbled tables of the new program
    in the device-resident table ring (--table_ring); every revealed word -- beta+, l+, l*, mean, se -- against the model"""
    m, d, P_ = expected
    print("model: l+ = %d, l* = %d, mean %s, se %s" % (m["index"], m["min"], m["mean"], m["se"]))
    assert len(set(m["beta"])) > 1 and min(m["se"]) > 0
    path, _ = fh._readme(tmp_path, golden_dir)
    _check_output(_run(path, P_, ["--table_ring"])[1][0].decode(), m, d)


def test_readme_run_with_ot_phase1(tmp_path, golden_dir, expected):
    """--use_ot: Gilboa products per fold; the sums of shares do not depend on the masks, so the same words are expected"""
    m, d, P_ = expected
    path, _ = fh._readme(tmp_path, golden_dir)
    _check_output(_run(path, P_, ["--use_ot"])[1][0].decode(), m, d)


def test_options_belong_to_folds(golden_dir):
    """--one_se and --reveal_curve without --folds are refused before anything connects"""
    exe = os.path.join(fh.HOST, "bin", "linreg")
    for opt in ("--one_se", "--reveal_curve"):
        q = subprocess.run([exe, os.path.join(golden_dir, "readme_example.in"), str(P), "1", "lasso", "5", "0.001", "--l1_ratios=1,0.5", opt],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=30)
        assert q.returncode != 0 and ("%s belongs to --folds" % opt).encode() in q.stderr + q.stdout
