"""Phase 1 on row folds (include/linreg_gc_folds.h) without a GPU: the fold rule, bin/linreg's --folds / --reveal_index
rejections (every check precedes device use), the wrapper's extra output line, the documents and the header's exports."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,K", [(2, 2), (10, 2), (10, 3), (83, 5), (16, 16), (1000, 16)])
def test_folds_partition_the_rows(lgc, n, K):
    rows = [lgc.fold_rows(n, K, k) for k in range(K)]
    assert rows[0][0] == 0 and rows[-1][1] == n
    assert all(rows[k][1] == rows[k + 1][0] for k in range(K - 1))
    sizes = [r1 - r0 for r0, r1 in rows]
    assert min(sizes) >= 1 and max(sizes) - min(sizes) <= 1
    assert rows == [(k * n // K, (k + 1) * n // K) for k in range(K)]


def test_fold_rule_rejections(lgc):
    for n, K, k in ((10, 1, 0), (10, 17, 0), (3, 4, 0), (10, 2, 2), (10, 0, 0)):
        with pytest.raises(lgc.LgcError) as e:
            lgc.fold_rows(n, K, k)
        assert e.value.code == -1, (n, K, k)                                   # LGC_EINVAL
    assert lgc.fold_rows(2 ** 62, 16, 15) == (15 * 2 ** 58, 2 ** 62)           # no overflow in k n


def _linreg(*args):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "linreg-mpc_amd", "host")], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "linreg-mpc_amd", "host", "bin", "linreg")
    inp = os.path.join(ROOT, "tests", "golden", "readme_example.in")             # n = 10, d = 5
    return subprocess.run([exe, inp, "56", "3"] + list(args), capture_output=True, timeout=60)


PATH = "--l1_ratios=1,0.5,0.1"


@pytest.mark.parametrize("args,want", [
    (["cgd", "10", "0.001", "--folds=2"], b"--folds is for Algorithm lasso"),
    (["lasso", "10", "0.001", "--l1=0.02", "--folds=2"], b"--folds selects among the values of a lasso path"),
    (["lasso", "10", "0.001", PATH, "--folds=1"], b"--folds wants 2..16"),
    (["lasso", "10", "0.001", PATH, "--folds=17"], b"--folds wants 2..16"),
    (["lasso", "10", "0.001", PATH, "--folds=0"], b"--folds wants 2..16"),
    (["lasso", "10", "0.001", PATH, "--folds=x"], b"--folds wants a number"),
    (["lasso", "10", "0.001", PATH, "--folds=11"], b"--folds=11: more folds than the 10 rows"),
    (["lasso", "10", "0.001", PATH, "--reveal_index"], b"--reveal_index belongs to --folds"),
    (["lasso", "10", "0.001", PATH, "--folds=2", "--ti_ring"], b"--folds and --ti_ring"),
    (["lasso", "10", "0.001", PATH, "--folds=2", "--ot_ring"], b"--folds and --ot_ring"),
    (["lasso", "10", "0.001", PATH, "--folds=2", "--input_ring"], b"--folds and --input_ring"),
    (["lasso", "10", "0.001", PATH, "--folds=2", "--lambdas=0.1,0.2"], b"--folds and --lambdas"),
    (["lasso", "10", "0.001", PATH, "--folds=2", "--lambdas=0.1,0.2", "--table_ring", "--devices=0,0"], b"--folds and --"),
])
def test_bin_linreg_rejections(args, want):
    r = _linreg(*args)
    assert r.returncode != 0 and want in r.stdout + r.stderr, (args, r.stdout[-300:], r.stderr[-300:])
    assert b"Party 3 finished phase 1" not in r.stdout


def test_wrapper_reads_the_selected_line():
    import mpc_linear_regression as m
    out = ["Folds: 2", "Selected index: 1 (L1 ratio: 0.5)", "Result:    0.250000000000000   -1.500000000000000 "]
    assert m.parse_selected_line(out) == (1, 0.5)
    assert m.parse_selected_line(["Selected index: 3 (L1: 0.002)"]) == (3, 0.002)
    assert m.parse_selected_line(out[2:]) is None
    assert m.parse_result_line(out[-1]) == [0.25, -1.5]
    r = m.MPCLinearRegression("127.0.0.1:1", "127.0.0.1:2", mpc_args=["56", "lasso", "40", "0.001", PATH, "--folds=2", "--reveal_index"])
    assert r.mpc_args[-2:] == ["--folds=2", "--reveal_index"] and r.selected is None


def test_header_is_exported_and_documented(lgc):
    hdr = open(os.path.join(ROOT, "include", "linreg_gc_folds.h")).read()
    names = set(re.findall(r"^[a-z][^\n(]*?\b(lgc_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    assert names == {"lgc_fold_rows", "lgc_p1_set_rows", "lgc_p1_local_folds"}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for nme in names:
        assert hasattr(lgc.lib(), nme), nme
        assert nme in doc, nme
    assert "linreg_gc_folds.h" in doc and "--folds" in doc and "--reveal_index" in doc
    for opt in ("--ti_ring", "--ot_ring", "--input_ring", "--lambdas", "--devices", "--use_ot", "--table_ring"):
        assert opt in doc.split("linreg_gc_folds.h", 1)[1], opt                  # which modes come with --folds and which do not
    assert "--folds=" in readme and "p1_gram_folds_kernel" in design
