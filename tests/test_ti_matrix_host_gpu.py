"""bin/linreg --ti_matrix and bin/secure_multiplication --ti_matrix on the MI355X, five processes per run, one run after
another: the printed results are those of the default trusted-initializer mode (both phases at one width: the shares' sums
are the same words), and the bytes on the sockets follow the formulas of include/linreg_gc_p1_matrix.h exactly."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import free_ports

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "linreg-mpc_amd", "host")
OWNED = [0, 1, 5]                 # three providers hold 1, 4 and 2 of the 7 columns; the last one holds y as well
D = 7


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


def _uneven(tmp_path, n, name):
    """a seeded n x 7 input; the first 40 rows of the n = 400 file are the n = 40 file's"""
    rng = np.random.default_rng(20240)
    X = rng.uniform(-1, 1, size=(400, D))
    y = X @ rng.uniform(-1, 1, size=D) + 0.1 * rng.standard_normal(400)
    ports = free_ports(5)
    head = ["%d %d 3" % (n, D), "127.0.0.1:%d" % ports[0], "127.0.0.1:%d" % ports[1]] + ["127.0.0.1:%d %d" % (ports[2 + k], OWNED[k]) for k in range(3)]
    rows = [" ".join("%.12g" % v for v in X[k]) for k in range(n)]
    path = str(tmp_path / name)
    open(path, "w").write("\n".join(head + ["%d %d" % (n, D)] + rows + ["%d" % n, " ".join("%.12g" % v for v in y[:n]), ""]))
    return path


def _run(exe, path, args, nparties=5, timeout=240, precision=56):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    procs = [subprocess.Popen([os.path.join(HOST, "bin", exe), path, str(precision), str(k)] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
             for k in range(1, nparties + 1)]
    outs = [q.communicate(timeout=timeout) for q in procs]
    assert all(q.returncode == 0 for q in procs), [e.decode()[-400:] for _, e in outs]
    return [o.decode() for o, _ in outs]


def _printed(out):
    """a party's output without the lines that carry a time"""
    return [l for l in out.splitlines() if not re.search("[Tt]ime", l)]


def _same_with_and_without(path, args):
    plain, matrix = _run("linreg", path, args), _run("linreg", path, args + ["--ti_matrix"])
    assert sum(l.startswith("Result:") for l in plain[1].splitlines()) >= 1
    for k in range(5):
        assert _printed(plain[k]) == _printed(matrix[k]), k + 1
    return plain[1]


def test_readme_example(tmp_path, golden_dir):
    """the README's line: cgd 10 0.001 prints the same Result with --ti_matrix"""
    path, P_ = _readme(tmp_path, golden_dir)
    assert P_ == 3
    ev = _same_with_and_without(path, ["cgd", "10", "0.001"])
    assert len(set(re.findall("-?[0-9]+\\.[0-9]+", [l for l in ev.splitlines() if l.startswith("Result:")][0]))) == 5


def test_uneven_columns_cholesky(tmp_path):
    _same_with_and_without(_uneven(tmp_path, 40, "uneven.in"), ["cholesky", "0", "0.001"])


def test_uneven_columns_lasso_folds(tmp_path):
    """--folds=3: the protocol once per row fold, a fresh master seed each"""
    ev = _same_with_and_without(_uneven(tmp_path, 40, "uneven.in"), ["lasso", "40", "0.001", "--l1_ratios=1,0.5,0.1", "--folds=3", "--reveal_index"])
    assert "Folds: 3" in ev and "Selected index:" in ev


def _bytes(outs):
    """bytes_sent[party k - 1][to party q - 1] from the JSON lines of bin/secure_multiplication"""
    sent = []
    for o in outs:
        line = [l for l in o.splitlines() if "bytes_sent" in l]
        assert len(line) == 1
        sent.append(json.loads(line[0])["bytes_sent"])
    return sent


@pytest.mark.parametrize("w", [64, 32])
def test_traffic_follows_the_formulas(tmp_path, w):
    """n = 40 against n = 400 on the same columns.  The initializer's bytes to every provider do not depend on n (seeds and a b
    words); a provider's bytes to a peer grow by exactly 360 (its columns facing that peer) W / 8 -- the framing cancels -- and
    are one blob of 8 + n cols W / 8 bytes beside the mesh's own 4-byte hello and barrier words.  In the default mode the
    initializer's bytes grow with n"""
    args = ["--width_phase1=%d" % w]
    prec = {64: 56, 32: 24}[w]
    small = _bytes(_run("secure_multiplication", _uneven(tmp_path, 40, "s.in"), args + ["--ti_matrix"], precision=prec))
    large = _bytes(_run("secure_multiplication", _uneven(tmp_path, 400, "l.in"), args + ["--ti_matrix"], precision=prec))
    ncols = {2: 1, 3: 4, 4: 3}                       # party index -> the columns it masks towards any peer (the last one: 2 and y)
    wb = w // 8
    assert small[0] == large[0] and all(v > 0 for v in small[0][2:])
    # the initializer: the magic, then per instance (seed_a, seed_s) to A and seed_b and T to B, each a blob with an 8-byte length
    exp = {k: 8 for k in ncols}
    for lo in ncols:
        for hi in ncols:
            if lo < hi:
                exp[hi] += 8 + 32
                exp[lo] += 8 + 16 + ncols[hi] * ncols[lo] * wb
    assert small[0][2:] == [exp[2], exp[3], exp[4]]
    for k in ncols:
        for q in ncols:
            if q == k:
                continue
            assert large[k][q] - small[k][q] == 360 * ncols[k] * wb, (k, q)
            assert 0 <= small[k][q] - (8 + 40 * ncols[k] * wb) <= 8, (k, q)      # one blob; the mesh's hello and the barrier: 4 bytes each
        assert small[k][:2] == large[k][:2]
    if w == 64:
        plain_s = _bytes(_run("secure_multiplication", _uneven(tmp_path, 40, "ps.in"), args, precision=prec))
        plain_l = _bytes(_run("secure_multiplication", _uneven(tmp_path, 400, "pl.in"), args, precision=prec))
        assert all(plain_l[0][q] > plain_s[0][q] > small[0][q] for q in (2, 3, 4))
