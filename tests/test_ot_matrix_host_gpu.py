"""bin/linreg --use_ot --ot_matrix and bin/secure_multiplication --use_ot --ot_matrix on the MI355X, five processes per run, one
run after another: the printed results are those of --use_ot alone (one width in both phases: the shares' sums are the same
words), the bytes between two providers follow the formulas of include/linreg_gc_ot_matrix.h exactly, and a provider whose peer
runs the other mode fails at once with a message."""
import os
import re
import subprocess

import numpy as np
import pytest

import ot_matrix_model as om
from helpers import free_ports
from test_ti_matrix_host_gpu import D, HOST, OWNED, _bytes, _printed, _readme, _run, _uneven

pytestmark = pytest.mark.gpu

OT = ["--use_ot"]
U_BYTES = lambda m: (m + 127) // 128 * 128 * 16                # lgc_ot_u_bytes


def _same_with_and_without(path, args, precision=56):
    plain, matrix = _run("linreg", path, args + OT, precision=precision), _run("linreg", path, args + OT + ["--ot_matrix"], precision=precision)
    assert sum(l.startswith("Result:") for l in plain[1].splitlines()) >= 1
    for k in range(5):
        assert _printed(plain[k]) == _printed(matrix[k]), k + 1
    return plain[1]


@pytest.mark.parametrize("w", [64, 32])
def test_readme_example(tmp_path, golden_dir, w):
    """the README's line: cgd 10 0.001 --use_ot prints the same Result with --ot_matrix, at phase-1 widths 64 and 32"""
    path, P_ = _readme(tmp_path, golden_dir)
    assert P_ == 3
    args = ["cgd", "10", "0.001"] + ([] if w == 64 else ["--width_phase1=32", "--width_phase2=32"])
    ev = _same_with_and_without(path, args, precision={64: 56, 32: 24}[w])
    assert len([l for l in ev.splitlines() if l.startswith("Result:")]) == 1


def test_uneven_columns_lasso_folds(tmp_path):
    """--folds=2: the protocol once per row fold (base OTs, magic and batches each time)"""
    ev = _same_with_and_without(_uneven(tmp_path, 40, "uneven.in"), ["lasso", "40", "0.001", "--l1_ratios=1,0.5,0.1", "--folds=2", "--reveal_index"])
    assert "Folds: 2" in ev and "Selected index:" in ev


def _pairs():
    """(sender, receiver, s, r) per provider pair, parties as 0-based indices: the sender rule of host/phase1_ot.c and the columns
    of OWNED (three providers hold 1, 4 and 2 of the 7 columns, the last one y as well)"""
    ncols = {2: 1, 3: 4, 4: 3}
    out = []
    for lo in (2, 3, 4):
        for hi in range(lo + 1, 5):
            lo_sends = ((lo % 2 == hi % 2) == (lo < hi))
            snd, rcv = (lo, hi) if lo_sends else (hi, lo)
            out.append((snd, rcv, ncols[snd], ncols[rcv]))
    return out


@pytest.mark.parametrize("w", [64, 32])
def test_traffic_follows_the_formulas(tmp_path, w):
    """n = 40 on uneven columns.  The per-pair mode's bytes between two providers are one blob of u and one of y for all r s pairs
    (8-byte length each) on top of the base OTs and the mesh; the matrix mode's are, over the batches of the shared batch rule,
    8 + lgc_ot_u_bytes(M) one way and 8 + M s W / 8 the other, the 8-byte magic each way, and the same base-OT and mesh bytes."""
    n = 40
    assert OWNED == [0, 1, 5]
    args = ["--width_phase1=%d" % w, "--use_ot"]
    prec = {64: 56, 32: 24}[w]
    path = _uneven(tmp_path, n, "u.in")
    plain = _bytes(_run("secure_multiplication", path, args, precision=prec))
    matrix = _bytes(_run("secure_multiplication", path, args + ["--ot_matrix"], precision=prec))
    for snd, rcv, s, r in _pairs():
        m = r * s * n * w                                         # per-pair mode: one batch of r s pairs (2^24 OTs are far away)
        base_r, base_s = plain[rcv][snd] - (8 + U_BYTES(m)), plain[snd][rcv] - (8 + m * 8)
        assert base_r > 0 and base_s > 0
        batches = om.batch_rows(n, r, s, w)
        assert batches == [n]
        exp_r = base_r + 8 + sum(8 + U_BYTES(b * r * w) for b in batches)
        exp_s = base_s + 8 + sum(8 + b * r * w * s * w // 8 for b in batches)
        assert matrix[rcv][snd] == exp_r, (snd, rcv)
        assert matrix[snd][rcv] == exp_s, (snd, rcv)
        assert s == 1 or matrix[rcv][snd] < plain[rcv][snd]       # u shrinks by the factor s; y only by 64 / W (and the magic is added)
    for k in (2, 3, 4):
        assert matrix[k][:2] == plain[k][:2]


def test_uneven_columns_cholesky(tmp_path):
    """the shares' sums on uneven columns (blocks of 1 x 4, 3 x 1 and 4 x 3 words, y among them).  bin/secure_multiplication prints
    no share (test_traffic_follows_the_formulas runs it to the end in both modes), so the sums are read where they show: phase 2 solves the
    system they form, and the cholesky result is the per-pair mode's digit for digit"""
    _same_with_and_without(_uneven(tmp_path, 40, "uneven.in"), ["cholesky", "0", "0.001"])


def _uneven_long(tmp_path, n, name):
    """a seeded n x 7 input on OWNED's columns, for n beyond _uneven's 400 rows"""
    rng = np.random.default_rng(20241)
    X = rng.uniform(-1, 1, size=(n, D))
    y = X @ rng.uniform(-1, 1, size=D) + 0.1 * rng.standard_normal(n)
    ports = free_ports(5)
    path = str(tmp_path / name)
    with open(path, "w") as f:
        f.write("\n".join(["%d %d 3" % (n, D), "127.0.0.1:%d" % ports[0], "127.0.0.1:%d" % ports[1]]
                          + ["127.0.0.1:%d %d" % (ports[2 + k], OWNED[k]) for k in range(3)] + ["%d %d" % (n, D)]) + "\n")
        np.savetxt(f, X, fmt="%.9g")
        f.write("%d\n" % n)
        f.write(" ".join("%.9g" % v for v in y) + "\n")
    return path


def test_three_batches_in_flight(tmp_path):
    """n = 88 000 rows: the block between parties 4 and 5 (r = 4, s = 3, W = 64) is cut by the 256 MiB bound on y into batches of
    43 690, 43 690 and 620 rows, so the helper threads, both u / y buffers, the gather at row k * per and the sum of the share
    blocks over the batches all run past k = 0 and k = 1; the block of parties 3 and 5 (r = 3, s = 1) is cut by the 2^24-OT bound
    into 87 381 and 619 rows, that of parties 3 and 4 is one batch.  The cholesky Result is that of
    --use_ot alone, and the providers' bytes in bin/secure_multiplication are the formulas' sums over those batches (the base-OT
    and mesh bytes do not depend on n: they are read off an n = 40 run of the per-pair mode).  The per-pair mode's bytes on the same
    input are pinned too: its batches are 2 pairs of columns each (the 2^24-OT rule at n w = 5 632 000), the last one ragged."""
    n, w = 88000, 64
    want = {(4, 3): [43690, 43690, 620], (1, 4): [n], (3, 1): [87381, 619]}
    for _, _, s, r in _pairs():
        assert om.batch_rows(n, r, s, w) == want[(r, s)]
    assert max(len(b) for b in want.values()) >= 3
    path = _uneven_long(tmp_path, n, "long.in")
    ev = _same_with_and_without(path, ["cholesky", "0", "0.001"])
    assert len(set(re.findall("-?[0-9]+\\.[0-9]+", [l for l in ev.splitlines() if l.startswith("Result:")][0]))) == D
    small = _bytes(_run("secure_multiplication", _uneven(tmp_path, 40, "s.in"), ["--use_ot"]))
    matrix = _bytes(_run("secure_multiplication", path, ["--use_ot", "--ot_matrix"]))
    for snd, rcv, s, r in _pairs():
        m = r * s * 40 * w
        base_r, base_s = small[rcv][snd] - (8 + U_BYTES(m)), small[snd][rcv] - (8 + m * 8)
        batches = om.batch_rows(n, r, s, w)
        assert matrix[rcv][snd] == base_r + 8 + sum(8 + U_BYTES(b * r * w) for b in batches), (snd, rcv)
        assert matrix[snd][rcv] == base_s + 8 + sum(8 + b * r * w * s * w // 8 for b in batches), (snd, rcv)
    # the per-pair mode over several batches: 2^24 // (n w) = 2 pairs each, so 6 batches for the 12 pairs of parties 4 and 5,
    # 2 + 2 for parties 3 and 4 and the ragged 2 + 1 for parties 3 and 5
    plain = _bytes(_run("secure_multiplication", path, ["--use_ot"]))
    per = (1 << 24) // (n * w)
    assert per == 2
    for snd, rcv, s, r in _pairs():
        m = r * s * 40 * w
        base_r, base_s = small[rcv][snd] - (8 + U_BYTES(m)), small[snd][rcv] - (8 + m * 8)
        pairs = [min(per, r * s - q) for q in range(0, r * s, per)]
        assert pairs == {12: [2] * 6, 4: [2, 2], 3: [2, 1]}[r * s]
        assert plain[rcv][snd] == base_r + sum(8 + U_BYTES(b * n * w) for b in pairs), (snd, rcv)
        assert plain[snd][rcv] == base_s + sum(8 + b * n * w * 8 for b in pairs), (snd, rcv)


@pytest.mark.parametrize("flagged", [3, 4])
def test_mode_mismatch_fails_at_once(tmp_path, flagged):
    """only one provider has the flag; it and its peer in the pair of parties 3 and 4 (the first pair either of them meets) exit
    non-zero, each with the mode-mismatch message.  Party 3 is that pair's receiver: flagged, it waits for the magic and meets the
    end of the connection while the per-pair sender meets the magic as the length of u; with party 4 flagged, the matrix-mode
    sender meets the length of u as the magic and the per-pair receiver meets the magic as the length of y."""
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    path = _uneven(tmp_path, 40, "u.in")
    other = 7 - flagged
    procs = []
    for k in range(1, 6):
        args = ["--use_ot"] + (["--ot_matrix"] if k == flagged else [])
        procs.append(subprocess.Popen([os.path.join(HOST, "bin", "secure_multiplication"), path, "56", str(k)] + args,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    try:
        outs = {k: procs[k - 1].communicate(timeout=120) for k in (3, 4)}
    finally:
        for q in procs:
            if q.poll() is None:
                q.kill()
            q.wait()
    assert procs[2].returncode != 0 and procs[3].returncode != 0
    assert b"does not speak --ot_matrix" in outs[flagged][1] and b"same mode" in outs[flagged][1], outs[flagged][1][-400:]
    assert b"the peer runs --ot_matrix" in outs[other][1] and b"same mode" in outs[other][1], outs[other][1][-400:]
    assert (b"could not receive u" if flagged == 3 else b"could not receive y") in outs[other][1], outs[other][1][-400:]
    assert b"bytes_sent" not in outs[3][0] and b"bytes_sent" not in outs[4][0]
