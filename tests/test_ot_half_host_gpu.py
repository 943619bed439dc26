"""bin/linreg and bin/secure_multiplication with --use_ot --ot_matrix --ot_half on the MI355X, five processes per run, one run
after another: the printed results are those of --use_ot --ot_matrix (the shares' sums are the same words), the bytes between
two providers follow the formulas of include/linreg_gc_ot_half.h exactly, and a provider whose peer runs another mode fails at
once with a message."""
import os
import subprocess

import pytest

import ot_half_model as hm
import ot_matrix_model as om
from test_ot_matrix_host_gpu import U_BYTES, _pairs
from test_ti_matrix_host_gpu import HOST, OWNED, _bytes, _printed, _readme, _run, _uneven

pytestmark = pytest.mark.gpu

MATRIX = ["--use_ot", "--ot_matrix"]


def _same_with_and_without(path, args, precision=56):
    full, half = _run("linreg", path, args + MATRIX, precision=precision), _run("linreg", path, args + MATRIX + ["--ot_half"], precision=precision)
    assert sum(l.startswith("Result:") for l in full[1].splitlines()) >= 1
    for k in range(5):
        assert _printed(full[k]) == _printed(half[k]), k + 1
    return full[1]


@pytest.mark.parametrize("w", [64, 32])
def test_readme_example(tmp_path, golden_dir, w):
    """the README's line: cgd 10 0.001 --use_ot --ot_matrix prints the same Result with --ot_half, at phase-1 widths 64 and 32"""
    path, P_ = _readme(tmp_path, golden_dir)
    assert P_ == 3
    args = ["cgd", "10", "0.001"] + ([] if w == 64 else ["--width_phase1=32", "--width_phase2=32"])
    ev = _same_with_and_without(path, args, precision={64: 56, 32: 24}[w])
    assert len([l for l in ev.splitlines() if l.startswith("Result:")]) == 1


def test_uneven_columns_lasso_folds(tmp_path):
    """--folds=2: the protocol once per row fold (base OTs, magic and batches each time), on blocks of 1 x 4, 3 x 1 and 4 x 3 words"""
    ev = _same_with_and_without(_uneven(tmp_path, 40, "uneven.in"), ["lasso", "40", "0.001", "--l1_ratios=1,0.5,0.1", "--folds=2", "--reveal_index"])
    assert "Folds: 2" in ev and "Selected index:" in ev


@pytest.mark.parametrize("w", [64, 32])
def test_traffic_follows_the_formulas(tmp_path, w):
    """n = 40 on uneven columns.  The per-pair mode's bytes between two providers are one blob of u and one of y for all r s pairs
    (8-byte length each) on top of the base OTs and the mesh; the half mode's are, over the batches of its batch rule,
    8 + lgc_ot_u_bytes(M) one way and 8 + lgc_ot_gilboa_half_y_bytes the other, the 8-byte magic each way, and the same base-OT and
    mesh bytes.  Against the matrix mode only y differs: rows r (W / 2 + 1) s W / 8 bytes for rows r W s W / 8."""
    n = 40
    assert OWNED == [0, 1, 5]
    args = ["--width_phase1=%d" % w, "--use_ot"]
    prec = {64: 56, 32: 24}[w]
    path = _uneven(tmp_path, n, "u.in")
    plain = _bytes(_run("secure_multiplication", path, args, precision=prec))
    matrix = _bytes(_run("secure_multiplication", path, args + ["--ot_matrix"], precision=prec))
    half = _bytes(_run("secure_multiplication", path, args + ["--ot_matrix", "--ot_half"], precision=prec))
    for snd, rcv, s, r in _pairs():
        m = r * s * n * w                                         # per-pair mode: one batch of r s pairs (2^24 OTs are far away)
        base_r, base_s = plain[rcv][snd] - (8 + U_BYTES(m)), plain[snd][rcv] - (8 + m * 8)
        assert base_r > 0 and base_s > 0
        batches = hm.batch_rows(n, r, s, w)
        assert sum(batches) == n
        exp_r = base_r + 8 + sum(8 + U_BYTES(b * r * w) for b in batches)
        exp_s = base_s + 8 + sum(8 + hm.y_bytes(b, r, s, w) for b in batches)
        assert half[rcv][snd] == exp_r, (snd, rcv)
        assert half[snd][rcv] == exp_s, (snd, rcv)
        assert batches == om.batch_rows(n, r, s, w)               # here the same single batch, so the two modes differ in y alone
        assert half[rcv][snd] == matrix[rcv][snd]
        assert matrix[snd][rcv] - half[snd][rcv] == n * r * s * (w // 8) * (w - (w // 2 + 1))
    for k in (2, 3, 4):
        assert half[k][:2] == plain[k][:2]


@pytest.mark.parametrize("flagged", [3, 4])
@pytest.mark.parametrize("others", ["matrix", "pair"])
def test_mode_mismatch_fails_at_once(tmp_path, flagged, others):
    """only one provider has --ot_half; the others run plain --ot_matrix or the per-pair mode.  It and its peer in the pair of
    parties 3 and 4 (the first pair either of them meets) exit non-zero, each with a mode-mismatch message and the hint.  Party 3
    is that pair's receiver."""
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    path = _uneven(tmp_path, 40, "u.in")
    other = 7 - flagged
    procs = []
    for k in range(1, 6):
        args = ["--use_ot"] + (["--ot_matrix", "--ot_half"] if k == flagged else (["--ot_matrix"] if others == "matrix" else []))
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
    assert b"does not speak --ot_half" in outs[flagged][1] and b"same mode" in outs[flagged][1], outs[flagged][1][-400:]
    if others == "matrix":
        assert b"the peer runs --ot_matrix without --ot_half" in outs[flagged][1], outs[flagged][1][-400:]
        assert b"the peer runs --ot_matrix with --ot_half" in outs[other][1] and b"same mode" in outs[other][1], outs[other][1][-400:]
    else:
        assert b"the peer runs --ot_matrix --ot_half" in outs[other][1] and b"same mode" in outs[other][1], outs[other][1][-400:]
    assert b"bytes_sent" not in outs[3][0] and b"bytes_sent" not in outs[4][0]
