"""Phase 1 end to end in the matrix OT mode, --use_ot --ot_matrix against the same with --ot_half: bin/secure_multiplication on
sockets, no rings, every party on this machine and one GPU, alternating the two modes --reps times each on one generated input
(the input writer and the runner are tests/tools/gpu_ti_matrix_e2e.py's).  Prints one JSON line per run (mode, realtime and
bytes_sent per party) and a summary line with the medians, the ranges and the bytes the formulas of include/linreg_gc_ot_matrix.h
and include/linreg_gc_ot_half.h give for the provider pair:
   python tests/tools/gpu_ot_half_e2e.py --n 10000 --d 100 [--reps 2] [--width 64 --precision 56] [--dir DIR]
Two providers with d / 2 columns each (the second holds y).  "realtime" is what the binary reports: from its start barrier to the
end of its phase 1, parsing of the input and the base OTs included.  "ranges_overlap" says whether the slowest party's realtime
of the two modes overlap over the runs: only if they do not is a speed-up claimed."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_ti_matrix_e2e import EXE, run, write_input  # noqa: E402


def u_bytes(m):
    return (m + 127) // 128 * 128 * 16


def y_bytes(rows, r, s, w, half):
    return rows * r * (w // 2 + 1) * s * w // 8 if half else rows * r * w * s * w // 8


def batch_rows(n, r, s, w, half):
    per = max(min((1 << 24) // (r * w), (256 << 20) // y_bytes(1, r, s, w, half)), 1)
    return [min(per, n - k) for k in range(0, n, per)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--d", type=int, default=100)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--precision", type=int, default=56)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--dir", default=None)
    o = ap.parse_args()
    n, d, w = o.n, o.d, o.width
    subprocess.check_call(["make", "-C", os.path.dirname(os.path.dirname(EXE))], stdout=subprocess.DEVNULL)
    with tempfile.TemporaryDirectory(dir=o.dir) as tmp:
        path = os.path.join(tmp, "phase1.in")
        write_input(path, n, d, 2)
        res = {"ot_matrix": [], "ot_half": []}
        sent = {}
        for _ in range(o.reps):
            for mode, extra in (("ot_matrix", []), ("ot_half", ["--ot_half"])):
                real, sent[mode] = run(path, 2, ["--width_phase1=%d" % w, "--use_ot", "--ot_matrix"] + extra, o.precision, o.timeout)
                res[mode].append(max(real))
                print(json.dumps({"mode": mode, "n": n, "d": d, "width": w, "realtime": real, "bytes_sent": sent[mode]}), flush=True)
    # providers are parties 3 and 4 (indices 2 and 3); party 4, which holds y, sends (host/phase1_ot.c's rule), party 3 receives
    r, s = d // 2, d - d // 2 + 1
    payload, y_only = {}, {}
    for mode, half in (("ot_matrix", False), ("ot_half", True)):
        b = batch_rows(n, r, s, w, half)
        y_only[mode] = sum(y_bytes(x, r, s, w, half) for x in b)
        payload[mode] = {"receiver_to_sender": 8 + sum(8 + u_bytes(x * r * w) for x in b), "sender_to_receiver": 8 + 8 * len(b) + y_only[mode], "batches": len(b)}
    measured = {m: {"receiver_to_sender": sent[m][2][3], "sender_to_receiver": sent[m][3][2]} for m in sent}
    rest = {m: {k: measured[m][k] - payload[m][k] for k in measured[m]} for m in sent}           # base OTs and mesh: the same in both modes
    med = {k: statistics.median(v) for k, v in res.items()}
    spread = {k: (max(v) - min(v)) / min(v) for k, v in res.items()}
    overlap = not (max(res["ot_half"]) < min(res["ot_matrix"]) or max(res["ot_matrix"]) < min(res["ot_half"]))
    print(json.dumps({"summary": True, "n": n, "d": d, "width": w, "slowest_party_realtime_s": res, "median_s": med, "run_to_run_spread": spread,
                      "time_ratio": med["ot_half"] / med["ot_matrix"], "ranges_overlap": overlap, "y_bytes_by_formula": y_only, "bytes_measured": measured,
                      "bytes_by_formula": payload, "bytes_beyond_formula": rest, "formulas_hold": rest["ot_matrix"] == rest["ot_half"]}), flush=True)


if __name__ == "__main__":
    main()
