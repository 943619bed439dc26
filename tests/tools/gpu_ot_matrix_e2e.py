"""Phase 1 end to end in OT mode, --use_ot against --use_ot --ot_matrix: bin/secure_multiplication on sockets, no rings, every
party on this machine and one GPU, alternating the two modes --reps times each on one generated input (the input writer and the
runner are tests/tools/gpu_ti_matrix_e2e.py's).  Prints one JSON line per run (mode, realtime and bytes_sent per party) and a
summary line with the medians and the bytes the formulas of include/linreg_gc_ot_matrix.h give for the provider pair:
   python tests/tools/gpu_ot_matrix_e2e.py --n 10000 --d 100 [--reps 2] [--width 64 --precision 56] [--dir DIR]
Two providers with d / 2 columns each (the second holds y).  "realtime" is what the binary reports: from its start barrier to the
end of its phase 1, parsing of the input and the base OTs included."""
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


def batch_rows(n, r, s, w):
    per = max(min((1 << 24) // (r * w), (256 << 20) // (r * w * s * (w // 8))), 1)
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
        res = {"use_ot": [], "ot_matrix": []}
        sent = {}
        for _ in range(o.reps):
            for mode, extra in (("use_ot", []), ("ot_matrix", ["--ot_matrix"])):
                real, sent[mode] = run(path, 2, ["--width_phase1=%d" % w, "--use_ot"] + extra, o.precision, o.timeout)
                res[mode].append(max(real))
                print(json.dumps({"mode": mode, "n": n, "d": d, "width": w, "realtime": real, "bytes_sent": sent[mode]}), flush=True)
    # providers are parties 3 and 4 (indices 2 and 3); party 4, which holds y, sends (host/phase1_ot.c's rule), party 3 receives
    r, s = d // 2, d - d // 2 + 1
    per = max(min((1 << 24) // (n * w), r * s), 1)
    pair_batches = [min(per, r * s - q) for q in range(0, r * s, per)]
    payload = {"use_ot": {"receiver_to_sender": sum(8 + u_bytes(b * n * w) for b in pair_batches), "sender_to_receiver": sum(8 + b * n * w * 8 for b in pair_batches)},
               "ot_matrix": {"receiver_to_sender": 8 + sum(8 + u_bytes(b * r * w) for b in batch_rows(n, r, s, w)),
                             "sender_to_receiver": 8 + sum(8 + b * r * w * s * w // 8 for b in batch_rows(n, r, s, w))}}
    measured = {m: {"receiver_to_sender": sent[m][2][3], "sender_to_receiver": sent[m][3][2]} for m in sent}
    rest = {m: {k: measured[m][k] - payload[m][k] for k in payload[m]} for m in sent}          # base OTs and mesh: the same in both modes
    med = {k: statistics.median(v) for k, v in res.items()}
    spread = {k: (max(v) - min(v)) / min(v) for k, v in res.items()}
    print(json.dumps({"summary": True, "n": n, "d": d, "width": w, "slowest_party_realtime_s": res, "median_s": med, "run_to_run_spread": spread,
                      "time_ratio": med["ot_matrix"] / med["use_ot"], "bytes_measured": measured, "bytes_by_formula": payload,
                      "bytes_beyond_formula": rest, "formulas_hold": rest["use_ot"] == rest["ot_matrix"]}), flush=True)


if __name__ == "__main__":
    main()
