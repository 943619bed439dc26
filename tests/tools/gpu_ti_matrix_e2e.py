"""Phase 1 end to end under the trusted initializer, default mode against --ti_matrix: bin/secure_multiplication on sockets, no
rings, every party on this machine and one GPU, alternating the two modes --reps times each on one generated input.  Prints one
JSON line per run (mode, realtime and bytes_sent per party) and a summary line with the medians:
   python tests/tools/gpu_ti_matrix_e2e.py --n 10000 --d 100 --providers 2 [--reps 2] [--width 64 --precision 56] [--dir DIR]
"realtime" is what the binary reports: from its start barrier to the end of its phase 1, parsing of the input included."""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EXE = os.path.join(ROOT, "linreg-mpc_amd", "host", "bin", "secure_multiplication")


def free_ports(k):
    socks = [socket.socket() for _ in range(k)]
    for s in socks:
        s.bind(("127.0.0.1", 0))
    ports = [s.getsockname()[1] for s in socks]
    for s in socks:
        s.close()
    return ports


def write_input(path, n, d, P):
    rng = np.random.default_rng(n + d)
    ports = free_ports(P + 2)
    with open(path, "w") as f:
        f.write("%d %d %d\n" % (n, d, P))
        f.write("127.0.0.1:%d\n127.0.0.1:%d\n" % (ports[0], ports[1]))
        for k in range(P):
            f.write("127.0.0.1:%d %d\n" % (ports[2 + k], k * d // P))
        f.write("%d %d\n" % (n, d))
        for r0 in range(0, n, 1000):
            np.savetxt(f, rng.uniform(-1, 1, size=(min(1000, n - r0), d)), fmt="%.6f")
        f.write("%d\n" % n)
        f.write(" ".join("%.6f" % v for v in rng.uniform(-1, 1, size=n)) + "\n")


def run(path, P, args, precision, timeout):
    procs = [subprocess.Popen([EXE, path, str(precision), str(k)] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE) for k in range(1, P + 3)]
    outs = [q.communicate(timeout=timeout) for q in procs]
    if any(q.returncode for q in procs):
        raise SystemExit("a party failed: %r" % [e.decode()[-300:] for _, e in outs])
    real, sent = [], []
    for o, _ in outs:
        for line in o.decode().splitlines():
            if line.startswith("{") and "realtime" in line:
                real.append(float(json.loads(line)["realtime"]))
            if line.startswith("{") and "bytes_sent" in line:
                sent.append(json.loads(line)["bytes_sent"])
    return real, sent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--d", type=int, default=100)
    ap.add_argument("--providers", type=int, default=2)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--precision", type=int, default=56)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--dir", default=None)
    o = ap.parse_args()
    subprocess.check_call(["make", "-C", os.path.dirname(os.path.dirname(EXE))], stdout=subprocess.DEVNULL)
    with tempfile.TemporaryDirectory(dir=o.dir) as tmp:
        path = os.path.join(tmp, "phase1.in")
        write_input(path, o.n, o.d, o.providers)
        res = {"default": [], "ti_matrix": []}
        for _ in range(o.reps):
            for mode, extra in (("default", []), ("ti_matrix", ["--ti_matrix"])):
                real, sent = run(path, o.providers, ["--width_phase1=%d" % o.width] + extra, o.precision, o.timeout)
                res[mode].append(max(real))
                print(json.dumps({"mode": mode, "n": o.n, "d": o.d, "providers": o.providers, "width": o.width, "realtime": real, "bytes_sent": sent}), flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    spread = {k: (max(v) - min(v)) / min(v) for k, v in res.items()}
    print(json.dumps({"summary": True, "n": o.n, "d": o.d, "providers": o.providers, "slowest_party_realtime_s": res, "median_s": med,
                      "run_to_run_spread": spread, "time_ratio": med["ti_matrix"] / med["default"]}), flush=True)


if __name__ == "__main__":
    main()
