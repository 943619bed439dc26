#!/usr/bin/env python3
"""bench.py -- headline benchmark of the garbled-circuit hot path on MI355X.

Metric (BASELINE.json): AND-gates/s, garble + evaluate, on the d=500 CGD-15
circuit (64-bit fixed point, precision 56) -- the circuit behind the
reference's published 4.63e6 gates/s (BASELINE.md 1.1,
experiments/results/phase2_64/test_LS_100000x500_0.1_0_cgd_64_20_p2.out:18).

A "step" is one complete solve: fresh input labels, garbling and evaluation of
the whole CGD-15 circuit, decode of beta.  Input shares are resident in HBM
before the timed region.  With N GPUs every rank solves its own independent
system (bootstrap-style sharding: no data-path collective), so scaling is weak.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--d D] [--iters I] [--dump-outputs DIR] [--full]

A plain run does what the headline needs and nothing more: it sets up, warms up, times the K steps, writes its outputs if
asked to and prints the result line.  --full adds everything else this script measures or checks, after the timed steps
(the HBM counter passes before them): the serialised profile pass, the roofline and AES figures, the OT accounting, the
end-to-end and two-process runs, the 64-lambda sweep and its model, the CPU baseline, the oracle's check of every result,
and the long record in bench_detail.json.  The --no-* options leave out parts of --full.

--dump-outputs DIR writes the beta of the last timed step to DIR (dump_outputs below); the input shares and the seed are
fixed, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "linreg-mpc_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
REF_RATE = 4.63e6                # reference gates/s on this circuit


def ref_equiv_gates(d, iters):
    """reference's own AND count for CGD at 64 bit (exact fit):
    per iteration 19300 d^2 + 221432 d + 206191; setup = 20-iteration total minus 20 iterations"""
    per_it = 19300 * d * d + 221432 * d + 206191
    total20 = 386233 * d * d + 4534169 * d + 4123635
    return (total20 - 20 * per_it) + iters * per_it


COMPACT_LIMIT = 4096             # the driver keeps ~8 000 characters of stdout: the LAST line must stay far below that


def _r(v, nd=6):
    """floats to `nd` significant digits (the full-precision figures are in bench_detail.json)"""
    if isinstance(v, bool) or v is None:
        return v
    if isinstance(v, float):
        return float("%.*g" % (nd, v))
    return v


def _pick(dct, keys):
    return {k: _r(dct[k]) for k in keys if dct is not None and k in dct}


def compact_line(out, limit=COMPACT_LIMIT):
    """The ONE stdout line of a bench run: the headline, its roofline / aes_roofline / cpu_baseline and one number per
    secondary measurement, at most `limit` bytes (the 30 KB line of round 4 did not survive the driver's
    8 000-character stdout tail, so the round's headline went unmeasured).  Everything else -- timelines, the sweep model,
    notes, definitions -- stays in the detail dict, which main() writes to bench_detail.json."""
    line = _pick(out, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                       "vs_baseline", "dtype", "data", "exact_vs_oracle", "barrier_backend", "rccl_ranks", "devices", "preflight",
                       "and_gates_per_solve", "ref_equiv_gates_per_s"))
    cfg = out.get("config") or {}
    line["config"] = {"workload": "d=%s CGD-%s %s-bit p=%s, two-party masked input, garbler+evaluator co-located; one system per GPU"
                                  % (cfg.get("d"), cfg.get("iterations"), cfg.get("width"), cfg.get("precision")),
                      **_pick(cfg, ("d", "iterations", "width", "precision", "sharding"))}
    rf = out.get("roofline")
    if rf:
        line["roofline"] = _pick(rf, ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_ms",
                                      "alg_bytes_per_launch", "binding"))
        fl = rf.get("flat_list_equiv")
        if fl:
            line["roofline"]["flat_list_required_over_peak"] = _r(fl.get("required_over_peak"))
    ar = out.get("aes_roofline")
    if ar:
        line["aes_roofline"] = _pick(ar, ("achieved", "achieved_eval_kernel", "peak", "unit", "frac", "frac_eval_kernel", "micro_kernel"))
    cb = out.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = _pick(cb, ("value", "unit", "cores", "kind", "model", "total_cores"))
        line["cpu_baseline"]["spread"] = _r((cb.get("repeats") or {}).get("spread"))
        line["cpu_baseline"]["sample"] = (cb.get("sample") or "")[:160]
        if cb.get("whole_solve"):
            line["cpu_baseline"]["whole_solve"] = _pick(cb["whole_solve"], ("value", "cores", "seconds", "circuit", "exact"))
        if cb.get("checker_error"):
            line["cpu_baseline"]["checker_error"] = str(cb["checker_error"])[:120]
    e2e = out.get("phase12")
    if e2e:
        p12 = {}
        for res in e2e:
            p12[res.get("config", "?")] = _r(res.get("phase12_wall_s"), 4) if "error" not in res else "error: " + str(res["error"])[-80:]
        p12["all_exact"] = all(res.get("exact_vs_oracle") is True for res in e2e)
        # a configuration that was run a second time (a party failed, or the first dispatch stalled behind the driver's memory
        # wipe) says so here, with the wall clock of the attempt that was set aside (no silent best-of-two)
        retried = {res.get("config", "?"): _r((res.get("first_attempt") or {}).get("phase12_wall_s"), 4) if res.get("first_attempt")
                   else "failed: " + str(res.get("first_error"))[-60:] for res in e2e if res.get("attempts", 1) > 1}
        if retried:
            p12["retried_first_attempt"] = retried
        line["phase12"] = p12
    ring = out.get("two_process_ring")
    if ring:
        line["two_process_ring"] = _pick(ring, ("seconds_garble_eval", "and_gates_per_s")) if "error" not in ring else {"error": str(ring["error"])[-120:]}
    sw = out.get("sweep64")
    if sw:
        c = _pick(sw, ("lambdas", "d", "iterations", "n_gpus", "seconds", "and_gates_per_s", "prefix_bytes_broadcast",
                       "create_s", "prefix_garble_s", "broadcast_s", "block_s", "gather_s", "block_lambdas",
                       "predicted_seconds", "measured_over_predicted", "predicted_from"))
        c["exact"] = sw.get("exact_vs_oracle")
        model = (sw.get("model") or {}).get("by_n_gpus")
        if model:                       # N = 1: what this GPU predicts for the sharded runs, one number each
            c["predicted_seconds_by_n_gpus"] = {k: _r(v["predicted_seconds"], 4) for k, v in model.items()}
        line["sweep64"] = c
    ot = out.get("ot")
    if ot:
        line["ot"] = _pick(ot, ("ot_per_s", "gb_per_s", "frac_hbm", "batch", "exact")) if "error" not in ot else {"error": str(ot["error"])[-120:]}
    if "detail_file" in out:                 # (--full: a plain run writes no long record)
        line["detail"] = out["detail_file"]
    txt = json.dumps(line, separators=(",", ":"))
    # belt and braces: drop the least important keys rather than ever print a line the driver cannot keep whole
    for victim in ("devices", "two_process_ring", "ot", "phase12", "sweep64", "cpu_baseline"):
        if len(txt) <= limit:
            break
        if victim == "devices":
            line["devices"] = len(line.get("devices") or [])
        else:
            line.pop(victim, None)
            line.setdefault("dropped", []).append(victim)
        txt = json.dumps(line, separators=(",", ":"))
    return txt


def ot_accounting(np, torch, lgc, npairs=64, n=10000, w=64, reps=4):
    """IKNP extension + Gilboa correlation of `npairs` inner products of length n (config 3: n = 10^4, 64-bit, 6.4e5 OTs per
    product; bin/linreg sends them in batches of 2^24 OTs): receiver start -> sender -> receiver finish, operands, u and y in
    HBM (lgc_ot_*_set_device_io), HIP-synchronised wall clock of the three calls, best of `reps`.  Bytes: SURVEY.md 8(d)'s
    48 B per extended OT on EACH side (16 B of PRG column material + 16 B transposed row + 8 B payload + the hash), both
    sides on this GPU."""
    import time
    rng = np.random.default_rng(11)
    seeds0 = rng.integers(0, 256, size=(128, 16), dtype=np.uint8); seeds1 = rng.integers(0, 256, size=(128, 16), dtype=np.uint8)
    delta = rng.integers(0, 256, size=16, dtype=np.uint8)
    dbits = np.unpackbits(delta, bitorder="little")
    m = npairs * n * w
    a = rng.integers(0, 2 ** 63, size=(npairs, n), dtype=np.uint64); b = rng.integers(0, 2 ** 63, size=(npairs, n), dtype=np.uint64)
    S = lgc.OtSender(delta.tobytes(), np.where(dbits[:, None] == 1, seeds1, seeds0)); R = lgc.OtReceiver(seeds0, seeds1)
    try:
        S.set_device_io(True); R.set_device_io(True)
        ub = lgc.lib().lgc_ot_u_bytes(m)
        da = torch.from_numpy(a.view(np.int64)).cuda(); db = torch.from_numpy(b.view(np.int64)).cuda()
        du = torch.empty(ub, dtype=torch.uint8, device="cuda"); dy = torch.empty(m, dtype=torch.int64, device="cuda")
        dss = torch.zeros(npairs, dtype=torch.int64, device="cuda"); dsr = torch.zeros(npairs, dtype=torch.int64, device="cuda")
        best = None
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            R.gilboa_start_ptr(da.data_ptr(), npairs, n, w, du.data_ptr())
            S.gilboa_ptr(db.data_ptr(), npairs, n, w, du.data_ptr(), dy.data_ptr(), dss.data_ptr())
            R.gilboa_finish_ptr(dy.data_ptr(), dsr.data_ptr())
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best
        ss, sr = dss.cpu().numpy().view(np.uint64), dsr.cpu().numpy().view(np.uint64)
        M = (1 << 64) - 1
        exact = all(((int(ss[q]) + int(sr[q])) & M) == (sum(int(x) * int(y) for x, y in zip(a[q], b[q])) & M) for q in (0, npairs - 1))
    finally:
        S.close(); R.close()
    rate = m / best
    gbs = 2 * 48.0 * rate / 1e9
    return {"ot_per_s": rate, "gb_per_s": gbs, "frac_hbm": gbs / HBM_PEAK_GBS, "batch": m, "exact": bool(exact), "seconds": best,
            "shape": "%d inner products x n = %d x %d bit (config 3's Gilboa batches), device-resident I/O" % (npairs, n, w),
            "bytes_per_ot": "2 x 48 B algorithmic (SURVEY.md 8(d): both sides of the extension run on this GPU)"}


def devices_preflight(torch, world, ndev, can_access=None):
    """the device side of `--gpus N`: one distinct GPU per rank, and every pair can reach the other (xGMI peer access; RCCL
    falls back to host memory without it, so a missing path is reported, not fatal).  can_access: injectable for the CPU tests."""
    if world > ndev:
        return {"error": "%d ranks but %d visible GPU(s): an RCCL group needs one GPU per rank (LGC_BENCH_BACKEND=gloo dry-runs "
                         "N ranks on fewer GPUs)" % (world, ndev)}
    can = can_access or torch.cuda.can_device_access_peer
    missing = [(i, j) for i in range(world) for j in range(world) if i != j and not can(i, j)]
    return {"distinct_devices": True, "peer_access": not missing,
            "no_peer_path": ["%d->%d" % ij for ij in missing[:8]] or None}


def cpu_info():
    model = None
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return model, os.cpu_count()


def measure_hbm_traffic(argv_tail, kernel_substr="gc_mack_kernel<true"):
    """HBM bytes per launch of the dominant kernel from the PMC counters, measured in THIS run:
    two child processes of this same script under `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE`
    (separate passes, counters only, the program directly after `--`; MI355X_MICROARCH.md, HBM
    section), started before this process touches the GPU.  Returns (bytes_per_launch, detail)."""
    import csv, glob, shutil, subprocess, tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, {"error": "rocprofv3 not found"}
    work = tempfile.mkdtemp(prefix="lgc_pmc_")
    env = dict(os.environ, TMPDIR=work)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    vals, launches = {}, 0
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(work, counter)
            cmd = [exe, "--pmc", counter, "--output-format", "csv", "-d", out, "--", sys.executable,
                   os.path.abspath(__file__), "--child"] + argv_tail
            r = subprocess.run(cmd, cwd=work, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
            files = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not files:
                return None, {"error": "rocprofv3 --pmc %s failed (rc %d): %s" % (counter, r.returncode, r.stderr.decode()[-300:])}
            acc = []
            rows = list(csv.DictReader(open(files[0])))
            for sub in (kernel_substr, "gc_mac_kernel<true"):          # (plain-array MAC kernel: 32-bit and non-default workloads)
                acc = [float(row["Counter_Value"]) for row in rows
                       if sub in row["Kernel_Name"] and row.get("Counter_Name", counter) == counter]
                if acc:
                    break
            if not acc:
                return None, {"error": "no %s rows for %s" % (counter, kernel_substr)}
            vals[counter] = sum(acc) / len(acc)
            launches = len(acc)
    except Exception as e:                                   # a profiler problem must not cost the bench line
        return None, {"error": "%s: %s" % (type(e).__name__, e)}
    finally:
        shutil.rmtree(work, ignore_errors=True)
    # gfx950: FETCH_SIZE counts wide coalesced reads at half (guide's correction) -> x2; both are in KiB
    total = (2.0 * vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024.0
    return total, {"source": "measured in this run: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE child passes of bench.py --child",
                   "fetch_kib_per_launch": vals["FETCH_SIZE"], "write_kib_per_launch": vals["WRITE_SIZE"],
                   "launches_sampled": launches, "correction": "bytes = (2*FETCH_SIZE + WRITE_SIZE) * 1024"}


def pick_two_cores():
    """two logical CPUs of this process's affinity set that are different physical cores (and, where the topology files say
    so, share an L3: garbler and evaluator hand every record over through memory)"""
    try:
        allowed = sorted(os.sched_getaffinity(0))
        def sibs(c):
            txt = open("/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list" % c).read().strip()
            out = set()
            for part in txt.split(","):
                lo, _, hi = part.partition("-")
                out.update(range(int(lo), int(hi or lo) + 1))
            return out
        def l3(c):
            try:
                return open("/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list" % c).read().strip()
            except OSError:
                return None
        a = allowed[0]
        others = [c for c in allowed[1:] if c not in sibs(a)]
        same = [c for c in others if l3(c) is not None and l3(c) == l3(a)]
        bsel = (same or others or allowed[1:] or [a])[0]
        return (a, bsel), "two physical cores%s, threads pinned with pthread_attr_setaffinity_np" % (" sharing an L3" if same else "")
    except Exception as e:           # no topology files: leave it to the scheduler, and say so
        return (-1, -1), "unpinned (%s)" % e


def sweep_model(np, sweep, shares, lams, d, make, t_all, st_all):
    """What ONE GPU can measure about the sharded sweep, and what it predicts for N = 2, 4, 8: the
    block a rank of an N-GPU run gets (64 / N lambdas, gate ids offset as on that rank) is created, fed the prefix and run
    here, alone on the chip, exactly as that rank would; the broadcast is priced at one xGMI link.  A MODEL: no second GPU
    was involved.  What it cannot see: RCCL's own latencies, eight processes creating rings at once, clock differences."""
    import time, torch
    nl = len(lams)
    link_bytes_per_s = 153e9            # one xGMI link (MI355X_MICROARCH.md); a broadcast root pushes the same bytes to 7 peers on 7 links
    rows = {}
    for n in (2, 4, 8):
        if nl % n:
            continue
        blk = nl // n
        first = nl - blk                 # the LAST block: it imports the prefix (ranks > 0 do), gate ids offset the furthest
        stt = {}
        # untimed pass first: it parks a ring of this block's size, as the warm-up of a real N-GPU run does on every rank
        for timed in (False, True):
            seed = os.urandom(16)
            t0 = time.perf_counter()
            src = make(lams[:blk], 0, seed)          # "rank 0": garbles and exports the prefix
            src.set_shares(shares)
            nbytes = src.prefix_bytes()
            buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            tg0 = time.perf_counter()
            src.prefix_garble(); src.prefix_export(buf.data_ptr()); torch.cuda.synchronize()
            t_prefix = time.perf_counter() - tg0
            src.close()
            tc0 = time.perf_counter()
            blkS = make(lams[first:first + blk], first, seed)
            t_create = time.perf_counter() - tc0
            blkS.prefix_import(buf.data_ptr())
            tb0 = time.perf_counter()
            blkS.run(); beta = blkS.beta(); torch.cuda.synchronize()
            t_block = time.perf_counter() - tb0
            blkS.close()
            del buf
        t_bcast = nbytes / link_bytes_per_s
        t_gather = 50e-6 + nl * d * 8 / link_bytes_per_s
        t_n = t_create + t_prefix + t_bcast + t_block + t_gather
        rows[str(n)] = {"block_lambdas": blk, "create_s": t_create, "prefix_garble_export_s": t_prefix, "prefix_bytes": nbytes,
                        "broadcast_s_at_153GBps": t_bcast, "block_s": t_block, "gather_s_assumed": t_gather,
                        "predicted_seconds": t_n, "predicted_speedup": t_all / t_n, "predicted_efficiency": t_all / t_n / n}
    return {"modelled": True, "measured_on": "one GPU: the last block of an N-GPU partition, alone on the chip, prefix imported as on a rank > 0",
            "n1_seconds": t_all, "n1_create_s": st_all.get("create_s"), "n1_block_s": st_all.get("block_s"), "by_n_gpus": rows,
            "assumptions": "broadcast = prefix bytes / 153 GB/s (one xGMI link per peer, links in parallel); gather = 50 us + bytes / link; "
                           "ring of the block already parked (the warm-up of a real run does that); no allowance for RCCL call latency"}


def load_sweep_prediction(world, nl, sd, sit):
    """predicted seconds of the `nl`-lambda sweep on `world` GPUs according to an N = 1 run's model, and where it came from"""
    cands = [os.path.join(os.environ.get("LGC_BENCH_DETAIL_DIR") or os.getcwd(), "bench_detail.json"),
             os.path.join(ROOT, "bench_detail.json"), os.path.join(ROOT, "profiles", "sweep_model.json")]
    for path in cands:
        try:
            dct = json.load(open(path))
        except (OSError, ValueError):
            continue
        sw = dct.get("sweep64") or {}
        row = ((sw.get("model") or {}).get("by_n_gpus") or {}).get(str(world))
        if row and (sw.get("lambdas"), sw.get("d"), sw.get("iterations")) == (nl, sd, sit):
            return float(row["predicted_seconds"]), os.path.relpath(path, ROOT)
    return None, None


def _free_ports(k):
    """k listening ports BELOW the kernel's ephemeral range (ip_local_port_range, 32768-60999 here): a port from bind(0)
    lies inside that range, and while its party is not listening yet a peer's connect() attempt can be given the same number as
    its SOURCE port -- the attempt then connects to itself (TCP simultaneous open) or the party's bind fails, and the run hangs
    (one such hang in ~600 runs of the GPU suite)"""
    import socket, random
    lo = 12000
    try:
        hi = min(30000, int(open("/proc/sys/net/ipv4/ip_local_port_range").read().split()[0]) - 1)
    except (OSError, ValueError):
        hi = 30000
    ports, rnd = [], random.SystemRandom()
    while len(ports) < k:
        p = rnd.randrange(lo, hi)
        if p in ports:
            continue
        s_ = socket.socket()
        try:
            s_.bind(("127.0.0.1", p))
            ports.append(p)
        except OSError:
            pass
        finally:
            s_.close()
    return ports


LINREG_EXE = None      # scripts/startup_probe.py --root: the bin/linreg of another build tree


def startup_timeline(stderrs, m0):
    """the LGCT marks of every party of one bin/linreg run, in seconds since the first spawn: per party the full list of
    (seconds, mark), and `steps`: the milestones VERDICT r3 item 1 asks for, each with the party that reaches it LAST
    (the run cannot go on before that)"""
    import re
    marks = {}
    for txt in stderrs:
        for mt in re.finditer(r"^LGCT (\S+) ([0-9.]+) (.*)$", txt, re.M):
            marks.setdefault(mt.group(1), []).append([round(float(mt.group(2)) - m0, 4), mt.group(3)])
    def last(pred):
        best = None
        for tag, lst in marks.items():
            for t, what in lst:
                if pred(tag, what) and (best is None or t > best[0]):
                    best = (t, tag)
        return {"t_s": best[0], "party": best[1]} if best else None
    steps = {
        "main_entered": last(lambda g, w_: w_ == "main entered"),                       # exec + dynamic linking
        "connected": last(lambda g, w_: w_ == "connected"),                             # socket mesh
        "hip_runtime_up": last(lambda g, w_: w_.startswith("lib: hip runtime up")),
        "device_context_up": last(lambda g, w_: w_.startswith("lib: device context up")),
        "code_objects_ready": last(lambda g, w_: w_.startswith("lib: constants uploaded")),
        "program_lowered": last(lambda g, w_: w_ == "lib: program lowered"),
        "evaluator_created": last(lambda g, w_: w_ == "evaluator created"),
        "phase1_done": last(lambda g, w_: w_ == "phase 1 done"),
        "barrier": last(lambda g, w_: w_ == "barrier"),
        "garbler_created": last(lambda g, w_: w_ == "garbler created"),                 # incl. the table ring
        "base_ots_done": last(lambda g, w_: w_ == "base OTs done"),
        "input_labels_in": last(lambda g, w_: w_ == "input labels received"),
        "first_table": last(lambda g, w_: w_ == "first table garbled"),
        "tables_evaluated": last(lambda g, w_: w_ == "tables evaluated"),
        "exit": last(lambda g, w_: w_ == "exit"),
    }
    return {"clock": "CLOCK_MONOTONIC, seconds since the first spawn", "steps": {k: v for k, v in steps.items() if v},
            "marks": marks}


def phase12_wall(*a, **kw):
    """phase12_wall_once, run again ONCE if a party failed (the runs share the box with whatever else is on it; a failed
    attempt is reported, not hidden: `attempts`, `first_error`)"""
    time.sleep(1.0)          # (the previous run's device memory is being wiped by the driver: see main)
    r = phase12_wall_once(*a, **kw)
    if "error" in r and "not built" not in str(r.get("error")):
        first = r["error"]
        r = phase12_wall_once(*a, **kw)
        r["attempts"] = 2
        r["first_error"] = first
        return r
    # ... and sometimes the wipe outlasts the second above (seen once in a dozen bench runs of round 5: every party of
    # config 2 waited 2.1 s, of config 1 5.1 s, between "hip runtime up" and its first kernel dispatch -- tens of GB freed by
    # the legs before them).  That is the box, not the path: run the configuration again, once, and say so.
    stall = _first_dispatch_stall(r)
    if stall is not None and stall > 1.0:
        first_wall = r.get("phase12_wall_s")
        r = phase12_wall_once(*a, **kw)
        r["attempts"] = 2
        r["first_attempt"] = {"phase12_wall_s": first_wall, "first_dispatch_stall_s": stall,
                              "why": "every party's first kernel dispatch waited for the driver (device memory of the previous leg being wiped)"}
    return r


def _first_dispatch_stall(r):
    """seconds between the CSP's 'hip runtime up' and its first kernel dispatch (LINREG_TRACE marks), None without marks"""
    try:
        marks = r["timeline"]["marks"]["p1"]
        up = [t for t, m in marks if "hip runtime up" in m]
        fd = [t for t, m in marks if "first dispatch done" in m]
        return (fd[0] - up[0]) if up and fd else None
    except (KeyError, TypeError, IndexError):
        return None


def phase12_wall_once(np, name, n, d, starts, alg, iters, extra, device_index, prec=56, source=None, exe_name="linreg", env_extra=None,
                      prec2=None, w2=64):
    """phases 1 + 2 end to end through bin/linreg, every party its own process on this box (the second
    half of the metric string): synthetic instance of experiments/generate_tests.py:159-169 (or the input file `source`
    with fresh ports: config 1), wall-clock from the first spawn to the last exit (the Result line is compared with the
    oracle later, in the cpu_baseline leg)."""
    import re, subprocess, tempfile
    exe = LINREG_EXE or os.path.join(ROOT, "linreg-mpc_amd", "host", "bin", exe_name)
    if not os.path.exists(exe):
        return {"config": name, "error": "bin/%s not built" % exe_name}
    ports = _free_ports(len(starts) + 2)
    tmp = tempfile.mkdtemp(prefix="lgc_e2e_")
    path = os.path.join(tmp, name + ".in")
    if source is not None:
        # the reference's own example file: endpoints replaced by free local ports, everything else byte for byte
        lines = open(source).read().split("\n")
        lines[1] = "127.0.0.1:%d" % ports[0]; lines[2] = "127.0.0.1:%d" % ports[1]
        for k in range(len(starts)):
            lines[3 + k] = "127.0.0.1:%d %s" % (ports[2 + k], lines[3 + k].split()[1])
        open(path, "w").write("\n".join(lines))
    else:
        rng = np.random.default_rng(7)
        X = rng.standard_normal((n, d)); X /= np.abs(X).max(axis=0)
        y = X @ rng.random(d) + 0.1 * rng.standard_normal(n)
        with open(path, "w") as f:
            f.write("%d %d %d\n127.0.0.1:%d\n127.0.0.1:%d\n" % (n, d, len(starts), ports[0], ports[1]))
            for k, st in enumerate(starts):
                f.write("127.0.0.1:%d %d\n" % (ports[2 + k], st))
            f.write("%d %d\n" % (n, d))
            for lo in range(0, n, 2000):          # (repr round-trips a double; np.savetxt takes minutes at 50 000 x 500)
                f.write("\n".join(" ".join(map(repr, row)) for row in X[lo:lo + 2000].tolist()) + "\n")
            f.write("%d\n" % n)
            f.write(" ".join(map(repr, y.tolist())) + "\n")
    # LINREG_TRACE: every process marks its steps on CLOCK_MONOTONIC (lgc_trace_mark) -- the clock time.monotonic() reads
    env = dict(os.environ, LINREG_DEVICE=str(device_index), LINREG_TRACE="1")
    env.update(env_extra or {})
    args = [str(prec), alg, str(iters), "0.001"] + extra
    t0 = time.perf_counter()
    m0 = time.monotonic()
    # stdout / stderr go to files: with pipes read one process after the other, the Evaluator (which prints the revealed
    # inputs and every iteration: > 64 KiB at d = 100) sat blocked in write() until party 1 had exited -- 80 ms of `wall`
    logs = [(open(os.path.join(tmp, "out%d" % k), "w+b"), open(os.path.join(tmp, "err%d" % k), "w+b")) for k in range(1, len(starts) + 3)]
    procs = [subprocess.Popen([exe, path, args[0], str(k)] + args[1:], stdout=logs[k - 1][0], stderr=logs[k - 1][1], env=env)
             for k in range(1, len(starts) + 3)]
    # (a blocking wait per child from a thread: Popen.wait(timeout=...) polls with sleeps of up to 50 ms)
    import threading
    ended = [None] * len(procs)

    def _wait(k_):
        procs[k_].wait()
        ended[k_] = time.monotonic()
    waiters = [threading.Thread(target=_wait, args=(k_,), daemon=True) for k_ in range(len(procs))]
    for th in waiters:
        th.start()
    deadline = time.time() + 900
    for th in waiters:
        th.join(max(0.0, deadline - time.time()))
    wall = time.perf_counter() - t0
    if any(q.poll() is None for q in procs):
        for q in procs:
            if q.poll() is None:
                q.kill()
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)
        return {"config": name, "error": "timed out"}
    outs = []
    for fo, fe in logs:
        fo.seek(0); fe.seek(0)
        outs.append((fo.read(), fe.read()))
        fo.close(); fe.close()
    res = {"config": name, "n": n, "d": d, "providers": len(starts), "algorithm": alg, "iterations": iters, "options": extra,
           "phase12_wall_s": wall, "processes": len(procs)}
    if any(q.returncode != 0 for q in procs):
        res["error"] = outs[[q.returncode != 0 for q in procs].index(True)][1].decode()[-300:]
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)
        return res
    res["timeline"] = startup_timeline([o[1].decode(errors="replace") for o in outs], m0)
    # when each process was gone (waitpid returned): the gap to its "exit" mark is the HIP runtime's and the driver's teardown
    res["timeline"]["process_end_s"] = {"p%d" % (k_ + 1): (round(ended[k_] - m0, 4) if ended[k_] else None) for k_ in range(len(procs))}
    ev = outs[1][0].decode()
    m = re.search("Time elapsed: ([0-9.]+)", ev)
    res["evaluator_time_elapsed_s"] = float(m.group(1)) if m else None
    # kept for the checker of the cpu_baseline leg (the only place of this script that touches oracle/)
    res["_check"] = {"tmp": tmp, "path": path, "alg": alg, "iters": iters, "prec": prec, "prec2": prec2, "w2": w2, "starts": starts,
                     "n": n, "d": d, "ti_seed": (env_extra or {}).get("LINREG_TI_SEED"),
                     "got": re.findall("-?[0-9]+\\.[0-9]+", ev.strip().splitlines()[-1])}
    return res


def two_process_ring(np, d, iters, p, Af, bf, gates, device_index, extra=()):
    """the deployment-shaped figure: CSP and Evaluator as two processes (bin/test_linear_system), garbled
    tables handed over through the device-resident hipIpc ring; rate = gates / (time of the last iteration)"""
    import re, subprocess, tempfile
    exe = os.path.join(ROOT, "linreg-mpc_amd", "host", "bin", "test_linear_system")
    if not os.path.exists(exe):
        return {"error": "bin/test_linear_system not built"}
    tmp = tempfile.mkdtemp(prefix="lgc_ring_")
    path = os.path.join(tmp, "ls.in")
    with open(path, "w") as f:
        f.write("%d %d\n" % (d, d))
        np.savetxt(f, Af, fmt="%.17g")
        f.write("%d\n" % d)
        np.savetxt(f, bf[None, :], fmt="%.17g")
        f.write("%d\n" % d)
        np.savetxt(f, np.zeros((1, d)), fmt="%g")
    port = _free_ports(1)[0]
    env = dict(os.environ, LINREG_DEVICE=str(device_index))
    t0 = time.perf_counter()
    procs = [subprocess.Popen([exe, str(port), str(k), path, "cgd", str(iters), str(p), "--host=127.0.0.1", "--table_ring"] + list(extra),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env) for k in (1, 2)]
    outs = [q.communicate(timeout=900) for q in procs]
    wall = time.perf_counter() - t0
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    if any(q.returncode != 0 for q in procs):
        return {"error": outs[0][1].decode()[-200:] + outs[1][1].decode()[-200:]}
    ev = outs[1][0].decode()
    its = [float(v) for v in re.findall("Iteration [0-9]+ time: ([0-9.]+)", ev)]
    g = re.search("Number of gates: ([0-9]+)", ev)
    if not its or not g:
        return {"error": "could not parse the evaluator's output"}
    return {"seconds_garble_eval": its[-1], "and_gates": int(g.group(1)), "and_gates_per_s": int(g.group(1)) / its[-1],
            "wall_all_s": wall, "note": "iteration clock of cgd.oc:190-194 on the evaluator: first table to last reveal; "
                                        "wall_all_s also holds process start, parsing of the 250 000-entry text file, base OTs and input OT"}


def dump_outputs(np, ddir, beta_fixed, p, suffix=""):
    """--dump-outputs: what a caller of the timed path receives from its last step -- beta, d words of fixed point with `p`
    fractional bits -- as float64 .npy files: beta (the values, word / 2^p) and beta_fixed_hi / beta_fixed_lo (the signed
    upper and the unsigned lower 32 bits of every word, each exact in float64), so that two builds compare bit for bit"""
    os.makedirs(ddir, exist_ok=True)
    words = np.asarray(beta_fixed, dtype=np.int64)
    arrays = {"beta": words.astype(np.float64) / float(1 << p),
              "beta_fixed_hi": (words >> 32).astype(np.float64),
              "beta_fixed_lo": (words & 0xffffffff).astype(np.float64)}
    for name, arr in arrays.items():
        np.save(os.path.join(ddir, name + suffix + ".npy"), arr)


def self_launch(n):
    """one child process per GPU; no exec, no GPU call in this (parent) process"""
    import subprocess
    port = _free_ports(1)[0]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=(subprocess.PIPE if r == 0 else subprocess.DEVNULL), stderr=None))
    # a rank that dies (out of memory, a failed check) leaves the others inside a collective until the group's timeout:
    # watch all of them, and when one exits non-zero give the rest ten seconds, then end them
    import threading, time as _t
    box = {}
    th = threading.Thread(target=lambda: box.update(out=procs[0].communicate()[0]), daemon=True)
    th.start()
    failed_at = None
    while any(q.poll() is None for q in procs):
        if failed_at is None and any(q.poll() not in (None, 0) for q in procs):
            failed_at = _t.time()
        if failed_at is not None and _t.time() - failed_at > 10.0:
            for q in procs:
                if q.poll() is None:
                    q.kill()                 # (our own children, by handle)
        _t.sleep(0.05)
    th.join()
    out0 = box.get("out") or b""
    rcs = [q.wait() for q in procs]
    sys.stdout.write(out0.decode())
    sys.stdout.flush()
    bad = [(r, rc) for r, rc in enumerate(rcs) if rc != 0]
    if bad:
        sys.stderr.write("bench.py: ranks failed (rank, exit code): %s\n" % bad)
        return 1
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--d", "--dimension", dest="d", type=int, default=500)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--precision", type=int, default=56)
    ap.add_argument("--full", action="store_true", help="besides the headline, every other measurement and check of this "
                                                            "script, and the long record in bench_detail.json (off: the headline alone)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline and the oracle's checks")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-traffic", action="store_true", help="--full: skip the two rocprofv3 --pmc child passes (roofline.traffic = null)")
    ap.add_argument("--no-e2e", action="store_true", help="--full: skip the phase-1+2 bin/linreg runs and the two-process ring run")
    ap.add_argument("--child", action="store_true", help="(internal) one bare solve, for the PMC passes")
    ap.add_argument("--no-sweep", action="store_true", help="--full: skip the 64-lambda sweep (BASELINE config 5)")
    ap.add_argument("--no-sweep-model", action="store_true", help="--full: skip the modelled 2/4/8-GPU figures of the sweep (three more block runs)")
    ap.add_argument("--no-c4", action="store_true", help="--full: skip the end-to-end run of config 4 (n = 50 000, d = 500: ~10 s to write its input, ~1 min to check it)")
    ap.add_argument("--sweep-d", type=int, default=100)
    ap.add_argument("--sweep-iters", type=int, default=15)
    ap.add_argument("--sweep-lambdas", type=int, default=64)
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last one computed (beta) as "
                                                         "DIR/<name>.npy in float64; the inputs are the same on every run")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    # `python bench.py --gpus N` without a launcher: this process becomes the launcher.  It starts one CHILD per GPU
    # (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment, as torch.distributed.run would set them) before
    # anything here touches the GPU, relays rank 0's JSON line, and exits non-zero if any rank does.
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and not args.child:
        raise SystemExit(self_launch(args.gpus))

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit("WORLD_SIZE (%d) != --gpus (%d)" % (world, args.gpus))

    # HBM counters first: the profiled children must start before this process initialises the GPU
    traffic, traffic_detail = None, {"source": "not measured (--no-traffic, N > 1, or a non-default workload)"}
    if args.full and rank == 0 and world == 1 and not args.child and not args.no_traffic:
        traffic, traffic_detail = measure_hbm_traffic(["--d", str(args.d), "--iters", str(args.iters), "--width", str(args.width),
                                                       "--precision", str(args.precision)])

    import numpy as np
    import torch                       # first: one HIP runtime per process (shared SONAME)
    import linreg_gc as lgc
    if os.environ.get("LGC_RING_SLACK_MB"):
        # run-ahead room of every co-located solver's table ring: less for ranks sharing one GPU (the 8-rank rehearsal of
        # tests/test_gpu_multirank.py), more to let a garbling MAC launch overlap the previous one's evaluation (experiments)
        lgc.set_table_ring_slack(int(os.environ["LGC_RING_SLACK_MB"]) << 20)

    if not torch.cuda.is_available() or lgc.device_count() < 1:
        raise SystemExit("bench.py needs an MI355X (no HIP device visible; there is no CPU fallback)")
    ndev = torch.cuda.device_count()
    device_index = local_rank % max(1, ndev)     # one rank per GPU; wraps only in single-GPU dry runs
    if world > ndev and os.environ.get("LGC_BENCH_BACKEND", "nccl") == "nccl":
        raise SystemExit("bench.py: %d ranks but %d visible GPU(s): an RCCL group needs one GPU per rank "
                         "(LGC_BENCH_BACKEND=gloo dry-runs N ranks on fewer GPUs)" % (world, ndev))
    # --gpus N preflight (rank 0 speaks for the node): N distinct devices exist and can reach each other -- the first run on a
    # real multi-GPU node should fail HERE, with the pair named, not inside an RCCL broadcast
    preflight = None
    if world > 1 and os.environ.get("LGC_BENCH_BACKEND", "nccl") == "nccl":
        preflight = devices_preflight(torch, world, ndev)
        if preflight.get("error"):
            raise SystemExit("bench.py --gpus %d: %s" % (world, preflight["error"]))
    torch.cuda.set_device(device_index)
    dist = None
    backend = os.environ.get("LGC_BENCH_BACKEND", "nccl")   # "gloo" only to dry-run N > 1 on one GPU
    # LGC_BENCH_FORCE_DIST=1: build the process group even for one rank, so that a one-GPU box can put every collective of
    # the N > 1 path (barrier, broadcasts, all_gather, all_reduce on device tensors) through RCCL (tests/test_gpu_multirank.py)
    if world > 1 or os.environ.get("LGC_BENCH_FORCE_DIST") == "1":
        import torch.distributed as dist
        if backend == "nccl":
            # no per-rank fallback: a rank that silently switched to gloo while the others stay in the RCCL
            # group would hang the job.  An RCCL failure ends this rank with a non-zero exit code;
            # LGC_BENCH_BACKEND=gloo is the explicit choice for dry runs (N ranks on one GPU).
            import datetime
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", device_index),
                                    timeout=datetime.timedelta(seconds=600))
            dist.barrier()                           # creates the RCCL communicator now, not inside the timed region
        else:
            import datetime
            dist.init_process_group(backend=backend, timeout=datetime.timedelta(seconds=600))

    # what the process group really is: ranks RCCL sees, and the distinct GPUs behind them
    rccl_ranks = dist.get_world_size() if (dist is not None and backend == "nccl") else None
    devices = [device_index]
    if dist is not None:
        ids = [None] * dist.get_world_size()
        dist.all_gather_object(ids, "%s/%d" % (os.uname().nodename, device_index))
        devices = sorted(set(ids))
        if backend == "nccl" and len(devices) != dist.get_world_size():
            raise SystemExit("bench.py: %d RCCL ranks on %d distinct GPU(s) (%s): one rank per GPU is required" % (dist.get_world_size(), len(devices), devices))

    d, iters, w, p = args.d, args.iters, args.width, args.precision
    T = d * (d + 1) // 2
    # synthetic two-party input (masked A, b as in test_linear_system.c:34-44): a well-conditioned
    # SPD system in fixed point, split into two additive shares; one system per rank
    rng = np.random.default_rng(1000 + rank)
    n = 4 * d
    X = rng.standard_normal((n, d)); X /= np.abs(X).max(axis=0)
    beta = rng.random(d)
    y = X @ beta + 0.1 * rng.standard_normal(n)
    Af = X.T @ X / (n * d) + np.eye(d) * 1e-3
    bf = X.T @ y / (n * d)
    scale = float(1 << p)
    tot = np.concatenate([[int(Af[i, j] * scale) for i in range(d) for j in range(i + 1)],
                          [int(v * scale) for v in bf]]).astype(np.int64).astype(np.uint64)
    mask = rng.integers(0, 2 ** 63, size=tot.size, dtype=np.uint64)
    if w == 32:
        tot &= np.uint64(0xffffffff); mask &= np.uint64(0xffffffff)
    with np.errstate(over="ignore"):
        shares = np.stack([tot - mask, mask])
    if w == 32:
        shares &= np.uint64(0xffffffff)

    sysm = lgc.make_system(d, w, p, "cgd", iters, 0.0, 2, 0, 0, 0)
    solver = lgc.Solver(sysm, seed=bytes((rank + i) & 0xff for i in range(16)), device=device_index)
    solver.set_shares(shares)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    if args.child:                     # PMC pass: one solve, nothing else
        solver.run()
        solver.close()
        return
    for _ in range(args.warmup):
        solver.run()
    barrier()
    t0 = time.perf_counter()
    mac_g = mac_e = 0.0
    mac_launches = 0
    for _ in range(args.steps):
        solver.run()
        st = solver.stats()
        mac_g += st["seconds_mac_garble"]; mac_e += st["seconds_mac_eval"]; mac_launches += st["mac_launches"]
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    st = solver.stats()
    beta_fixed = solver.beta()
    if args.dump_outputs:
        dump_outputs(np, args.dump_outputs, beta_fixed, p, "" if world == 1 else "_rank%d" % rank)
    gates = st["and_gates"]
    total_gates = gates * args.steps * world
    value = total_gates / elapsed
    refg = ref_equiv_gates(d, iters) if w == 64 else None
    # the headline record: what the timed steps measured, nothing else (--full adds its legs to it below)
    out = {
        "metric": "AND-gates/sec (garble+eval) d=500 CGD-15; phase1+2 wall-clock",
        "value": value, "unit": "AND-gates/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "barrier_backend": (backend if dist is not None else None),
        "rccl_ranks": rccl_ranks, "devices": devices, "preflight": preflight,
        # BASELINE.md's published rate (4.63e6 gates/s) counts the REFERENCE's circuit, 2.8x this build's gate count for the same
        # integers: the comparable ratio divides reference-equivalent gates by it; the own-count ratio is printed beside it
        "vs_baseline": (refg * args.steps * world / elapsed / REF_RATE) if (refg and d == 500 and iters == 15 and w == 64) else None,
        "vs_baseline_definition": "ref_equiv_gates_per_s / 4.63e6 (reference gates of this circuit per second of this build "
                                  "over the reference's published rate)",
        "vs_baseline_own_gate_count": value / REF_RATE if (d == 500 and iters == 15 and w == 64) else None,
        # the arithmetic type of the path: two's-complement fixed point of `width` bits (config.width / config.precision);
        # the garbled circuit computes it gate by gate on 128-bit wire labels (4 x u32 per lane)
        "dtype": "int%d" % w, "data": "synthetic",
        "config": {"workload": "phase-2 CGD solve, d=%d, %d iterations, %d-bit fixed point, precision %d, "
                               "two-party masked input (test_linear_system path), garbler+evaluator co-located; "
                               "one independent system per GPU" % (d, iters, w, p),
                   "d": d, "iterations": iters, "width": w, "precision": p, "sharding": "circuits x%d" % world},
        "and_gates_per_solve": gates, "gate_steps_per_solve": st["gate_steps"],
        "table_bytes_per_solve": st["table_bytes"], "launches_per_solve": st["launches"],
        "ref_equiv_gates_per_solve": refg,
        "ref_equiv_gates_per_s": (refg * args.steps * world / elapsed) if refg else None,
        "seconds_mac_garble_per_solve": mac_g / args.steps,
        "beta0": float(int(beta_fixed[0]) / scale),
    }
    if not args.full:
        solver.close()
        if rank == 0:
            print(compact_line(out), flush=True)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ---- --full from here on
    # one extra pass outside the timed region with the garbler and evaluator chains serialised:
    # exclusive per-kernel durations (HIP events on the launching stream)
    solver.run(profile=True)
    stx = solver.stats()
    # the table ring of this solver is its one large allocation (largest launch + 8 GiB: 69 GB at d = 500).  close() parks
    # it for the next solver on this device -- the sweep below takes it over instead of allocating its own
    solver.close()

    # ---- BASELINE config 5: the 64-lambda sweep of the d=100 CGD-15 circuit, sharded over the ranks.  The
    # lambda-independent prefix (input labels + garbled share summation) is garbled on rank 0 and broadcast
    # (RCCL over xGMI at N > 1), every rank runs its contiguous block as one merged program, all_gather
    # collects the results (python/sweep.py).  Timed like the main region: barrier + synchronize, max over ranks.
    sweep_res = None
    sweep_check = None
    if not args.no_sweep:
        import sweep
        sd, sit, nl = args.sweep_d, args.sweep_iters, args.sweep_lambdas
        srng = np.random.default_rng(5)
        sT = sd * (sd + 1) // 2
        sn = 4 * sd
        sX = srng.standard_normal((sn, sd)); sX /= np.abs(sX).max(axis=0)
        sy = sX @ srng.random(sd) + 0.1 * srng.standard_normal(sn)
        sA = sX.T @ sX / sn; sb = sX.T @ sy / sn                       # aggregate before the in-circuit division by d
        stot = np.concatenate([[int(sA[i, j] * scale) for i in range(sd) for j in range(i + 1)],
                               [int(v * scale) for v in sb]]).astype(np.int64).astype(np.uint64)
        smask = srng.integers(0, 2 ** 63, size=stot.size, dtype=np.uint64)
        with np.errstate(over="ignore"):
            sshares = np.stack([stot - smask, smask])
        if w == 32:
            sshares &= np.uint64(0xffffffff)
        lams = sweep.c5_lambdas(nl)
        make = sweep.gpu_block_solver_factory(sd, w, p, "cgd", sit, 2, device_index)
        # warm-up: at N > 1 with the blocks of the timed run, so that every rank's table ring is already parked at full size
        # (a fresh hipMalloc of a block's 42 GB ring is 0.27 s against 1.07 s of kernels); at N = 1 two circuits do
        warm = lams if (world > 1 and (nl + world - 1) // world <= 16) else lams[:max(2 * world, 2)]
        sweep.shared_prefix_sweep(sshares if rank == 0 else None, warm, sd, make, dist=dist, tensor_device="cuda")
        barrier()
        ts = time.perf_counter()
        sst = {}
        sres = sweep.shared_prefix_sweep(sshares if rank == 0 else None, lams, sd, make, dist=dist, tensor_device="cuda", stats=sst)
        barrier()
        sdt = time.perf_counter() - ts
        phase_keys = ("create_s", "prefix_garble_s", "broadcast_s", "block_s", "gather_s")
        phases = [float(sst.get(k, 0.0)) for k in phase_keys]
        if dist is not None:
            tmax = torch.tensor([sdt] + phases, dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            sdt = float(tmax[0].item())
            phases = [float(v) for v in tmax[1:].tolist()]
        dump = os.environ.get("LGC_BENCH_DUMP")
        if dump:                                                   # tests: what every rank holds after the gather
            json.dump({"rank": rank, "lambdas": lams, "beta": sres.tolist(), "shares": sshares.tolist(), "d": sd, "iters": sit,
                       "width": w, "precision": p}, open(os.path.join(dump, "sweep_rank%d.json" % rank), "w"))
        if rank == 0:
            sprog = lgc.Program(lgc.make_system(sd, w, p, "cgd", sit, 0.0, 2, 1, 0, 0), lambdas=lams)
            sgates = int(sprog.info.total_gates)
            sweep_res = {"lambdas": nl, "d": sd, "iterations": sit, "n_gpus": world, "seconds": sdt,
                         "circuits_per_s": nl / sdt, "and_gates": sgates, "and_gates_per_s": sgates / sdt,
                         "prefix_bytes_broadcast": sst.get("prefix_bytes") if world > 1 else 0,
                         # wall-clock of each phase, max over ranks (python/sweep.py): solver creation on every rank at once;
                         # rank 0 garbles + exports the prefix while the others wait at the broadcast with their buffers
                         # allocated; the broadcast itself as rank 0 sees it; this rank's block; the result gather
                         **dict(zip(phase_keys, phases)),
                         "collectives": ("broadcast(seed, garbled prefix) + all_gather(results) over %s" % backend) if world > 1 else None,
                         "sharding": "contiguous blocks of %d lambdas per rank; prefix (input labels + share-summation and normalizer tables) garbled once on rank 0" % ((nl + world - 1) // world)}
            sweep_res["block_lambdas"] = (nl + world - 1) // world
            sweep_check = (stot, sT, sd, sit, lams, sres, nl)      # compared with the oracle in the cpu_baseline leg
            if world > 1:
                # what the N = 1 run's model said this N would take (sweep_model, below): from the N = 1 detail file when that run
                # left one beside us, else from the committed profile of the builder's last N = 1 run -- so that the first
                # real multi-GPU run shows measured / predicted in its own line
                pred, src = load_sweep_prediction(world, nl, sd, sit)
                if pred is not None:
                    sweep_res["predicted_seconds"] = pred
                    sweep_res["measured_over_predicted"] = sdt / pred
                    sweep_res["predicted_from"] = src
            if world == 1 and not args.no_sweep_model and nl >= 16:
                sweep_res["model"] = sweep_model(np, sweep, sshares, lams, sd, make, sdt, sst)

    lgc.release_cached_memory()          # the separate-process runs below bring their own rings
    if world == 1 and not args.no_e2e:
        # the driver wipes released device memory in the background (tens of GB here) and an allocation made meanwhile may wait
        # for it (profiles/r4_hip_exit.txt: 0.25 s for 11 GB taken right after 11 GB were freed, 0.3 ms two seconds later):
        # let it finish before the end-to-end runs start, and give every run's own memory a moment as well (phase12_wall)
        time.sleep(4.0)
    if rank == 0:
        # ---- roofline of the dominant kernel (garbling of the MAC launches), HIP events on its stream
        prog = lgc.Program(sysm)
        macL = [L for L in prog.launches() if L["mac_only"]]
        recs = np.frombuffer(prog.records().tobytes(), dtype=np.dtype([
            ("op", "<u4"), ("cnt", "<u4"), ("dst", "<u4"), ("a", "<u4"), ("b", "<u4"), ("c", "<u4"),
            ("sa", "<i4"), ("sb", "<i4"), ("step0", "<u8")]))
        mac_gates = sum(L["gates"] for L in macL)
        mac_products = int(sum(int(recs["cnt"][L["first_rec"]:L["first_rec"] + L["nrec"]].sum()) for L in macL))
        mac_recs = sum(L["nrec"] for L in macL)
        karatsuba = bool(macL) and int(recs["op"][macL[0]["first_rec"]]) == 20          # OP_MACK records (gc_mack_kernel)
        # algorithmic HBM bytes of the garbling MAC kernel: 32 B of garbled table per AND gate written; operand words
        # (1 KiB each) read per product: 2 for the plain array, 6 for a Karatsuba product (a pair reads both halves of
        # a, b and of their half-difference words -- eight packed 1 KiB loads -- and a, b again for the sign
        # corrections); 2 words written per record
        alg_bytes_per_solve = 32 * mac_gates + (6144 if karatsuba else 2048) * mac_products + 2048 * mac_recs
        n_launch_per_solve = max(1, len(macL))
        avg_dur = mac_g / max(1, mac_launches)
        alg_bytes_per_launch = alg_bytes_per_solve / n_launch_per_solve
        achieved = alg_bytes_per_launch / avg_dur / 1e9 if avg_dur > 0 else 0.0
        aes_rate = max(lgc.aes_bench(65536, 256, device=device_index)[0] for _ in range(3))
        # 160 ds_read_b32 lookups per block, 2 LDS cycles per wave-instruction (MI355X_MICROARCH.md, LDS),
        # 256 CUs x 64 lanes at the 2.4 GHz peak clock: an upper bound no T-table kernel can exceed
        lds_roof = 256 * 64 * 2.4e9 / (160 * 2)
        # exclusive (serialised) pass: 4 AES per AND garbling, 2 evaluating
        xg, xe = stx["seconds_mac_garble"], stx["seconds_mac_eval"]
        aes_achieved = 4.0 * mac_gates / xg if xg > 0 else 0.0
        aes_achieved_eval = 2.0 * mac_gates / xe if xe > 0 else 0.0
        achieved_excl = alg_bytes_per_launch / (xg / n_launch_per_solve) / 1e9 if xg > 0 else 0.0
        # SURVEY.md 8(d) asks for both readings: the word machine's own traffic (labels stay on chip: 32 B of table per
        # AND each way -- `achieved` / `frac` above) and what a flat gate list of the same circuit would move:
        # 96 B per AND and 64 B per XOR on each side, every label through HBM
        n_xor = int(prog.info.total_xors)
        flat_bytes = 192.0 * gates + 128.0 * n_xor
        step_s = elapsed / args.steps
        roofline = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_detail": traffic_detail,
                    "binding": "lds_aes",
                    "flat_list_equiv": {"bytes_per_solve": flat_bytes, "GBs": flat_bytes / step_s / 1e9,
                                        "required_over_peak": flat_bytes / step_s / 1e9 / HBM_PEAK_GBS,
                                        "formula": "192 N_AND + 128 N_XOR over the whole solve / seconds per solve: what a flat gate "
                                                   "list WOULD have to stream to keep this pace (not achieved bandwidth; > 1 = more than the HBM delivers)",
                                        "n_and": gates, "n_xor": n_xor,
                                        "n_xor_rule": "word-level XORs of two wire words x width (lane moves, public selects, inverters = wiring)"},
                    "kernel": "gc_mack_kernel<garbler>" if karatsuba else "gc_mac_kernel<garbler>", "avg_launch_ms": avg_dur * 1e3,
                    "alg_bytes_per_launch": alg_bytes_per_launch,
                    "achieved_exclusive": achieved_excl, "avg_launch_ms_exclusive": xg / n_launch_per_solve * 1e3,
                    "timing": "achieved: HIP events on the garbler stream over the timed region (large MAC launches "
                              "alternate with their evaluator launches; small launches of the two chains overlap); "
                              "*_exclusive: the same kernels in a fully serialised pass",
                    "note": "integer/bitwise kernel bound by LDS T-table AES issue, not HBM: see aes_roofline"}
        aes_roofline = {"achieved": aes_achieved, "achieved_eval_kernel": aes_achieved_eval,
                        "peak": lds_roof, "unit": "AES-128 blocks/s", "frac": aes_achieved / lds_roof,
                        "frac_eval_kernel": aes_achieved_eval / lds_roof,
                        "peak_source": "LDS lookup roof: 256 CUs x 64 lanes x 2.4 GHz / (160 ds_read_b32 x 2 LDS cycles)",
                        "micro_kernel": aes_rate,
                        "micro_kernel_source": "lgc_aes_bench (stand-alone four-table AES kernel), best of 3 in this run"}
        # ---- OT-extension accounting (replaces honestCorrelatedOTExt{Send,Recv}1Of2, src/phase1.c:58-65, 84-89):
        # the Gilboa batches of config 3's --use_ot phase 1 through the C ABI with every operand resident in HBM
        ot_res = None
        if world == 1 and not args.no_e2e:
            try:
                ot_res = ot_accounting(np, torch, lgc)
            except Exception as e:
                ot_res = {"error": str(e)}
        # the second half of the metric string and the deployment-shaped rate, measured in this run
        e2e, ring = None, None
        if world == 1 and not args.no_e2e:
            import shutil as _sh
            warm = phase12_wall(np, "warm-up", 200, 4, [0, 2], "cholesky", 0, ["--table_ring"], device_index)   # untimed: pages the binaries in
            if warm.get("_check"):
                _sh.rmtree(warm["_check"]["tmp"], ignore_errors=True)
            # every party runs on this box, so every bulk message may stay in HBM: --table_ring (garbled tables), --ti_ring / --ot_ring
            # (phase 1), --input_ring (the label OT of phase 2)
            e2e = [phase12_wall(np, "c2", 1000, 20, [0, 10], "cholesky", 0, ["--table_ring", "--input_ring"], device_index),
                   phase12_wall(np, "c3-ti", 10000, 100, [0, 50], "cgd", 15, ["--ti_ring", "--input_ring", "--table_ring"], device_index),
                   # BASELINE config 3 proper: --use_ot phase 1 (1.6e9 extended OTs); all parties are on this node,
                   # so the bulk messages of both phases stay in HBM (--ot_ring = --use_ot through device rings)
                   phase12_wall(np, "c3-ot", 10000, 100, [0, 50], "cgd", 15, ["--ot_ring", "--input_ring", "--table_ring"], device_index),
                   # config 1: the reference's own example (README.md:81), five processes
                   phase12_wall(np, "c1", 10, 5, [0, 1, 2], "cgd", 10, ["--ti_ring", "--input_ring", "--table_ring"], device_index,
                                source=os.path.join(ROOT, "tests", "golden", "readme_example.in"))]
            if not args.no_c4:
                # config 4: phase 1 in 64 bits, phase 2 in 32 (every share shifted on its own, phase1.c:609-638), with three
                # data providers rather than the config's five: with the CSP, the Evaluator and this process that is six
                # processes on the GPU, the most the bench puts there at once.
                # bin/linreg_testhooks = bin/linreg plus ONE getenv that pins the TI's seed, so that the checker can replay the
                # TI stream and compare the Result line exactly (what a share-level check needs; tests/test_gpu_configs.py)
                e2e.append(phase12_wall(np, "c4", 50000, 500, [0, 167, 334], "cgd", 20,
                                        ["--width_phase2=32", "--prec_phase2=30", "--ti_ring", "--input_ring", "--table_ring"], device_index,
                                        exe_name="linreg_testhooks", env_extra={"LINREG_TI_SEED": bytes(range(0x60, 0x70)).hex()},
                                        prec2=30, w2=32))
            if (w, p) == (64, 56):
                ring = two_process_ring(np, d, iters, p, Af, bf, gates, device_index)
        # ---- cpu_baseline leg: the only part of this script that imports, links or runs anything under oracle/.
        # (1) the baseline itself: the CPU mirror of the garbling protocol, timed on a bounded sample;
        # (2) the oracle as CHECKER of what the runs above produced (never of anything that is timed).
        cpu = None
        if not args.no_cpu_baseline and world == 1:
            import gccpu
            g = gccpu.load()
            # bounded sample of the same workload: OP_MAC records (the 90+ % unit of the circuit)
            # two DISTINCT physical cores (not SMT siblings), pinned: left to the scheduler the pair sometimes shared one core's
            # AES units and sometimes did not -- 8.3e7 (r02) against 5.2e7 (r03) AND-gates/s on the same CPU model
            cpus, cpu_note = pick_two_cores()
            rate1, _, s1 = g.baseline_mac(w, p, 40, 4, cpus)
            nrec = max(40, int(40 * (args.cpu_seconds / 3.0) / max(s1, 1e-3)))
            reps = [g.baseline_mac(w, p, nrec, 4, cpus) for _ in range(3)]
            rates = sorted(r_[0] for r_ in reps)
            cg, cs = reps[0][1], sum(r_[2] for r_ in reps)
            model, total_cores = cpu_info()
            cpu = {"value": rates[1], "unit": "AND-gates/s", "cores": 2, "kind": "port", "model": model, "total_cores": total_cores,
                   "repeats": {"min": rates[0], "median": rates[1], "max": rates[2], "spread": (rates[2] - rates[0]) / rates[1]},
                   "pinned_cpus": list(cpus), "pinning": cpu_note,
                   "sample": "3 x %d OP_MAC records x 4 products (%d AND gates each, %.1f s in all): AES-NI half-gates, one "
                             "garbler thread + one evaluator thread, gates in program order; value = the median" % (nrec, cg, cs)}
            try:
                import orc
                from helpers import oracle_solve
                orc_ = orc.load()
                # a WHOLE solve beside the MAC records: d = 100 CGD-1 (input labels, share sums, dividers, inner products,
                # the matrix-vector product, reveals) through the CPU garbler and evaluator, launch by launch on ONE thread
                # (garble launch k, evaluate launch k), decoded result checked against the oracle
                wd, wit = 100, 5
                wrng = np.random.default_rng(77)
                wX = wrng.standard_normal((4 * wd, wd)); wX /= np.abs(wX).max(axis=0)
                wy = wX @ wrng.random(wd) + 0.1 * wrng.standard_normal(4 * wd)
                wA = wX.T @ wX / (4 * wd * wd) + np.eye(wd) * 1e-3; wb = wX.T @ wy / (4 * wd * wd)
                wtot = np.concatenate([[int(wA[i, j] * scale) for i in range(wd) for j in range(i + 1)],
                                       [int(v * scale) for v in wb]]).astype(np.int64).astype(np.uint64)
                wmask = wrng.integers(0, 2 ** 63, size=wtot.size, dtype=np.uint64)
                if w == 32:
                    wtot &= np.uint64(0xffffffff); wmask &= np.uint64(0xffffffff)
                with np.errstate(over="ignore"):
                    wsh = np.stack([wtot - wmask, wmask])
                if w == 32:
                    wsh &= np.uint64(0xffffffff)
                wprog = lgc.Program(lgc.make_system(wd, w, p, "cgd", wit, 0.0, 2, 0, 0, 0))
                tw0 = time.perf_counter()
                wdec, wgates, _ = g.garble_eval(wprog, wsh, seed=bytes(range(16)))
                wsec = time.perf_counter() - tw0
                wT = wd * (wd + 1) // 2
                wexp, _, _ = oracle_solve(orc_, wtot[:wT], wtot[wT:], wd, w, p, "cgd", wit, 0.0, 0)
                wgot = wdec[wprog.info.rv_beta:wprog.info.rv_beta + wd]
                if w == 32:
                    wgot = wgot & np.uint64(0xffffffff)
                wmaskw = (1 << w) - 1
                cpu["whole_solve"] = {"value": wgates / wsec, "unit": "AND-gates/s", "cores": 1, "seconds": wsec, "and_gates": int(wgates),
                                      "circuit": "d=%d CGD-%d %d-bit" % (wd, wit, w),
                                      "exact": [int(v) & wmaskw for v in wgot] == [int(v) & wmaskw for v in wexp],
                                      "sample": "one whole solve, every launch garbled then evaluated on one thread (AES-NI); the "
                                                "two-thread pipeline of `value` is the reference's structure, this is the whole circuit"}
                for res in (e2e or []):
                    ck = res.get("_check")
                    if ck and ck["w2"] == 64:
                        beta = orc_.linreg_file(ck["path"], ck["prec"], -1, 64, 64, {"cholesky": 0, "ldlt": 1, "cgd": 2}[ck["alg"]], ck["iters"], 0.001)
                        res["exact_vs_oracle"] = ck["got"] == ["%.15f" % (int(v) / 2.0 ** ck["prec"]) for v in beta]
                    elif ck:
                        # 64 -> 32 bits: the result depends on the individual shares, so the oracle replays the pinned TI stream
                        # pair by pair and converts share by share (src/phase1.c:609-638)
                        tck = time.perf_counter()
                        seed_ = bytes.fromhex(ck["ti_seed"])
                        n_, d_, p1_, p2_ = ck["n"], ck["d"], ck["prec"], ck["prec2"]
                        inp = orc_.read_input(ck["path"])
                        Xq = orc_.quantize(inp["X"], p1_, n_, 32); yq = orc_.quantize(inp["y"], p1_, n_, 32)
                        sA, sb, _ = orc_.ti_shares_stream(Xq.reshape(n_, d_), yq, n_, d_, p1_, 64, ck["starts"],
                                                          lambda first, count: g.ti_stream_words(seed_, first, count, 64))
                        cA = np.stack([orc_.convert_shares(r_, p1_, p2_, 64, 32) for r_ in sA])
                        cb = np.stack([orc_.convert_shares(r_, p1_, p2_, 64, 32) for r_ in sb])
                        a_, bb_ = orc_.circuit_input(orc_.sum_shares(cA, 32), orc_.sum_shares(cb, 32), d_, 0.001, p2_, 32)
                        beta = orc_.cgd(a_, bb_, d_, p2_, 32, ck["iters"])
                        res["exact_vs_oracle"] = ck["got"] == ["%.15f" % (int(v) / 2.0 ** p2_) for v in beta]
                        res["check_seconds"] = time.perf_counter() - tck
                if sweep_res is not None and sweep_check is not None:
                    stot_, sT_, sd_, sit_, lams_, sres_, nl_ = sweep_check
                    ok = True
                    for k in (0, nl_ - 1):
                        exp, _, _ = oracle_solve(orc_, stot_[:sT_], stot_[sT_:], sd_, w, p, "cgd", sit_, lams_[k], 1)
                        ok = ok and [int(v) for v in exp] == [int(v) for v in sres_[k]]
                    sweep_res["exact_vs_oracle"] = ok
            except Exception as e:
                cpu["checker_error"] = str(e)
        # the headline solve itself against the oracle (after all timing; the oracle solves d = 500 in seconds)
        headline_exact = None
        if not args.no_cpu_baseline and world == 1:
            try:
                import orc
                from helpers import oracle_solve
                expb, _, _ = oracle_solve(orc.load(), tot[:T], tot[T:], d, w, p, "cgd", iters, 0.0, 0)
                headline_exact = [int(v) for v in expb] == [int(v) for v in beta_fixed]
            except Exception as e:
                headline_exact = "checker error: %s" % e
        import shutil
        for res in (e2e or []):
            ck = res.pop("_check", None)
            if ck:
                shutil.rmtree(ck["tmp"], ignore_errors=True)
        out.update({
            "n_xor_per_solve": n_xor, "exact_vs_oracle": headline_exact,
            "seconds_exclusive_per_solve": {"mac_garble": xg, "mac_eval": xe, "all_garble": stx["seconds_garble"],
                                            "all_eval": stx["seconds_eval"]},
            "roofline": roofline, "aes_roofline": aes_roofline, "cpu_baseline": cpu, "ot": ot_res,
            "phase12": e2e, "two_process_ring": ring, "sweep64": sweep_res,
        })
        # the full record goes to a side file (and nowhere near stdout); stdout gets ONE compact line
        ddir = os.environ.get("LGC_BENCH_DETAIL_DIR") or os.getcwd()
        dname = "bench_detail.json" if world == 1 else "bench_detail_n%d.json" % world
        out["detail_file"] = dname
        try:
            with open(os.path.join(ddir, dname), "w") as f:
                json.dump(out, f, indent=1)
        except OSError as e:                      # a read-only working directory must not cost the line
            out["detail_file"] = "not written: %s" % e
        print(compact_line(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
