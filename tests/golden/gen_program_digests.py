#!/usr/bin/env python3
"""Pins the lowered programs and the build-time rejections of the product library.

    python tests/golden/gen_program_digests.py     # rewrites tests/golden/program_digests.json

For every program of a fixed matrix (programs()) the JSON holds sha256 digests of its records, of its launch list and of
every lgc_program_info field; for every invalid request (rejections()) the (code, message) that Program, Solver and Party
creation return.  Every rejection happens before any device lookup, so all of it runs without a GPU.
tests/test_program_digests.py rebuilds both and compares."""
import ctypes as C
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "program_digests.json")

WP = {64: 56, 32: 20}           # width -> precision
LAM, L1 = 0.125, 0.05


def _sys(lgc, d, w, alg, iters=0, normalize=0, reveal=0, trace=0, nshares=2, lam=LAM):
    return lgc.make_system(d, w, WP.get(w, 8), alg, iters, lam, nshares, normalize, reveal, trace)


def programs(lgc):
    """(name, builder, karatsuba) for every pinned program; builder(lgc) returns an lgc.Program"""
    out = []

    def add(name, fn, kara=True):
        out.append((name, fn, kara))

    for alg in ("cholesky", "ldlt", "cgd"):
        it = 3 if alg == "cgd" else 0
        for w in (32, 64):
            for d in (1, 5, 17, 100, 184):
                for nz in (0, 1):
                    add("%s w%d d%d norm%d reveal%s" % (alg, w, d, nz, " trace" if it else ""),
                        lambda lgc, a=alg, w=w, d=d, nz=nz, it=it: lgc.Program(_sys(lgc, d, w, a, it, nz, 1, 1 if it else 0)))
                    add("%s w%d d%d norm%d targets3" % (alg, w, d, nz),
                        lambda lgc, a=alg, w=w, d=d, nz=nz, it=it: lgc.Program(_sys(lgc, d, w, a, it, nz), targets=3))
    for w in (32, 64):
        for d in (1, 5, 17, 184):
            add("lasso w%d d%d trace" % (w, d), lambda lgc, w=w, d=d: lgc.Program(_sys(lgc, d, w, "lasso", 3, 1, 0, 1), l1=L1))
    add("dimcheck", lambda lgc: lgc.Program(_sys(lgc, 1, 64, "dimcheck")))
    add("cgd w64 d5 nshares3", lambda lgc: lgc.Program(_sys(lgc, 5, 64, "cgd", 2, 1, nshares=3)))
    add("cgd w64 d17 sweep_at first2", lambda lgc: lgc.Program(_sys(lgc, 17, 64, "cgd", 2, 1), lambdas=[0.1, 0.2, 0.3], first=2))
    add("cholesky w32 d5 sweep_at first1", lambda lgc: lgc.Program(_sys(lgc, 5, 32, "cholesky", 0, 1), lambdas=[0.5, 0.25], first=1))
    add("d500 cgd15", lambda lgc: lgc.Program(_sys(lgc, 500, 64, "cgd", 15, 1)))
    add("d500 lasso15", lambda lgc: lgc.Program(_sys(lgc, 500, 64, "lasso", 15, 1), l1=L1))
    add("d500 cholesky targets8", lambda lgc: lgc.Program(_sys(lgc, 500, 64, "cholesky", 0, 1), targets=8))
    add("d500 ldlt", lambda lgc: lgc.Program(_sys(lgc, 500, 64, "ldlt", 0, 1)))
    add("cgd w64 d100 no-karatsuba", lambda lgc: lgc.Program(_sys(lgc, 100, 64, "cgd", 3, 1)), False)
    add("cholesky w64 d184 no-karatsuba", lambda lgc: lgc.Program(_sys(lgc, 184, 64, "cholesky", 0, 1)), False)
    return out


def digest(prog):
    """sha256 of the records, of the launch list and of every lgc_program_info field"""
    info = {k: int(getattr(prog.info, k)) for k, _ in prog.info._fields_}
    h = lambda b: hashlib.sha256(b).hexdigest()
    return {"records": h(prog.records().tobytes()),
            "launches": h(json.dumps(prog.launches(), sort_keys=True).encode()),
            "info": h(json.dumps(info, sort_keys=True).encode())}


def build_digests(lgc):
    res, t_small, t_big = {}, 0.0, 0.0
    for name, fn, kara in programs(lgc):
        t0 = time.perf_counter()
        lgc.set_karatsuba(kara)
        try:
            prog = fn(lgc)
            res[name] = digest(prog)
            prog.close()
        finally:
            lgc.set_karatsuba(True)
        dt = time.perf_counter() - t0
        if name.startswith("d500"): t_big += dt
        else: t_small += dt
    return res, t_small, t_big


# invalid requests: (name, variant, system or None, argument of the variant).  variant: plain, targets (k), lasso (l1),
# sweep ((count, lambdas or None, first))
def rejections(lgc):
    s = lambda **kw: {**dict(d=5, w=64, alg="cgd", iters=2, normalize=1), **kw}
    sw = (3, [0.1, 0.2, 0.3], 0)
    return [
        ("null system", "plain", None, None),
        ("null system", "targets", None, 2),
        ("null system", "lasso", None, L1),
        ("null system", "sweep", None, sw),
        ("lasso without lambda1", "plain", s(alg="lasso"), None),
        ("width", "plain", s(w=48), None),
        ("precision negative", "plain", s(p=-1), None),
        ("precision = width", "plain", s(w=32, p=32), None),
        ("d = 0", "plain", s(d=0), None),
        ("d = 4097", "plain", s(d=4097), None),
        ("nshares = 0", "plain", s(nshares=0), None),
        ("algorithm 5", "plain", s(alg=5), None),
        ("algorithm -1", "plain", s(alg=-1), None),
        ("dimcheck d = 2", "plain", s(alg="dimcheck", d=2, normalize=0), None),
        ("dimcheck normalize", "plain", s(alg="dimcheck", d=1, normalize=1), None),
        ("cgd negative iterations", "plain", s(iters=-1), None),
        ("lasso call, cgd system", "lasso", s(), L1),
        ("lasso call, cgd system before width", "lasso", s(w=48), L1),
        ("lasso width", "lasso", s(alg="lasso", w=48), L1),
        ("lasso negative iterations", "lasso", s(alg="lasso", iters=-1), L1),
        ("lambda1 negative", "lasso", s(alg="lasso"), -0.5),
        ("lambda1 inf", "lasso", s(alg="lasso"), float("inf")),
        ("lambda1 nan", "lasso", s(alg="lasso"), float("nan")),
        ("lasso k = 2", "targets", s(alg="lasso"), 2),
        ("lasso k = 2 before width", "targets", s(alg="lasso", w=48), 2),
        ("lasso k = 1 through targets", "targets", s(alg="lasso"), 1),
        ("targets width", "targets", s(w=48), 2),
        ("k = 0", "targets", s(), 0),
        ("k = 257", "targets", s(), 257),
        ("dimcheck k = 2", "targets", s(alg="dimcheck", d=1, normalize=0), 2),
        ("trace k = 2", "targets", s(trace=1), 2),
        ("lasso sweep", "sweep", s(alg="lasso"), sw),
        ("lasso sweep before width", "sweep", s(alg="lasso", w=48), sw),
        ("sweep width", "sweep", s(w=48), sw),
        ("sweep null lambdas", "sweep", s(), (3, None, 0)),
        ("sweep count 0", "sweep", s(), (0, [0.1], 0)),
        ("sweep count 4097", "sweep", s(), (4097, [0.1] * 4097, 0)),
        ("sweep normalize 0", "sweep", s(normalize=0), sw),
        ("sweep trace", "sweep", s(trace=1), sw),
        ("sweep reveal", "sweep", s(reveal=1), sw),
        ("sweep d = 0 before lambdas", "sweep", s(d=0), (3, None, 0)),
    ]


def _raw_system(lgc, spec):
    if spec is None:
        return None
    kw = dict(spec)
    p = kw.pop("p", WP.get(kw["w"], 8))
    return lgc.make_system(kw["d"], kw["w"], p, kw["alg"], kw["iters"], LAM, kw.get("nshares", 2), kw["normalize"],
                           kw.get("reveal", 0), kw.get("trace", 0))


def _call(lgc, kind, variant, sysm, arg):
    """(rc, message) of one create call; kind: program, solver, party"""
    L = lgc.lib()
    h = C.c_void_p()
    sp = C.byref(sysm) if sysm is not None else None
    seed = bytes(range(16))
    L.lgc_party_create_sweep_at.restype = C.c_int           # (not in the binding)
    L.lgc_party_create_sweep_at.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.c_size_t,
                                            C.c_void_p, C.c_size_t]
    if variant == "sweep":
        count, lams, first = arg
        if lams is None:
            lp = None
        else:
            buf = (C.c_double * len(lams))(*lams)
            lp = C.cast(buf, C.c_void_p)
    if kind == "program":
        if variant == "plain": rc = L.lgc_program_build(C.byref(h), sp)
        elif variant == "targets": rc = L.lgc_program_build_targets(C.byref(h), sp, arg)
        elif variant == "lasso": rc = L.lgc_program_build_lasso(C.byref(h), sp, arg)
        else: rc = L.lgc_program_build_sweep_at(C.byref(h), sp, count, lp, first)
    elif kind == "solver":
        if variant == "plain": rc = L.lgc_solver_create(C.byref(h), 0, sp, seed)
        elif variant == "targets": rc = L.lgc_solver_create_targets(C.byref(h), 0, sp, seed, arg)
        elif variant == "lasso": rc = L.lgc_solver_create_lasso(C.byref(h), 0, sp, seed, arg)
        else: rc = L.lgc_solver_create_sweep_at(C.byref(h), 0, sp, seed, count, lp, first)
    else:
        if variant == "plain": rc = L.lgc_party_create(C.byref(h), 0, sp, 1, seed, 0)
        elif variant == "targets": rc = L.lgc_party_create_targets(C.byref(h), 0, sp, 1, seed, 0, arg)
        elif variant == "lasso": rc = L.lgc_party_create_lasso(C.byref(h), 0, sp, 1, seed, 0, arg)
        else: rc = L.lgc_party_create_sweep_at(C.byref(h), 0, sp, 1, seed, 0, count, lp, first)
    assert rc != 0 and not h.value, (kind, variant, rc)
    return [int(rc), L.lgc_last_error().decode()]


def build_rejections(lgc):
    res = {}
    for name, variant, spec, arg in rejections(lgc):
        for kind in ("program", "solver", "party"):
            res["%s: %s %s" % (kind, variant, name)] = _call(lgc, kind, variant, _raw_system(lgc, spec), arg)
    # the argument checks after validation (a valid system)
    L, sp, lam = lgc.lib(), C.byref(_raw_system(lgc, dict(d=5, w=64, alg="cgd", iters=2, normalize=1))), (C.c_double * 1)(0.1)
    h, seed = C.c_void_p(), bytes(range(16))
    for name, call in [("program: plain null out", lambda: L.lgc_program_build(None, sp)),
                     ("program: sweep null out", lambda: L.lgc_program_build_sweep_at(None, sp, 1, C.cast(lam, C.c_void_p), 0)),
                     ("solver: plain null seed", lambda: L.lgc_solver_create(C.byref(h), 0, sp, None)),
                     ("party: plain role 3", lambda: L.lgc_party_create(C.byref(h), 0, sp, 3, seed, 0)),
                     ("party: plain garbler without seed", lambda: L.lgc_party_create(C.byref(h), 0, sp, 1, None, 0))]:
        rc = call()
        assert rc != 0 and not h.value, name
        res[name] = [int(rc), L.lgc_last_error().decode()]
    return res


def main():
    root = os.path.dirname(os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(root, "linreg-mpc_amd", "python"))
    import linreg_gc as lgc
    progs, t_small, t_big = build_digests(lgc)
    rej = build_rejections(lgc)
    with open(OUT, "w") as f:
        json.dump({"programs": progs, "rejections": rej}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d programs (%d at d = 500: %.2f s; the others: %.2f s), %d rejections -> %s"
          % (len(progs), sum(1 for k in progs if k.startswith("d500")), t_big, t_small, len(rej), OUT))


if __name__ == "__main__":
    main()
