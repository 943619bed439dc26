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
    for w in (32, 64):
        for nz in (0, 1):
            for name, d, iters, kw in lasso_matrix():
                add("lasso w%d norm%d %s" % (w, nz, name),
                    lambda lgc, w=w, nz=nz, d=d, iters=iters, kw=kw: lgc.Program(_sys(lgc, d, w, "lasso", iters, nz, 1), **kw))
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


ABS3, RAT3, RAT2 = [0.2, 0.1, 0.05], [0.5, 0.2, 0.05], [0.5, 0.1]
# options all at their defaults lower to the plain path, record for record (tests/test_program_digests.py compares the two)
DEFAULT_OPTS, PLAIN_PATH = "path abs default-opts d17 L3", "path abs d17 L3"


def lasso_options(d):
    """non-uniform penalty factors (one coordinate unpenalised), a few boxed coordinates and one one-sided bound"""
    inf = float("inf")
    pf = [(0.0, 0.5, 1.0, 2.0)[i % 4] for i in range(d)]
    lo = [-0.25 if i % 5 == 1 else 0.0 if i == 3 else -inf for i in range(d)]
    hi = [0.5 if i % 5 == 1 else inf for i in range(d)]
    return dict(penalty_factors=pf, lower=lo, upper=hi)


def lasso_matrix():
    """(name, d, iterations, Program arguments) of the lasso paths, selections and cross-validations pinned at both widths on
    both input paths, the inputs revealed: the smallest shapes that reach every branch of the input assembly and of the
    lasso lowering"""
    inf = float("inf")
    both = dict(reveal_index=True, reveal_scores=True)
    return [
        ("path abs d17 L3", 17, 3, dict(l1=ABS3)),
        ("path ratio d70 L2", 70, 3, dict(l1_ratios=RAT2)),                      # row sums in two chunks; the lambda_max tree
        ("path ratio opts d17 L3", 17, 3, dict(l1_ratios=RAT3, **lasso_options(17))),
        (DEFAULT_OPTS, 17, 3, dict(l1=ABS3, penalty_factors=[1.0] * 17, lower=[-inf] * 17, upper=[inf] * 17)),
        ("select abs opts d17 L3 flags0", 17, 3, dict(l1=ABS3, validation=True, **lasso_options(17))),
        ("select abs opts d17 L3 flags3", 17, 3, dict(l1=ABS3, validation=True, **both, **lasso_options(17))),
        ("select ratio d100 L2 flags3", 100, 3, dict(l1_ratios=RAT2, validation=True, **both)),   # w = 64: Karatsuba shadow
        ("select abs d5 L1 flags3", 5, 3, dict(l1=[L1], validation=True, **both)),
        ("cv2 abs opts d17 L3 flags3", 17, 3, dict(l1=ABS3, folds=2, **both, **lasso_options(17))),
        ("cv3 ratio d100 L2 flags1", 100, 3, dict(l1_ratios=RAT2, folds=3, reveal_index=True)),
        ("cv5 abs d5 L9 iters2 flags3", 5, 2, dict(l1=[0.4 * 0.7 ** k for k in range(9)], folds=5, **both)),   # two-level minimum tree
        ("cv4 abs d5 L1 flags3", 5, 3, dict(l1=[L1], folds=4, **both)),
    ]


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
# sweep ((count, lambdas or None, first)), path ((values or None, count, mode)), opts (the fields of lgc_lasso_opts, or None
# for a null pointer), select ((opts, reveal flags)), cv ((opts, folds, reveal flags))
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
    ] + _lasso_rejections(s)


def _lasso_rejections(s):
    """one invalid request per message of the path's, the options' and the selection / cross-validation checks"""
    la = lambda **kw: s(alg="lasso", **kw)
    inf, nan = float("inf"), float("nan")
    o = lambda l1=(0.1, 0.05), mode=0, **kw: dict(l1=list(l1), mode=mode, **kw)
    five = lambda v, at=2: [v if i == at else None for i in range(5)]         # (None: the field's default)
    pf = lambda v: dict(pf=[1.0 if x is None else x for x in five(v)])
    lo = lambda v: dict(lo=[-inf if x is None else x for x in five(v)])
    hi = lambda v: dict(hi=[inf if x is None else x for x in five(v)])
    return [
        ("null system", "path", None, ([0.1], 1, 0)),
        ("cgd system", "path", s(), ([0.1], 1, 0)),
        ("null values", "path", la(), (None, 2, 0)),
        ("count 0", "path", la(), ([0.1], 0, 0)),
        ("count 257", "path", la(), ([0.1] * 257, 257, 0)),
        ("mode 2", "path", la(), ([0.1], 1, 2)),
        ("value negative", "path", la(), ([0.1, -0.5], 2, 0)),
        ("value nan", "path", la(), ([nan], 1, 1)),
        ("ratio above 2", "path", la(), ([0.5, 2.5], 2, 1)),
        ("ratio beyond the precision", "path", la(w=32, p=30), ([2.0], 1, 1)),
        ("trace with two values", "path", la(trace=1), ([0.1, 0.05], 2, 0)),
        ("path checks before width", "path", la(w=48), ([0.1, -0.5], 2, 0)),
        ("width", "path", la(w=48), ([0.1], 1, 0)),
        ("null opts", "opts", la(), None),
        ("null system", "opts", None, o()),
        ("cgd system", "opts", s(), o()),
        ("null values", "opts", la(), dict(l1=None, count=2, mode=0)),
        ("penalty factor negative", "opts", la(), o(**pf(-1.0))),
        ("penalty factor inf", "opts", la(), o(**pf(inf))),
        ("bound nan", "opts", la(), o(**lo(nan))),
        ("lower +inf", "opts", la(), o(**lo(inf))),
        ("upper -inf", "opts", la(), o(**hi(-inf))),
        ("lower above upper", "opts", la(), o(**lo(0.5), **hi(0.25))),
        ("bound beyond the precision", "opts", la(w=32, p=20), o(**hi(1e6))),
        ("ratio times factor beyond the precision", "opts", la(w=32, p=30), o(l1=(1.5,), mode=1, **pf(2.0))),
        ("lambda1 times factor beyond the precision", "opts", la(w=32, p=20), o(l1=(1000.0,), **pf(1e4))),
        ("path checks before options", "opts", la(), o(l1=(0.1, -0.5), **pf(-1.0))),
        ("width before options", "opts", la(w=48), o(**pf(-1.0))),
        ("null opts", "select", la(), (None, 0)),
        ("null system", "select", None, (o(), 0)),
        ("reveal flags 4", "select", la(), (o(), 4)),
        ("trace", "select", la(trace=1), (o(l1=(0.1,)), 0)),
        ("trace with two values", "select", la(trace=1), (o(), 0)),
        ("options after the flags", "select", la(), (o(**pf(-1.0)), 4)),
        ("penalty factor negative", "select", la(), (o(**pf(-1.0)), 3)),
        ("null opts", "cv", la(), (None, 3, 0)),
        ("null system", "cv", None, (o(), 3, 0)),
        ("folds 0", "cv", la(), (o(), 0, 0)),
        ("folds 1", "cv", la(), (o(), 1, 0)),
        ("folds 17", "cv", la(), (o(), 17, 0)),
        ("folds before the flags", "cv", la(), (o(), 1, 4)),
        ("reveal flags 8", "cv", la(), (o(), 3, 8)),
        ("trace", "cv", la(trace=1), (o(l1=(0.1,)), 3, 0)),
        ("too large for 31-bit word ids", "cv", la(d=4096, nshares=16), (o(), 16, 0)),
        ("lower above upper", "cv", la(), (o(**lo(0.5), **hi(0.25)), 3, 3)),
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
    keep = []

    def dbl(v):
        if v is None:
            return None
        keep.append((C.c_double * len(v))(*v))
        return C.cast(keep[-1], C.c_void_p)
    if variant == "sweep":
        count, lams, first = arg
        lp = dbl(lams)
    if variant == "path":
        values, count, mode = arg
        lp = dbl(values)
    if variant in ("opts", "select", "cv"):
        o, extra = (arg, ()) if variant == "opts" else (arg[0], tuple(arg[1:]))
        if o is not None:
            keep.append(lgc.LassoOpts(o.get("count", len(o["l1"] or ())), dbl(o["l1"]), o["mode"], dbl(o.get("pf")), dbl(o.get("lo")),
                                      dbl(o.get("hi"))))
        op = C.byref(keep[-1]) if o is not None else None
        create = "lasso_" + variant
        if kind == "program": rc = getattr(L, "lgc_program_build_" + create)(C.byref(h), sp, op, *extra)
        elif kind == "solver": rc = getattr(L, "lgc_solver_create_" + create)(C.byref(h), 0, sp, seed, op, *extra)
        else: rc = getattr(L, "lgc_party_create_" + create)(C.byref(h), 0, sp, 1, seed, 0, op, *extra)
        assert rc != 0 and not h.value, (kind, variant, rc)
        return [int(rc), L.lgc_last_error().decode()]
    if kind == "program":
        if variant == "plain": rc = L.lgc_program_build(C.byref(h), sp)
        elif variant == "targets": rc = L.lgc_program_build_targets(C.byref(h), sp, arg)
        elif variant == "lasso": rc = L.lgc_program_build_lasso(C.byref(h), sp, arg)
        elif variant == "path": rc = L.lgc_program_build_lasso_path(C.byref(h), sp, count, lp, mode)
        else: rc = L.lgc_program_build_sweep_at(C.byref(h), sp, count, lp, first)
    elif kind == "solver":
        if variant == "plain": rc = L.lgc_solver_create(C.byref(h), 0, sp, seed)
        elif variant == "targets": rc = L.lgc_solver_create_targets(C.byref(h), 0, sp, seed, arg)
        elif variant == "lasso": rc = L.lgc_solver_create_lasso(C.byref(h), 0, sp, seed, arg)
        elif variant == "path": rc = L.lgc_solver_create_lasso_path(C.byref(h), 0, sp, seed, count, lp, mode)
        else: rc = L.lgc_solver_create_sweep_at(C.byref(h), 0, sp, seed, count, lp, first)
    else:
        if variant == "plain": rc = L.lgc_party_create(C.byref(h), 0, sp, 1, seed, 0)
        elif variant == "targets": rc = L.lgc_party_create_targets(C.byref(h), 0, sp, 1, seed, 0, arg)
        elif variant == "lasso": rc = L.lgc_party_create_lasso(C.byref(h), 0, sp, 1, seed, 0, arg)
        elif variant == "path": rc = L.lgc_party_create_lasso_path(C.byref(h), 0, sp, 1, seed, 0, count, lp, mode)
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
