"""The pure-host plan of phase 1 (host/phase1_plan.c) without a GPU, through libhosttest.so: the cross-party pairs in the
initializer's loop order and in the OT modes' block order against the double loops written out here; a provider's view of its
pairs has one role per peer; the rule book of the phase-1 switches against the ordered rules bin/linreg had before the module
existed, over the full product of the switches; the three batch rules against their formulas; and the module under ASan + UBSan
as a program of its own (tests/tools/asan_phase1_plan.c)."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "linreg-mpc_amd", "host")

# (d, first column of every provider, M): the README example (the middle provider is party a towards one peer and b towards the
# other); a provider with no columns; one provider (no pairs); a candidate block inside one provider, ending at the boundary,
# crossing it, and M = d - 1
LAYOUTS = [(5, (0, 2, 4), 0), (4, (0, 0, 2), 0), (3, (0,), 0)] + [(6, (0, 3), M) for M in (0, 2, 3, 5)]
IDS = ["d%d-%s-M%d" % (d, "_".join(map(str, st)), M) for d, st, M in LAYOUTS]


class Pair(C.Structure):
    _fields_ = [("pa", C.c_int), ("pb", C.c_int), ("ci", C.c_uint32), ("cj", C.c_uint32)]


class View(C.Structure):
    _fields_ = [("peer", C.c_int), ("is_a", C.c_int), ("col", C.c_uint32)]


class Flags(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("use_ot", "ot_ring", "ti_ring", "ti_matrix", "ot_matrix", "ot_half", "scan", "folds")]


class Mode(C.Structure):
    _fields_ = [("transport", C.c_int), ("scan", C.c_size_t), ("folds", C.c_size_t)]


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-C", HOST, "libhosttest.so"], stdout=subprocess.DEVNULL)
    L = C.CDLL(os.path.join(HOST, "libhosttest.so"))
    L.p1_plan_ti.restype = C.c_size_t
    L.p1_plan_ti.argtypes = [C.POINTER(C.c_int), C.c_size_t, C.c_size_t, C.POINTER(C.POINTER(Pair))]
    L.p1_pair_view.argtypes = [C.POINTER(Pair), C.c_int, C.POINTER(View)]
    L.p1_plan_ot.restype = C.c_size_t
    L.p1_plan_ot.argtypes = [C.c_size_t] * 4 + [C.c_int] + [C.c_size_t] * 2 + [C.c_int] + [C.POINTER(C.POINTER(C.c_size_t))] * 2
    L.p1_mode_check.restype = C.c_char_p
    L.p1_mode_check.argtypes = [C.POINTER(Flags)]
    L.p1_transport_of.argtypes = [C.POINTER(Flags)]
    L.p1_mode_refuses.restype = C.c_char_p
    L.p1_mode_refuses.argtypes = [C.POINTER(Mode)]
    for f in (L.p1_ti_batch_pairs, L.p1_ring_batch_pairs, L.p1_ot_batch_pairs):
        f.restype = C.c_size_t
    L.p1_ti_batch_pairs.argtypes = L.p1_ring_batch_pairs.argtypes = [C.c_size_t]
    L.p1_ot_batch_pairs.argtypes = [C.c_size_t, C.c_int, C.c_size_t]
    L.free = C.CDLL(None).free
    L.free.argtypes = [C.c_void_p]
    return L


# ---- the model: the loops as the host wrote them out before the module
def owners(d, starts):
    """config_owner: 0-based party indices, providers from 2; the last provider that starts at or before the column"""
    return [max(k + 2 for k, s in enumerate(starts) if k == 0 or s <= i) for i in range(d + 1)]


def skips(d, M, i, j):
    return bool(M) and i < d and j < d and i != j and i >= d - M and j >= d - M


def ti_order(d, starts, M):
    own = owners(d, starts)
    return [(own[i], own[j], i, j) for i in range(d + 1) for j in range(min(i + 1, d)) if own[i] != own[j] and not skips(d, M, i, j)]


def ot_orders(d, starts, M):
    """{(sender, receiver): [(ri, rj)]} for every provider pair, the sender by the rule of src/phase1.c:392"""
    NP, out = len(starts) + 2, {}
    last = NP - 1
    rng = lambda p: (starts[p - 2], starts[p - 1] if p < last else d)
    for lo in range(2, NP):
        for hi in range(lo + 1, NP):
            s = lo if (lo % 2 == hi % 2) == (lo < hi) else hi
            r = hi if s == lo else lo
            (i0, i1), (j0, j1) = rng(s), rng(r)
            lst = []
            for i in range(i0, i1):
                lst += [(i, j) for j in range(j0, j1) if not skips(d, M, i, j)]
                if r == last:
                    lst.append((i, d))
            if s == last:
                lst += [(d, j) for j in range(j0, j1)]
            out[(s, r)] = (lst, (i0, i1, s == last, j0, j1, r == last))
    return out


def host_ti(lib, d, starts, M):
    own = (C.c_int * (d + 1))(*owners(d, starts))
    p = C.POINTER(Pair)()
    n = lib.p1_plan_ti(own, d, M, C.byref(p))
    assert n != C.c_size_t(-1).value
    got = [(p[q].pa, p[q].pb, p[q].ci, p[q].cj) for q in range(n)]
    return got, p, n


@pytest.mark.parametrize("d,starts,M", LAYOUTS, ids=IDS)
def test_ti_order_is_the_double_loop(lib, d, starts, M):
    got, p, n = host_ti(lib, d, starts, M)
    lib.free(p)
    want = ti_order(d, starts, M)
    assert got == want
    assert (n == 0) == (len(starts) == 1)
    assert all(pa > pb and ci >= cj for pa, pb, ci, cj in got)          # the later party holds the higher column: it is party a


@pytest.mark.parametrize("d,starts,M", LAYOUTS, ids=IDS)
def test_a_view_is_a_filter_with_one_role_per_peer(lib, d, starts, M):
    got, p, n = host_ti(lib, d, starts, M)
    for me in range(2, len(starts) + 2):
        roles, mine = {}, []
        for q in range(n):
            v = View()
            if lib.p1_pair_view(C.byref(p[q]), me, C.byref(v)):
                mine.append((v.peer, v.is_a, v.col))
                roles.setdefault(v.peer, set()).add(v.is_a)
        want = [(pb, 1, ci) if pa == me else (pa, 0, cj) for pa, pb, ci, cj in got if me in (pa, pb)]
        assert mine == want
        assert all(len(r) == 1 for r in roles.values()), (me, roles)
        assert all(r == {int(me > peer)} for peer, r in roles.items())
        if (d, starts, me) == (5, (0, 2, 4), 3):                        # the README example's middle provider plays both roles
            assert roles == {2: {1}, 4: {0}}
    lib.free(p)


@pytest.mark.parametrize("d,starts,M", LAYOUTS, ids=IDS)
def test_ot_block_order_of_every_provider_pair(lib, d, starts, M):
    cross = set()
    for (s, r), (want, (i0, i1, ys, j0, j1, yr)) in ot_orders(d, starts, M).items():
        ri, rj = C.POINTER(C.c_size_t)(), C.POINTER(C.c_size_t)()
        n = lib.p1_plan_ot(d, M, i0, i1, int(ys), j0, j1, int(yr), C.byref(ri), C.byref(rj))
        assert n == len(want)
        assert [(ri[q], rj[q]) for q in range(n)] == want
        assert bool(ri) == bool(n) and bool(rj) == bool(n)
        lib.free(ri); lib.free(rj)
        cross |= {(max(a, b), min(a, b)) for a, b in want}
    # both orders hold the same pairs of columns: what one transport shares, every transport shares
    assert cross == {(i, j) for _, _, i, j in ti_order(d, starts, M)}


# ---- the rule book.  The rules of bin/linreg's option checks as they stood before the module, in their order; --ot_ring set
# both bits of its use_ot word, so "use_ot" there is --use_ot or --ot_ring
RULES = [
    (lambda f: f["ti_matrix"] and f["ot_ring"], b"--ti_matrix and --ot_ring exclude each other"),
    (lambda f: f["ti_matrix"] and (f["use_ot"] or f["ot_ring"]), b"--ti_matrix and --use_ot exclude each other (it is a mode of the trusted initializer)"),
    (lambda f: f["ti_matrix"] and f["ti_ring"], b"--ti_matrix and --ti_ring exclude each other"),
    (lambda f: f["ti_matrix"] and f["scan"], b"--ti_matrix and --scan exclude each other"),
    (lambda f: f["ot_half"] and not ((f["use_ot"] or f["ot_ring"]) and f["ot_matrix"]), b"--ot_half needs --use_ot --ot_matrix"),
    (lambda f: f["ot_matrix"] and f["ot_ring"], b"--ot_matrix and --ot_ring exclude each other"),
    (lambda f: f["ot_matrix"] and not (f["use_ot"] or f["ot_ring"]), b"--ot_matrix needs --use_ot (it is a mode of the OT-based phase 1)"),
    (lambda f: f["ot_matrix"] and f["scan"], b"--ot_matrix and --scan exclude each other"),
]
SWITCHES = ("use_ot", "ot_ring", "ti_ring", "ti_matrix", "ot_matrix", "ot_half", "scan")
TRANSPORTS = ("ti_sockets", "ti_ring", "ti_matrix", "ot_pairs", "ot_ring", "ot_matrix", "ot_half")


def test_mode_check_over_the_full_product_of_the_switches(lib):
    accepted = set()
    for bits in itertools.product((0, 1), repeat=len(SWITCHES)):
        for folds in (0, 1):
            f = dict(zip(SWITCHES, bits), folds=folds)
            want = next((msg for cond, msg in RULES if cond(f)), None)
            fl = Flags(**f)
            assert lib.p1_mode_check(C.byref(fl)) == want, f
            if want is None:
                t = TRANSPORTS[lib.p1_transport_of(C.byref(fl))]
                accepted.add(t)
                # the transport says what the switches said; --use_ot wins over --ti_ring, which no rule refuses
                ot = f["use_ot"] or f["ot_ring"]
                assert t == ("ot_half" if f["ot_half"] else "ot_matrix" if f["ot_matrix"] else "ot_ring" if f["ot_ring"] else "ot_pairs" if ot
                             else "ti_matrix" if f["ti_matrix"] else "ti_ring" if f["ti_ring"] else "ti_sockets"), f
    assert accepted == set(TRANSPORTS)


def test_a_mode_no_entry_point_runs(lib):
    """the ring transports move whole files in the full loop order, the matrix transports know no scan: refused with a message,
    whoever filled the struct"""
    for t, name in enumerate(TRANSPORTS):
        ring, matrix = name.endswith("ring"), "matrix" in name or name == "ot_half"
        for scan, folds in itertools.product((0, 3), (0, 4)):
            msg = lib.p1_mode_refuses(C.byref(Mode(t, scan, folds)))
            assert (msg is not None) == bool((ring and (scan or folds)) or (matrix and scan) or (scan and folds)), (name, scan, folds)


# ---- the batch rules
def test_batch_rules_at_their_clamps_and_inside(lib):
    clamp = lambda v, lo, hi: max(lo, min(v, hi))
    # result 1 (exactly, and clamped up from 0), result 1024 (exactly, and clamped down), one interior point
    for n in (1 << 23, 1 << 24, 1 << 13, 100, 50000):
        assert lib.p1_ti_batch_pairs(n) == clamp((64 << 20) // (n * 8), 1, 1024), n
    assert [lib.p1_ti_batch_pairs(n) for n in (1 << 23, 1 << 24, 1 << 13, 100, 50000)] == [1, 1, 1024, 1024, 167]
    for n in (1 << 25, 1 << 26, 1 << 15, 100, 50000):
        assert lib.p1_ring_batch_pairs(n) == clamp((256 << 20) // (n * 8), 1, 1024), n
    assert [lib.p1_ring_batch_pairs(n) for n in (1 << 25, 1 << 26, 1 << 15, 100, 50000)] == [1, 1, 1024, 1024, 671]
    # 2^24 OTs of n w per pair: result 1 (exactly, and from 0), per > npairs, inside
    for n, w, npairs in ((1 << 18, 64, 9), (1 << 20, 64, 9), (10, 32, 7), (50000, 64, 1000), (50000, 32, 1000), (50000, 64, 5), (50000, 64, 4)):
        assert lib.p1_ot_batch_pairs(n, w, npairs) == clamp((1 << 24) // (n * w), 1, npairs), (n, w, npairs)
    assert [lib.p1_ot_batch_pairs(*a) for a in ((1 << 18, 64, 9), (1 << 20, 64, 9), (10, 32, 7), (50000, 64, 1000), (50000, 32, 1000))] == [1, 1, 7, 5, 10]


# ---- under the sanitizers, as a program of its own
def test_plan_under_sanitizers(tmp_path):
    """host/phase1_plan.c compiled with ASan + UBSan into a program of its own and run on every layout: each list is allocated at
    exactly its size, so a count that disagrees with its fill is an overrun the run reports; nothing is loaded into python"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "asan_phase1_plan")
    cc = subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", HOST,
                         os.path.join(ROOT, "tests", "tools", "asan_phase1_plan.c"), os.path.join(HOST, "phase1_plan.c"), "-o", exe],
                        capture_output=True, text=True)
    if cc.returncode != 0 and "cannot find" in cc.stderr and "san" in cc.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert cc.returncode == 0, cc.stderr[-2000:]
    for d, starts, M in LAYOUTS:
        run = subprocess.run([exe, str(d), str(M)] + [str(s) for s in starts], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and run.stdout.rstrip().endswith("all ok"), (run.stdout[-1500:], run.stderr[-3000:])
        rows = [ln.split() for ln in run.stdout.splitlines()[:-1]]
        ti = [tuple(map(int, r[1:])) for r in rows if r[0] == "ti"]
        assert ti == ti_order(d, starts, M)
        views = [tuple(map(int, r[1:])) for r in rows if r[0] == "view"]
        assert views == [(me, pb, 1, ci) if pa == me else (me, pa, 0, cj) for me in range(2, len(starts) + 2) for pa, pb, ci, cj in ti if me in (pa, pb)]
        ot = {}
        for r in rows:
            if r[0] == "ot":
                ot.setdefault((int(r[1]), int(r[2])), []).append((int(r[3]), int(r[4])))
        assert ot == {k: v[0] for k, v in ot_orders(d, starts, M).items() if v[0]}
