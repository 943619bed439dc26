"""The pure-host description of a run of bin/linreg (host/linreg_run.c) without a GPU and without a process, through
libhosttest.so: the rule book against what the binary of the commit before the module said to every line of a corpus
(tests/golden/linreg_cli_rules.json); the rules that need the configuration on both sides of their edges; the phase-2 request, the
phase-1 job, the share layout and the result layout against values and models written out here; and the module under ASan + UBSan
as a program of its own (tests/tools/asan_linreg_run.c)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import pytest

from linreg_cli_corpus import INPUT, base, corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "linreg-mpc_amd", "host")
NONE = C.c_size_t(-1).value                     # RUN_NO_OFFSET


# ---- the module's structs (host/linreg_run.h, host/phase1_plan.h, include/linreg_gc.h, include/linreg_gc_lasso_opts.h)
class Flags(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("use_ot", "ot_ring", "ti_ring", "ti_matrix", "ot_matrix", "ot_half", "scan", "folds")]


class List(C.Structure):
    _fields_ = [("v", C.POINTER(C.c_double)), ("n", C.c_size_t)]


class Opts(C.Structure):
    _fields_ = ([(k, C.c_char_p) for k in ("input", "algorithm", "iterations")] + [(k, C.c_int) for k in ("precision", "party", "party_read")]
                + [("lam", C.c_double), ("fl", Flags)]
                + [(k, C.c_int) for k in ("w1", "w2", "prec_phase2", "ring_slots", "table_lanes", "input_ring")]
                + [("lambdas", List), ("l1", List), ("have_l1", C.c_int), ("have_ratios", C.c_int), ("positive", C.c_int), ("box", List * 3),
                   ("folds", C.c_long), ("scan", C.c_long)]
                + [(k, C.c_int) for k in ("reveal_index", "one_se", "reveal_curve", "inference", "no_se", "scan_se")]
                + [("devices", C.c_int * 16), ("n_devices", C.c_int), ("err", C.c_char_p)])


class System(C.Structure):
    _fields_ = [("d", C.c_size_t), ("width", C.c_int), ("precision", C.c_int), ("algorithm", C.c_int), ("num_iterations", C.c_int),
                ("lam", C.c_double), ("nshares", C.c_size_t), ("normalize", C.c_int), ("reveal_inputs", C.c_int), ("trace", C.c_int)]


class LassoOpts(C.Structure):
    _fields_ = [("l1_count", C.c_size_t), ("l1", C.POINTER(C.c_double)), ("l1_mode", C.c_int), ("penalty_factors", C.POINTER(C.c_double)),
                ("lower", C.POINTER(C.c_double)), ("upper", C.POINTER(C.c_double))]


class Mode(C.Structure):
    _fields_ = [("transport", C.c_int), ("scan", C.c_size_t), ("folds", C.c_size_t)]


class Job(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("precision", "precision_p2", "w1", "w2", "device")] + [("mode", Mode), ("want_yy", C.c_int)]


class Result(C.Structure):
    _fields_ = [(k, C.c_size_t) for k in ("words", "n_results", "result_len", "off_se", "off_fit", "off_index", "off_curve")]


class Plan(C.Structure):
    _fields_ = [("o", C.POINTER(Opts)), ("n", C.c_size_t), ("d", C.c_size_t), ("providers", C.c_int), ("device", C.c_int), ("n_blocks", C.c_int),
                ("sys", System), ("create", C.c_int), ("n_lambdas", C.c_size_t), ("lambdas", C.POINTER(C.c_double)), ("n_path", C.c_size_t),
                ("l1_mode", C.c_int), ("lasso", C.POINTER(LassoOpts)), ("folds", C.c_size_t), ("reveal", C.c_int), ("rule", C.c_int),
                ("infer", C.c_int), ("scan_M", C.c_size_t), ("scan_c", C.c_size_t), ("scan_bits", C.c_int), ("resid_scale", C.c_double),
                ("job", Job), ("table_chunk", C.c_size_t), ("share_words", C.c_size_t), ("result", Result), ("output", C.c_int),
                ("lasso_store", LassoOpts), ("zeros", C.POINTER(C.c_double)), ("err", C.c_char_p)]


CREATE = ("scan", "inference", "ridge_cv", "sweep_blocks", "sweep", "lasso_cv_se", "lasso_cv", "lasso_opts", "lasso_path", "lasso", "plain")
OUTPUT = ("full", "sweep", "cv", "scan")
TI_SOCKETS, OT_PAIRS = 0, 3                     # p1_transport
ABSOLUTE, RATIO = 0, 1                          # LGC_L1_*
REVEAL_INDEX, REVEAL_CURVE, RULE_MIN, RULE_ONE_SE, INFER_SE, INFER_FIT, SCAN_SE = 1, 4, 0, 1, 1, 2, 1
CHOLESKY, LDLT, CGD, LASSO = 0, 1, 2, 4


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-C", HOST, "libhosttest.so"], stdout=subprocess.DEVNULL)
    L = C.CDLL(os.path.join(HOST, "libhosttest.so"))
    L.run_opts_scan.restype = L.run_opts_check.restype = L.run_plan_build.restype = C.c_char_p
    L.run_opts_scan.argtypes = [C.POINTER(Opts), C.c_int, C.POINTER(C.c_char_p)]
    L.run_opts_check.argtypes = L.run_opts_free.argtypes = [C.POINTER(Opts)]
    L.run_opts_free.restype = L.run_plan_free.restype = None
    L.run_plan_build.argtypes = [C.POINTER(Plan), C.POINTER(Opts), C.c_size_t, C.c_size_t, C.c_int, C.c_int]
    L.run_plan_free.argtypes = [C.POINTER(Plan)]
    L.run_share_word.restype = C.c_uint64
    L.run_share_word.argtypes = [C.POINTER(Plan)] + [C.POINTER(C.c_uint64)] * 3 + [C.c_size_t]
    return L


class Run:
    """one command line through the module: .message is what bin/linreg would print (None: accepted), .plan the plan for
    (n, d, parties) when those are given and every rule passed"""

    def __init__(self, lib, args, shape=None, device=0):
        self.lib, self.opts, self.plan, self.planned = lib, Opts(), Plan(), False
        self.argv = (C.c_char_p * (len(args) + 2))(b"linreg", *[a.encode() for a in args], None)     # kept: the options point into it
        msg = lib.run_opts_scan(C.byref(self.opts), len(args) + 1, self.argv)
        if msg is None:
            msg = lib.run_opts_check(C.byref(self.opts))
        if msg is None and shape is not None:
            n, d, parties = shape
            msg = lib.run_plan_build(C.byref(self.plan), C.byref(self.opts), n, d, parties, device)
            self.planned = True
        self.message = None if msg is None else msg.decode()

    def close(self):
        if self.planned:
            self.lib.run_plan_free(C.byref(self.plan))
        self.lib.run_opts_free(C.byref(self.opts))


# ---- 1. the rule book against the binary before the module
with open(os.path.join(ROOT, "tests", "golden", "linreg_cli_rules.json")) as _f:
    GOLDEN = json.load(_f)

# the fixed text of every check(...) of the old main() ahead of config_new, in its order; where the format began with %s, once per
# option the corpus gives it.  The eight of p1_mode_check (a bare "%s" there) are spelled out
CHECKS = [
    "Usage: linreg [Input_file] [Precision] [Party] [Algorithm] [Num. iterations CGD] [Lambda] [Options]",
    "strtol: ", "Precision must be a number", "Party must be a number", "Algorithm must be cholesky, ldlt, cgd, or lasso.", "strtod: ",
    "lambda must be a number",
    "--lambdas wants a comma-separated list of numbers", "--lambdas wants at least one value",
    "--l1 is given twice", "--l1_ratios is given twice", "--l1 wants a comma-separated list of numbers",
    "--l1_ratios: every ratio must lie in [0, 2] (got ", "--l1 and --l1_ratios exclude each other",
    "--scan is given twice", "--scan wants a candidate count >= 1", "--folds is given twice", "--folds wants a number",
    "--lower is given twice", "--upper is given twice", "--penalty_factors is given twice", "--lower wants a comma-separated list of numbers",
    "--devices wants a comma-separated list of at most 16 device indices",
    "Bit widths must be 32 or 64", "Precision of phase 1 must be nonnegative", "Precision of phase 2 must be nonnegative",
    "Precision of phase 1 must be smaller than bit size of phase 1", "Precision of phase 2 must be smaller than bit size of phase 2",
    "--ti_matrix and --ot_ring exclude each other", "--ti_matrix and --use_ot exclude each other", "--ti_matrix and --ti_ring exclude each other",
    "--ti_matrix and --scan exclude each other", "--ot_half needs --use_ot --ot_matrix", "--ot_matrix and --ot_ring exclude each other",
    "--ot_matrix needs --use_ot", "--ot_matrix and --scan exclude each other",
    "Algorithm lasso needs --l1=<value>", "--l1 is for Algorithm lasso", "--l1_ratios is for Algorithm lasso", "--positive is for Algorithm lasso",
    "--lower is for Algorithm lasso", "--upper is for Algorithm lasso", "--penalty_factors is for Algorithm lasso",
    "--positive and --lower exclude each other", "a lasso path takes at most 256 values",
    "--folds is for Algorithm lasso", "--reveal_index belongs to --folds", "--one_se belongs to --folds", "--reveal_curve belongs to --folds",
    "--folds wants 2..16 folds (got ", "--folds selects among the values of a lasso path", "--folds and --lambdas exclude each other",
    "--folds cross-validates at most 256 values of --lambdas (got ", "--one_se and --reveal_curve are for the cross-validation of a lasso path",
    "--folds and --devices exclude each other", "--folds and --ti_ring exclude each other", "--folds and --ot_ring exclude each other",
    "--folds and --input_ring exclude each other",
    "--no_se belongs to --inference", "--inference is for Algorithm cholesky", "--inference and --folds exclude each other",
    "--inference and --lambdas exclude each other", "--inference and --devices exclude each other", "--inference and --ti_ring exclude each other",
    "--inference and --ot_ring exclude each other", "--inference and --input_ring exclude each other",
    "--scan_se belongs to --scan", "--scan is for Algorithm cholesky", "--scan and --lambdas exclude each other",
    "--scan and --inference exclude each other", "--scan and --devices exclude each other", "--scan and --ti_ring exclude each other",
    "--scan and --ot_ring exclude each other", "--scan and --input_ring exclude each other", "--scan takes at most 1048576 candidate columns",
    "--devices shards a --lambdas sweep and needs --table_ring",
]
# ... and the two that no command line of the corpus's form reaches
UNREACHED = {
    "--scan and --folds exclude each other": "--folds passes its own rules only beside --lambdas (a ridge cross-validation: --scan is cholesky's), "
                                             "and --scan refuses --lambdas one line earlier",
    "--devices: ": "lgc_devices_preflight's message: parties 1 and 2 only, it needs the library, and it stands behind the rule book, in main()",
}


def test_the_fixture_reaches_every_check_of_the_old_main():
    messages = GOLDEN["messages"][1:]
    assert GOLDEN["messages"][0] == "accepted" and GOLDEN["lines"] == len(GOLDEN["index"]) == len(corpus())
    missing = [c for c in CHECKS if not any(m.startswith(c) for m in messages)]
    assert not missing, missing
    assert not [m for m in messages if any(m.startswith(u) for u in UNREACHED)]
    stray = [m for m in messages if not any(m.startswith(c) for c in CHECKS)]
    assert not stray, stray                     # nothing the list above does not know
    assert 0 in GOLDEN["index"]                 # and lines that pass


def test_scan_and_check_say_what_the_binary_said(lib):
    said = GOLDEN["messages"]
    wrong = []
    for args, want in zip(corpus(), GOLDEN["index"]):
        r = Run(lib, args)
        got = r.message.split("\n")[0] if r.message is not None else "accepted"        # (of the usage text its first line, as recorded)
        if got != said[want]:
            wrong.append((args[3:], got, said[want]))
        r.close()
    assert not wrong, (len(wrong), wrong[:5])


def test_the_scan_keeps_what_was_said(lib):
    r = Run(lib, base("lasso", precision="24", iterations="7", lam="0.5") + ["--l1_ratios=1,0.5,0.25", "--upper=1,inf", "--penalty_factors=1,0", "--folds=3",
                                                                            "--one_se", "--table_ring=4", "--table_lanes=2", "--width_phase1=32",
                                                                            "--prec_phase2=40", "--use_ot", "--ot_matrix"])
    o = r.opts
    assert r.message is None
    assert (o.input, o.algorithm, o.iterations, o.precision, o.party, o.party_read, o.lam) == (INPUT.encode(), b"lasso", b"7", 24, 3, 1, 0.5)
    assert [getattr(o.fl, k) for k, _ in Flags._fields_] == [1, 0, 0, 0, 1, 0, 0, 1]
    assert (o.w1, o.w2, o.prec_phase2, o.ring_slots, o.table_lanes, o.input_ring) == (32, 64, 40, 4, 2, 0)
    assert (o.lambdas.n, o.have_l1, o.have_ratios, o.l1.v[:o.l1.n]) == (0, 0, 1, [1.0, 0.5, 0.25])
    assert (o.positive, o.box[0].n, o.box[1].v[:o.box[1].n], o.box[2].v[:o.box[2].n]) == (0, 0, [1.0, float("inf")], [1.0, 0.0])
    assert (o.folds, o.scan, o.reveal_index, o.one_se, o.reveal_curve, o.inference, o.no_se, o.scan_se, o.n_devices) == (3, 0, 0, 1, 0, 0, 0, 0, 0)
    r.close()
    r = Run(lib, base("cholesky") + ["--prec_phase2=30", "--devices=2,0,1", "--table_ring", "--lambdas=1,2", "--lambdas=3", "--no_such_option"])
    o = r.opts
    # (any option the scan does not know resets --prec_phase2, as it always has); --lambdas twice appends; plain --table_ring is the byte ring
    assert (o.prec_phase2, o.devices[:o.n_devices], o.ring_slots, o.lambdas.v[:o.lambdas.n]) == (-1, [2, 0, 1], 65, [1.0, 2.0, 3.0])
    r.close()


# ---- 2. the rules that need the configuration, in their order
def config_rules(n, d, box, K, inference, M, scan_se):
    """box: {option: entries}; K, M: 0 without --folds / --scan"""
    for opt in ("--lower", "--upper", "--penalty_factors"):
        if opt in box and box[opt] != d:
            return "%s wants d = %d entries (got %d)" % (opt, d, box[opt])
    if K > n:
        return "--folds=%d: more folds than the %d rows of the input" % (K, n)
    if inference and not n > d:
        return "--inference needs more rows than columns: the residual has n - d degrees of freedom (n = %d, d = %d)" % (n, d)
    if M and not M < d:
        return "--scan needs at least one covariate column: M = %d candidates of d = %d feature columns" % (M, d)
    if scan_se and not n > d - M + 1:
        return "--scan_se needs more rows than columns: the residual has n - (c + 1) degrees of freedom (n = %d, c = %d)" % (n, d - M)
    return None


def test_config_rules_on_both_sides_of_every_edge(lib):
    d, seen = 3, set()
    cases = []
    for K in (3, 4):                                                    # K = n, K = n + 1 at n = 3
        cases.append((3, base("lasso") + ["--l1=0.1,0.01", "--folds=%d" % K], dict(K=K)))
    for n in (d, d + 1):
        cases.append((n, base("cholesky") + ["--inference"], dict(inference=True)))
    for M in (d - 1, d):
        cases.append((6, base("cholesky") + ["--scan=%d" % M], dict(M=M)))
    for n in (3, 4):                                                    # M = 1: c = 2, n = c + 1 and c + 2
        cases.append((n, base("cholesky") + ["--scan=1", "--scan_se"], dict(M=1, scan_se=True)))
    for k in (d - 1, d, d + 1):
        for opt in ("--lower", "--upper", "--penalty_factors"):
            cases.append((6, base("lasso") + ["--l1=0.01", opt + "=" + ",".join(["0.5"] * k)], dict(box={opt: k})))
    # two broken at once: the order decides
    cases.append((2, base("lasso") + ["--l1=0.1,0.01", "--folds=3", "--upper=1,1"], dict(K=3, box={"--upper": 2})))
    cases.append((3, base("cholesky") + ["--scan=3", "--scan_se"], dict(M=3, scan_se=True)))
    cases.append((6, base("lasso") + ["--l1=0.01", "--penalty_factors=1,1", "--lower=0"], dict(box={"--lower": 1, "--penalty_factors": 2})))
    for n, args, kw in cases:
        r = Run(lib, args, (n, d, 5))
        want = config_rules(n, d, kw.get("box", {}), kw.get("K", 0), kw.get("inference", False), kw.get("M", 0), kw.get("scan_se", False))
        assert r.message == want, (n, args[6:])
        seen.add(want and want.split(":")[0].split(" wants")[0])
        r.close()
    assert seen == {None, "--lower", "--upper", "--penalty_factors", "--folds=4", "--inference needs more rows than columns",
                    "--scan needs at least one covariate column", "--scan_se needs more rows than columns"}


# ---- 3. the plan: the request of phase 2 and the job of phase 1, one command line per kind.  n = 10, d = 5, three providers
def plan_of(lib, args, shape=(10, 5, 5), device=0):
    r = Run(lib, args, shape, device)
    assert r.message is None, r.message
    return r


def system(p):
    s = p.sys
    return (s.d, s.width, s.precision, s.algorithm, s.num_iterations, s.lam, s.nshares, s.normalize, s.reveal_inputs, s.trace)


def job(p):
    j = p.job
    return (j.precision, j.precision_p2, j.w1, j.w2, j.device, j.mode.transport, j.mode.scan, j.mode.folds, j.want_yy)


def request(p):
    return (CREATE[p.create], p.n_lambdas, p.n_path, p.l1_mode, bool(p.lasso), p.folds, p.reveal, p.rule, p.infer, p.scan_M, p.scan_bits, p.resid_scale)


SOCKET_CHUNK, RING_CHUNK = 64 << 20, 64 << 30
LASSO_PATH, LASSO_CV = ["--l1=0.1,0.01"], ["--l1=0.1,0.01", "--folds=2"]
#        (algorithm, options)                                              kind        nl np mode  lasso  K  reveal rule infer M bits resid      system: d trace reveal_inputs   job: M K want_yy   output
PLANS = [
    (("cholesky", []),                                                    ("plain", 0, 0, ABSOLUTE, False, 0, 0, RULE_MIN, 0, 0, 0, 0.0),         (5, 1, 1), (0, 0, 0), "full"),
    (("ldlt", []),                                                        ("plain", 0, 0, ABSOLUTE, False, 0, 0, RULE_MIN, 0, 0, 0, 0.0),         (5, 1, 1), (0, 0, 0), "full"),
    (("cgd", []),                                                         ("plain", 0, 0, ABSOLUTE, False, 0, 0, RULE_MIN, 0, 0, 0, 0.0),         (5, 1, 1), (0, 0, 0), "full"),
    (("lasso", ["--l1=0.01"]),                                            ("lasso", 0, 0, ABSOLUTE, False, 0, 0, RULE_MIN, 0, 0, 0, 0.0),         (5, 0, 1), (0, 0, 0), "full"),
    (("lasso", LASSO_PATH),                                               ("lasso_path", 0, 2, ABSOLUTE, False, 0, 0, RULE_MIN, 0, 0, 0, 0.0),    (5, 0, 1), (0, 0, 0), "full"),
    (("lasso", ["--l1_ratios=1"]),                                        ("lasso_path", 0, 1, RATIO, False, 0, 0, RULE_MIN, 0, 0, 0, 0.0),       (5, 0, 1), (0, 0, 0), "full"),
    (("lasso", ["--l1=0.01", "--positive"]),                              ("lasso_opts", 0, 0, ABSOLUTE, True, 0, 0, RULE_MIN, 0, 0, 0, 0.0),     (5, 0, 1), (0, 0, 0), "full"),
    (("lasso", LASSO_PATH + ["--upper=1,1,1,1,1"]),                       ("lasso_opts", 0, 2, ABSOLUTE, True, 0, 0, RULE_MIN, 0, 0, 0, 0.0),     (5, 0, 1), (0, 0, 0), "full"),
    (("lasso", LASSO_CV),                                                 ("lasso_cv", 0, 2, ABSOLUTE, True, 2, 0, RULE_MIN, 0, 0, 0, 0.0),       (5, 0, 0), (0, 2, 0), "cv"),
    (("lasso", LASSO_CV + ["--reveal_index", "--positive"]),              ("lasso_cv", 0, 2, ABSOLUTE, True, 2, REVEAL_INDEX, RULE_MIN, 0, 0, 0, 0.0), (5, 0, 0), (0, 2, 0), "cv"),
    (("lasso", LASSO_CV + ["--one_se"]),                                  ("lasso_cv_se", 0, 2, ABSOLUTE, True, 2, 0, RULE_ONE_SE, 0, 0, 0, 0.0), (5, 0, 0), (0, 2, 1), "cv"),
    (("lasso", ["--l1_ratios=1,0.5,0.1", "--folds=4", "--reveal_curve", "--reveal_index"]),
                                                                          ("lasso_cv_se", 0, 3, RATIO, True, 4, REVEAL_INDEX | REVEAL_CURVE, RULE_MIN, 0, 0, 0, 0.0), (5, 0, 0), (0, 4, 1), "cv"),
    (("cholesky", ["--lambdas=0.1,0.01,0.001"]),                          ("sweep", 3, 0, ABSOLUTE, False, 0, 0, RULE_MIN, 0, 0, 0, 0.0),         (5, 0, 0), (0, 0, 0), "sweep"),
    (("cgd", ["--lambdas=0.1,0.01,0.001", "--table_ring", "--devices=0,1"]),
                                                                          ("sweep_blocks", 3, 0, ABSOLUTE, False, 0, 0, RULE_MIN, 0, 0, 0, 0.0),  (5, 0, 0), (0, 0, 0), "sweep"),
    (("cholesky", ["--lambdas=0.1,0.01", "--folds=2", "--reveal_index"]), ("ridge_cv", 2, 0, ABSOLUTE, False, 2, REVEAL_INDEX, RULE_MIN, 0, 0, 0, 0.0), (5, 0, 0), (0, 2, 0), "cv"),
    (("cholesky", ["--inference"]),                                       ("inference", 0, 0, ABSOLUTE, False, 0, 0, RULE_MIN, INFER_SE | INFER_FIT, 0, 0, 10 / 5), (5, 0, 0), (0, 0, 1), "full"),
    (("cholesky", ["--inference", "--no_se"]),                            ("inference", 0, 0, ABSOLUTE, False, 0, 0, RULE_MIN, INFER_FIT, 0, 0, 10 / 5), (5, 0, 0), (0, 0, 1), "full"),
    (("cholesky", ["--scan=2"]),                                          ("scan", 0, 0, ABSOLUTE, False, 0, 0, RULE_MIN, 0, 2, 0, 0.0),          (4, 0, 0), (2, 0, 1), "scan"),
    (("cholesky", ["--scan=2", "--scan_se"]),                             ("scan", 0, 0, ABSOLUTE, False, 0, 0, RULE_MIN, 0, 2, SCAN_SE, 10 / (10 - 4)), (4, 0, 0), (2, 0, 1), "scan"),
]


@pytest.mark.parametrize("line,req,sysm,jobm,output", PLANS, ids=["-".join([a] + [t.split("=")[0][2:] for t in o]) for (a, o), *_ in PLANS])
def test_plan_request_system_and_job(lib, line, req, sysm, jobm, output):
    alg, options = line
    r = plan_of(lib, base(alg) + options, device=3)
    p = r.plan
    assert request(p) == req
    algorithm = dict(cholesky=CHOLESKY, ldlt=LDLT, cgd=CGD, lasso=LASSO)[alg]
    # (width, precision and lambda from the line; the iteration count is read for cgd and lasso alone; one share per provider)
    assert system(p) == (sysm[0], 64, 20, algorithm, 10 if alg in ("cgd", "lasso") else 0, 0.001, 3, 1, sysm[2], sysm[1])
    assert job(p) == (20, 20, 64, 64, 3, TI_SOCKETS) + jobm
    assert (OUTPUT[p.output], p.n, p.d, p.providers, p.device) == (output, 10, 5, 3, 3)
    ring = "--table_ring" in options
    assert (p.table_chunk, p.n_blocks) == (RING_CHUNK if ring else SOCKET_CHUNK, 2 if ring else 0)
    if req[1]:
        assert p.lambdas[:req[1]] == [float(t) for t in options[0].split("=")[1].split(",")]
    if req[4]:                                                          # the lasso options: the path (or the one value), the lists, --positive's zeros
        l = p.lasso.contents
        values = [float(t) for t in options[0].split("=")[1].split(",")]
        assert (l.l1_count, l.l1[:l.l1_count], l.l1_mode) == (len(values), values, req[3])
        assert (l.lower[:5] if l.lower else None) == ([0.0] * 5 if "--positive" in options else None)
        assert (l.upper[:5] if l.upper else None) == ([1.0] * 5 if "--upper=1,1,1,1,1" in options else None)
        assert not l.penalty_factors
    r.close()


def test_plan_formats_transport_and_blocks(lib):
    r = plan_of(lib, base("cholesky") + ["--prec_phase2=40", "--width_phase1=32", "--use_ot"])
    assert job(r.plan) == (20, 40, 32, 64, 0, OT_PAIRS, 0, 0, 0) and (r.plan.sys.precision, r.plan.sys.width) == (40, 64)
    r.close()
    r = plan_of(lib, base("cholesky") + ["--width_phase2=32", "--prec_phase2=10"])
    assert job(r.plan)[:4] == (20, 10, 64, 32) and (r.plan.sys.precision, r.plan.sys.width) == (10, 32)
    r.close()
    # no empty blocks: four entries of --devices for three values are three blocks
    r = plan_of(lib, base("cholesky") + ["--lambdas=0.1,0.01,0.001", "--table_ring=4", "--devices=0,0,0,0"])
    assert (CREATE[r.plan.create], r.plan.n_blocks, r.opts.n_devices, r.plan.table_chunk) == ("sweep_blocks", 3, 4, RING_CHUNK)
    r.close()


# ---- 4. the share layout against the documented ones
def tri(i, j):
    return i * (i + 1) // 2 + j


def share_model(d, K, yy_words, M, A, b, yy):
    """include/linreg_gc_folds.h: K systems [A_k][b_k]; linreg_gc_lasso_cv_se.h / linreg_gc_inference.h: then the K (one) words yy;
    include/linreg_gc_scan.h: [A (T_c)] [b (c)] [yy] [h_0 (c)] .. [h_{M-1} (c)] [gg (M)] [gy (M)] out of the full triangle"""
    T = d * (d + 1) // 2
    if M:
        c = d - M
        out = [A[tri(i, j)] for i in range(c) for j in range(i + 1)] + b[:c] + [yy[0]]
        out += [A[tri(c + m, j)] for m in range(M) for j in range(c)]
        return out + [A[tri(c + m, c + m)] for m in range(M)] + [b[c + m] for m in range(M)]
    out = []
    for k in range(max(K, 1)):
        out += A[k * T:(k + 1) * T] + b[k * d:(k + 1) * d]
    return out + (yy[:max(K, 1)] if yy_words else [])


SHARES = [
    ("plain", 3, "cholesky", [], 0, False, 0),
    ("folds", 3, "lasso", ["--l1=0.1,0.01", "--folds=2"], 2, False, 0),
    ("folds-yy", 3, "lasso", ["--l1=0.1,0.01", "--folds=2", "--one_se"], 2, True, 0),
    ("inference", 3, "cholesky", ["--inference"], 0, True, 0),
    ("scan-M1", 4, "cholesky", ["--scan=1"], 0, True, 1),
    ("scan-M2", 4, "cholesky", ["--scan=2"], 0, True, 2),
    ("scan-M3", 4, "cholesky", ["--scan=3"], 0, True, 3),
]


@pytest.mark.parametrize("name,d,alg,options,K,yy_words,M", SHARES, ids=[s[0] for s in SHARES])
def test_share_words_follow_the_documented_layout(lib, name, d, alg, options, K, yy_words, M):
    r = plan_of(lib, base(alg) + options, (10, d, 5))
    T, systems = d * (d + 1) // 2, max(K, 1)
    A, b, yy = [1000 + i for i in range(systems * T)], [2000 + i for i in range(systems * d)], [3000 + i for i in range(systems)]
    want = share_model(d, K, yy_words, M, A, b, yy)
    assert len(set(want)) == len(want)                                  # distinct values: a wrong index cannot collide
    assert r.plan.share_words == len(want) and r.plan.job.want_yy == int(yy_words)
    cA, cb, cyy = (C.c_uint64 * len(A))(*A), (C.c_uint64 * len(b))(*b), (C.c_uint64 * len(yy))(*yy)
    got = [lib.run_share_word(C.byref(r.plan), cA, cb, cyy if yy_words else None, i) for i in range(len(want))]
    assert got == want
    r.close()


# ---- 5. the result layout, d = 3
def beta_words(d, n_lambdas, n_path, inference, M):
    """the old main()'s allocation of beta, in words"""
    return (n_lambdas if n_lambdas else n_path if n_path else 1) * d + 2 * n_path + 4 + (d + 2 if inference else 0) + 2 * M


CV = ["--l1=0.1,0.01", "--folds=2"]
#           algorithm   options                                              n_lambdas n_path inference M   output  results len   se    fit  index curve
RESULTS = [
    ("lasso", ["--l1=0.1,0.01"],                                             0, 2, False, 0, "full", 2, 3, NONE, NONE, NONE, NONE),
    ("lasso", CV,                                                            0, 2, False, 0, "cv", 1, 3, NONE, NONE, NONE, NONE),
    ("lasso", CV + ["--reveal_index"],                                       0, 2, False, 0, "cv", 1, 3, NONE, NONE, 3, NONE),
    ("lasso", CV + ["--one_se"],                                             0, 2, False, 0, "cv", 1, 3, NONE, NONE, NONE, NONE),
    ("lasso", CV + ["--reveal_curve"],                                       0, 2, False, 0, "cv", 1, 3, NONE, NONE, NONE, 3),
    ("lasso", CV + ["--reveal_index", "--reveal_curve"],                     0, 2, False, 0, "cv", 1, 3, NONE, NONE, 3, 4),
    ("lasso", CV + ["--reveal_index", "--one_se", "--reveal_curve"],         0, 2, False, 0, "cv", 1, 3, NONE, NONE, 3, 5),
    ("cholesky", ["--lambdas=1,2", "--folds=2", "--reveal_index"],           2, 0, False, 0, "cv", 1, 3, NONE, NONE, 3, NONE),
    ("cholesky", ["--inference"],                                            0, 0, True, 0, "full", 1, 3, 3, 6, NONE, NONE),
    ("cholesky", ["--inference", "--no_se"],                                 0, 0, True, 0, "full", 1, 3, NONE, 3, NONE, NONE),
    ("cholesky", ["--scan=2"],                                               0, 0, False, 2, "scan", 1, 2, NONE, NONE, NONE, NONE),
    ("cholesky", ["--scan=2", "--scan_se"],                                  0, 0, False, 2, "scan", 1, 2, 2, NONE, NONE, NONE),
    ("ldlt", ["--lambdas=1,2,3"],                                            3, 0, False, 0, "sweep", 3, 3, NONE, NONE, NONE, NONE),
    ("cgd", [],                                                              0, 0, False, 0, "full", 1, 3, NONE, NONE, NONE, NONE),
]


@pytest.mark.parametrize("case", RESULTS, ids=["-".join([c[0]] + [t.split("=")[0][2:] for t in c[1]]) for c in RESULTS])
def test_result_layout(lib, case):
    alg, options, n_lambdas, n_path, inference, M, output, results, length, se, fit, index, curve = case
    d = 3
    r = plan_of(lib, base(alg) + options, (10, d, 5))
    res = r.plan.result
    assert res.words == beta_words(d, n_lambdas, n_path, inference, M)
    assert (OUTPUT[r.plan.output], res.n_results, res.result_len, res.off_se, res.off_fit, res.off_index, res.off_curve) == (output, results, length, se, fit, index, curve)
    # everything the layout names lies inside the allocation
    ends = [res.n_results * d if output != "scan" else M]
    ends += [res.off_se + (M if M else d)] * (se != NONE) + [res.off_fit + 2] * (fit != NONE) + [res.off_curve + 2 * n_path] * (curve != NONE)
    ends += [res.off_index + (2 if "--one_se" in options else 1)] * (index != NONE)
    assert max(ends) <= res.words
    r.close()


# ---- 6. under the sanitizers, as a program of its own
def test_module_under_sanitizers(tmp_path):
    """host/linreg_run.c with the two pure modules it calls, compiled with ASan + UBSan into a program of its own; it runs on the
    lines that grow, reset and drop the lists (an option twice, a list that breaks off) and on one line per request kind, and says
    what the fixture says; the share is read out of buffers of exactly phase 1's sizes.  Nothing is loaded into python"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "asan_linreg_run")
    cc = subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", HOST,
                         os.path.join(ROOT, "tests", "tools", "asan_linreg_run.c")] + [os.path.join(HOST, f) for f in ("linreg_run.c", "phase1_plan.c", "sweep_plan.c")]
                        + ["-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "cannot find" in cc.stderr and "san" in cc.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert cc.returncode == 0, cc.stderr[-2000:]
    lines, said = corpus(), GOLDEN["messages"]
    lists = ("--lambdas", "--l1", "--l1_ratios", "--lower", "--upper", "--penalty_factors", "--devices")
    twice = [i for i, a in enumerate(lines) if a[3] == "lasso" and len(a) == 8 and all(t.split("=")[0] in lists for t in a[6:])]
    picked = twice[::max(1, len(twice) // 40)] + list(range(len(lines) - 40, len(lines)))
    assert len(picked) >= 60 and any(lines[i][6] == lines[i][7] for i in picked) and any(lines[i][-1] in ("--lambdas=x", "--l1=x", "--lower=x") for i in picked)

    def run(shape, args):
        out = subprocess.run([exe] + [str(v) for v in shape] + ["linreg"] + args, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.rstrip().endswith("all ok"), (args[6:], out.stdout[-500:], out.stderr[-3000:])
        return out.stdout.splitlines()[:-1]

    for i in picked:
        # (d = 2: the box lists of the corpus have two entries; a line the rules accept gets its plan built and freed)
        rows = run((10, 2, 5), lines[i])
        want = said[GOLDEN["index"][i]]
        if want == "accepted":                                          # (--scan=2 and more passes the rule book and has no covariate at d = 2)
            assert rows[0].startswith(("create ", "message: --scan needs at least one covariate column")), (lines[i][6:], rows[:1])
        else:
            assert rows[0] == "message: " + want, (lines[i][6:], rows[:1])
    for name, d, alg, options, K, yy_words, M in SHARES:
        rows = dict(row.split(" ", 1) for row in run((10, d, 5), base(alg) + options) if " " in row)
        T, systems = d * (d + 1) // 2, max(K, 1)
        A, b, yy = [1000 + i for i in range(systems * T)], [2000 + i for i in range(systems * d)], [3000 + i for i in range(systems)]
        assert [int(v) for v in rows["share"].split()] == share_model(d, K, yy_words, M, A, b, yy), name
    for (alg, options), req, sysm, jobm, output in PLANS:
        rows = dict(row.split(" ", 1) for row in run((10, 5, 5), base(alg) + options) if " " in row)
        assert (CREATE[int(rows["create"])], OUTPUT[int(rows["output"])], int(rows["sys_d"]), int(rows["want_yy"])) == (req[0], output, sysm[0], jobm[2])
        assert float(rows["resid_scale"]) == req[11]
