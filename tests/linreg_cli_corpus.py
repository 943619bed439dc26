"""The command lines that pin bin/linreg's rule book: a deterministic corpus for party 3 with an input path that does not exist,
so that a line the rules accept ends at "Could not read config".  Imported by tests/golden/gen_linreg_cli_rules.py, which records
what the binary of the parent commit says to each line, and by tests/test_linreg_run_cpu.py, which asks host/linreg_run.c.

Every line is the argument vector behind the program's name."""
import itertools

ALGORITHMS = ("cholesky", "ldlt", "cgd", "lasso")
INPUT = "/nonexistent/linreg_cli_corpus.in"

# each option once in a valid form, then the malformed forms
TOKENS = (
    "--use_ot", "--ot_ring", "--ti_ring", "--ti_matrix", "--ot_matrix", "--ot_half", "--input_ring",
    "--table_ring", "--table_ring=4", "--table_lanes=2", "--width_phase1=32", "--width_phase2=32", "--prec_phase2=40",
    "--lambdas=0.1,0.01", "--l1=0.01", "--l1=0.1,0.01", "--l1_ratios=1,0.5",
    "--positive", "--lower=0,0", "--upper=1,inf", "--penalty_factors=1,0",
    "--folds=2", "--reveal_index", "--one_se", "--reveal_curve", "--inference", "--no_se", "--scan=2", "--scan_se", "--devices=0,0",
    "--folds=x", "--folds=1", "--scan=0", "--l1_ratios=3", "--l1=x", "--lambdas=", "--lambdas=x", "--lower=x", "--devices=x",
    "--width_phase2=48", "--prec_phase2=-2",
)


def base(algorithm, precision="20", party="3", iterations="10", lam="0.001"):
    return [INPUT, precision, party, algorithm, iterations, lam]


def many(n):
    return ",".join("0.%03d" % (i + 1) for i in range(n))


def corpus():
    lines = []
    for alg in ALGORITHMS:
        lines += [base(alg) + [t] for t in TOKENS]
        lines += [base(alg) + [s, t] for s, t in itertools.product(TOKENS, repeat=2)]
    # the positionals: too few arguments; not numbers; out of a long's / a double's range; an unknown algorithm; the precisions
    # against the widths
    lines += [
        [INPUT, "20", "3", "cholesky", "10"],
        base("cholesky", precision="2x"), base("cholesky", party="three"), base("cholesky", lam="0.1l"),
        base("cholesky", precision="99999999999999999999"), base("cholesky", party="99999999999999999999"), base("cholesky", lam="1e999"),
        base("qr"), base("cholesky", precision="-1"), base("cholesky", precision="64"), base("cholesky", precision="40") + ["--width_phase1=32"],
        base("cholesky", precision="56") + ["--width_phase2=32"],
    ]
    # rules that only three options reach: what --folds excludes once it is a cross-validation, on both kinds of it; the limits
    ridge, path = base("cholesky") + ["--lambdas=0.1,0.01", "--folds=2"], base("lasso") + ["--l1=0.1,0.01", "--folds=2"]
    for more in ("--one_se", "--reveal_curve", "--devices=0,0", "--ti_ring", "--ot_ring", "--input_ring", "--inference", "--scan=2",
                 "--reveal_index", "--table_ring"):
        lines += [ridge + [more], path + [more]]
    lines += [
        path + ["--lambdas=0.1"], path + ["--one_se", "--reveal_curve", "--reveal_index"],
        base("lasso") + ["--l1=" + many(256)], base("lasso") + ["--l1=" + many(257)], base("lasso") + ["--l1_ratios=" + many(257)],
        base("cholesky") + ["--lambdas=" + many(256), "--folds=2"], base("cholesky") + ["--lambdas=" + many(257), "--folds=2"],
        base("cholesky") + ["--scan=1048576"], base("cholesky") + ["--scan=1048577"], base("cholesky") + ["--folds=17", "--lambdas=0.1"],
        base("cholesky") + ["--lambdas=0.1,0.01,0.001", "--table_ring", "--devices=0,0,0,0"],
        base("cholesky") + ["--devices=" + ",".join(["0"] * 17)], base("cholesky") + ["--unknown_option"],
        base("cholesky") + ["--prec_phase2=30", "--unknown_option"],
        base("cholesky") + ["--use_ot", "--ot_matrix", "--scan=2"], base("lasso") + ["--l1=0.01", "--positive", "--lower=0,0"],
    ]
    return lines
