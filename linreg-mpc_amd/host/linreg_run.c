/* linreg_run.c -- the pure-host description of one run of bin/linreg (linreg_run.h): the scan of the command line, the rule
 * book, and the plan of a run for a given configuration.  The order of the rules is part of the contract: it decides which
 * message a command line that breaks two of them gets (tests/golden/linreg_cli_rules.json pins it). */
#define _GNU_SOURCE
#include <errno.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "linreg_run.h"
#include "../../include/linreg_gc_lasso.h"
#include "../../include/linreg_gc_lasso_path.h"
#include "../../include/linreg_gc_folds.h"
#include "../../include/linreg_gc_lasso_cv.h"
#include "../../include/linreg_gc_lasso_cv_se.h"
#include "../../include/linreg_gc_ridge_cv.h"
#include "../../include/linreg_gc_inference.h"
#include "../../include/linreg_gc_scan.h"

/* sweep_plan.c */
int sweep_parse_devices(const char *text, int *devices, int max);

const char run_usage[] =
    "Usage: %s [Input_file] [Precision] [Party] [Algorithm] [Num. iterations CGD] [Lambda] [Options]\n"
    "Options: --use_ot: Enables the OT-based phase 1 protocol\n"
    "         --prec_phase2=<Precision phase 2>: Use different precision for phase 2 of the protocol\n"
    "         --width_phase1=<32|64>, --width_phase2=<32|64>: bit widths (default 64)\n"
    "         --table_ring[=slots]: parties 1 and 2 share one node; garbled tables stay in HBM (a byte ring of the largest\n"
    "                  launch plus slack; =slots: that many slots of the largest launch instead)\n"
    "         --table_lanes=<K>: garbled tables through the network over K extra TCP connections\n"
    "         --ti_ring: (TI mode) all parties on this node: the vectors of the multiplication protocol stay in HBM\n"
    "         --ti_matrix: (TI mode) one matrix triple per pair of data providers instead of one vector triple per pair of\n"
    "                  columns: a provider sends each peer its masked column block once (n (a + b) words between two providers\n"
    "                  with a and b columns, not n a b), the initializer seeds and a b words.  Same shares' sums; excludes\n"
    "                  --use_ot, --ot_ring, --ti_ring and --scan\n"
    "         --ot_matrix: (with --use_ot) one vector OT per bit of the receiving provider's words carries the correlations of\n"
    "                  all the sending provider's columns: between providers with r and s columns the OT extension shrinks by\n"
    "                  the factor s and y travels in words of the phase-1 width.  Same shares' sums; every provider must be\n"
    "                  started with it; excludes --ot_ring and --scan\n"
    "         --ot_half: (with --use_ot --ot_matrix) bit b of the product runs modulo 2^(W - b) and is shifted afterwards, so y\n"
    "                  carries W - b bits for it: 33/64 of --ot_matrix's bytes of y at width 64, 17/32 at 32.  Same OTs, same\n"
    "                  shares' sums; every provider must be started with it\n"
    "         --ot_ring: --use_ot with all data providers on this node: the OT extension's messages stay in HBM\n"
    "         --input_ring: (every party, all on this node) the messages of the label OT of phase 2 stay in HBM\n"
    "         --lambdas=l1,l2,...: regularisation sweep -- one circuit per value on the same shares (the data\n"
    "                  providers share their inputs once); [Lambda] is then ignored\n"
    "         --devices=g0,g1,...: (parties 1 and 2, with --lambdas and --table_ring) contiguous blocks of the sweep on\n"
    "                  these GPUs, one block per entry (an index may repeat); without it LINREG_DEVICE (default 0)\n"
    "         --l1=<value>: (Algorithm lasso, required there) the L1 penalty lambda1; [Lambda] is lambda2 and\n"
    "                  [Num. iterations CGD] the number of FISTA iterations.  --l1=v1,v2,...: a lasso path, one\n"
    "                  secure solve for every value (one L1 line and one Result line per value)\n"
    "         --l1_ratios=r1,r2,...: (Algorithm lasso, instead of --l1) a lasso path on ratios in [0, 2] of\n"
    "                  lambda_max = max_i |b_i|, which stays secret (one L1 ratio line and one Result line per ratio)\n"
    "         --positive: (Algorithm lasso) every coefficient >= 0; excludes --lower\n"
    "         --lower=v1,...,vd, --upper=v1,...,vd: (Algorithm lasso) per-coefficient bounds, d entries each; inf and\n"
    "                  -inf leave that side unbounded\n"
    "         --penalty_factors=w1,...,wd: (Algorithm lasso) coefficient i is penalised by w_i lambda1 (0: not at all)\n"
    "         --folds=K: (a lasso path) K-fold cross-validation inside the circuit, 2 <= K <= 16 contiguous row folds: phase 1\n"
    "                  runs once per fold, one Result line: the refit on all rows at the value with the least summed score\n"
    "           With cgd, cholesky or ldlt and --lambdas=l1,l2,...: the ridge sweep cross-validated the same way -- one Result\n"
    "           line, the refit on all rows at the value of lambda with the least cross-validated error\n"
    "         --reveal_index: (with --folds) also print which value of the path won\n"
    "         --one_se: (with --folds) the one-standard-error rule: the most regularised value whose cross-validated error is\n"
    "           within one standard error of the minimum (lambda.1se); with --reveal_index both indices are printed\n"
    "         --reveal_curve: (with --folds) also print the mean and the standard error of the folds' errors per value\n"
    "         --inference: (Algorithm cholesky) also print the standard errors of the coefficients, the residual variance\n"
    "                  (n - d degrees of freedom) and R^2, formed inside the circuit; --no_se: leave the standard errors out\n"
    "         --scan=M: (Algorithm cholesky) an association scan: the last M feature columns are candidates, each fitted with\n"
    "                  the first d - M columns (the shared covariates); one Result line with the M candidates' coefficients.\n"
    "                  --scan_se: also print their standard errors";

static const char *const box_opt[3] = {"--lower", "--upper", "--penalty_factors"};

static const char *fail(char **slot, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
static const char *fail(char **slot, const char *fmt, ...) {
    va_list ap;
    free(*slot);
    va_start(ap, fmt);
    if (vasprintf(slot, fmt, ap) < 0) *slot = NULL;
    va_end(ap);
    return *slot ? *slot : "out of memory";
}
#define rule(cond, ...) do { if (!(cond)) return fail(err, __VA_ARGS__); } while (0)

static int is_algorithm(const run_opts *o, const char *name) { return !strcmp(o->algorithm, name); }

/* a list "v1,v2,..." behind *l (strtod reads inf and -inf).  0, or 1: not a list of numbers, or 2: with `ratios`, *bad lies
 * outside [0, 2].  Value by value, so that the first offence of either kind is the one reported */
static int list_append(run_list *l, const char *q, int ratios, double *bad) {
    while (1) {
        char *e2;
        errno = 0;
        double v = strtod(q, &e2);
        if (!(!errno && e2 != q && (*e2 == ',' || !*e2))) return 1;
        if (ratios && !(v >= 0 && v <= 2)) { *bad = v; return 2; }
        l->v = realloc(l->v, (l->n + 1) * sizeof *l->v);
        l->v[l->n++] = v;
        if (!*e2) return 0;
        q = e2 + 1;
    }
}

const char *run_opts_scan(run_opts *o, int argc, char **argv) {
    memset(o, 0, sizeof *o);
    o->prec_phase2 = -1; o->w1 = o->w2 = 64;
    char **err = &o->err;
    rule(argc > 6, run_usage, argv[0]);
    char *end;
    errno = 0;
    o->input = argv[1];
    o->precision = (int)strtol(argv[2], &end, 10);
    rule(!errno, "strtol: %s", strerror(errno));
    rule(!*end, "Precision must be a number");
    o->party = (int)strtol(argv[3], &end, 10);
    rule(!errno, "strtol: %s", strerror(errno));
    rule(!*end, "Party must be a number");
    o->party_read = 1;
    o->algorithm = argv[4];
    rule(is_algorithm(o, "cholesky") || is_algorithm(o, "ldlt") || is_algorithm(o, "cgd") || is_algorithm(o, "lasso"),
         "Algorithm must be cholesky, ldlt, cgd, or lasso.");
    o->iterations = argv[5];
    o->lambda = strtod(argv[6], &end);
    rule(!errno, "strtod: %s", strerror(errno));
    rule(!*end, "lambda must be a number");

    for (int i = 7; i < argc; i++) {
        if (!strcmp(argv[i], "--use_ot")) o->fl.use_ot = 1;
        else if (!strcmp(argv[i], "--ot_ring")) o->fl.ot_ring = 1;            /* --use_ot with u / y of the extension in device rings */
        else if (!strcmp(argv[i], "--input_ring")) o->input_ring = 1;         /* all parties on this node: the label OT's messages stay in HBM */
        else if (!strcmp(argv[i], "--ti_ring")) o->fl.ti_ring = 1;            /* TI mode, all parties on this node: vectors stay in HBM */
        else if (!strcmp(argv[i], "--ti_matrix")) o->fl.ti_matrix = 1;        /* TI mode, one matrix triple per provider pair */
        else if (!strcmp(argv[i], "--ot_matrix")) o->fl.ot_matrix = 1;        /* OT mode, one vector OT per operand bit */
        else if (!strcmp(argv[i], "--ot_half")) o->fl.ot_half = 1;            /* that mode with W - bit bits of y per bit */
        else if (!strncmp(argv[i], "--lambdas=", 10)) {                       /* (lambda enters at linear.oc:52-57) */
            const char *q = argv[i] + 10;
            while (*q) {
                char *e2;
                double v = strtod(q, &e2);
                rule(e2 != q && (*e2 == ',' || !*e2), "--lambdas wants a comma-separated list of numbers");
                o->lambdas.v = realloc(o->lambdas.v, (o->lambdas.n + 1) * sizeof *o->lambdas.v);
                o->lambdas.v[o->lambdas.n++] = v;
                q = *e2 ? e2 + 1 : e2;
            }
            rule(o->lambdas.n > 0, "--lambdas wants at least one value");
        }
        else if (!strncmp(argv[i], "--l1=", 5) || !strncmp(argv[i], "--l1_ratios=", 12)) {
            const int ratios = argv[i][4] == '_';
            const char *opt = ratios ? "--l1_ratios" : "--l1";
            double bad = 0;
            rule(!(ratios ? o->have_ratios : o->have_l1), "%s is given twice", opt);
            o->l1.n = 0;
            const int r = list_append(&o->l1, argv[i] + (ratios ? 12 : 5), ratios, &bad);
            rule(r != 1, "%s wants a comma-separated list of numbers", opt);
            rule(r != 2, "--l1_ratios: every ratio must lie in [0, 2] (got %g)", bad);
            if (ratios) o->have_ratios = 1;
            else o->have_l1 = 1;
            rule(!(o->have_l1 && o->have_ratios), "--l1 and --l1_ratios exclude each other");
        }
        else if (!strcmp(argv[i], "--positive")) o->positive = 1;
        else if (!strcmp(argv[i], "--reveal_index")) o->reveal_index = 1;
        else if (!strcmp(argv[i], "--one_se")) o->one_se = 1;
        else if (!strcmp(argv[i], "--reveal_curve")) o->reveal_curve = 1;
        else if (!strcmp(argv[i], "--inference")) o->inference = 1;
        else if (!strcmp(argv[i], "--no_se")) o->no_se = 1;
        else if (!strcmp(argv[i], "--scan_se")) o->scan_se = 1;
        else if (!strncmp(argv[i], "--scan=", 7)) {
            char *e2;
            rule(!o->fl.scan, "--scan is given twice");
            errno = 0;
            o->scan = strtol(argv[i] + 7, &e2, 10);
            rule(!errno && e2 != argv[i] + 7 && !*e2 && o->scan >= 1, "--scan wants a candidate count >= 1");
            o->fl.scan = 1;
        }
        else if (!strncmp(argv[i], "--folds=", 8)) {
            char *e2;
            rule(!o->fl.folds, "--folds is given twice");
            errno = 0;
            o->folds = strtol(argv[i] + 8, &e2, 10);
            rule(!errno && e2 != argv[i] + 8 && !*e2, "--folds wants a number");
            o->fl.folds = 1;
        }
        else if (!strncmp(argv[i], "--lower=", 8) || !strncmp(argv[i], "--upper=", 8) || !strncmp(argv[i], "--penalty_factors=", 18)) {
            const int k = argv[i][2] == 'l' ? RUN_BOX_LOWER : argv[i][2] == 'u' ? RUN_BOX_UPPER : RUN_BOX_PENALTY;
            rule(!o->box[k].v, "%s is given twice", box_opt[k]);
            rule(!list_append(&o->box[k], strchr(argv[i], '=') + 1, 0, NULL), "%s wants a comma-separated list of numbers", box_opt[k]);
        }
        else if (!strncmp(argv[i], "--devices=", 10)) {
            o->n_devices = sweep_parse_devices(argv[i] + 10, o->devices, kMaxDevices);
            rule(o->n_devices > 0, "--devices wants a comma-separated list of at most %d device indices", kMaxDevices);
        }
        else if (!strcmp(argv[i], "--table_ring")) o->ring_slots = 65;       /* TABLE_RING_BYTES (protocol.h): the byte ring */
        else if (sscanf(argv[i], "--table_ring=%i", &o->ring_slots) == 1) {}
        else if (sscanf(argv[i], "--table_lanes=%i", &o->table_lanes) == 1) {}
        else if (sscanf(argv[i], "--width_phase1=%i", &o->w1) == 1) {}
        else if (sscanf(argv[i], "--width_phase2=%i", &o->w2) == 1) {}
        else if (sscanf(argv[i], "--prec_phase2=%i", &o->prec_phase2) != 1) o->prec_phase2 = -1;
    }
    return NULL;
}

const char *run_opts_check(run_opts *o) {
    char **err = &o->err;
    const int is_lasso = is_algorithm(o, "lasso"), have_folds = o->fl.folds, have_scan = o->fl.scan;
    const size_t n_lambdas = o->lambdas.n;
    rule((o->w1 == 32 || o->w1 == 64) && (o->w2 == 32 || o->w2 == 64), "Bit widths must be 32 or 64");
    rule(o->precision >= 0, "Precision of phase 1 must be nonnegative");
    rule(o->prec_phase2 >= -1, "Precision of phase 2 must be nonnegative");
    rule(o->precision < o->w1, "Precision of phase 1 must be smaller than bit size of phase 1");
    rule(o->prec_phase2 < o->w2, "Precision of phase 2 must be smaller than bit size of phase 2");
    /* which of phase 1's switches go together: the one rule book (phase1_plan.h) */
    rule(!p1_mode_check(&o->fl), "%s", p1_mode_check(&o->fl));
    rule(!is_lasso || o->have_l1 || o->have_ratios, "Algorithm lasso needs --l1=<value> (or --l1=v1,v2,... or --l1_ratios=r1,r2,...)");
    rule(is_lasso || !o->have_l1, "--l1 is for Algorithm lasso");
    rule(is_lasso || !o->have_ratios, "--l1_ratios is for Algorithm lasso");
    rule(is_lasso || !o->positive, "--positive is for Algorithm lasso");
    for (int k = 0; k < 3; k++) rule(is_lasso || !o->box[k].v, "%s is for Algorithm lasso", box_opt[k]);
    rule(!(o->positive && o->box[RUN_BOX_LOWER].v), "--positive and --lower exclude each other (--positive is --lower=0,...,0)");
    /* a path: several --l1 values, or any --l1_ratios; one --l1 value is the single solve */
    const size_t n_path = o->have_ratios || o->l1.n > 1 ? o->l1.n : 0;
    rule(n_path <= LGC_MAX_L1_PATH, "a lasso path takes at most %d values", LGC_MAX_L1_PATH);
    /* --folds: the path cross-validated over K row folds (include/linreg_gc_folds.h, include/linreg_gc_lasso_cv.h) */
    /* ... or, for cgd / cholesky / ldlt with --lambdas, the ridge sweep (include/linreg_gc_ridge_cv.h) */
    const int ridge_cv = have_folds && !is_lasso && n_lambdas > 0;
    rule(is_lasso || !have_folds || ridge_cv, "--folds is for Algorithm lasso");
    rule(have_folds || !o->reveal_index, "--reveal_index belongs to --folds");
    rule(have_folds || !o->one_se, "--one_se belongs to --folds");
    rule(have_folds || !o->reveal_curve, "--reveal_curve belongs to --folds");
    if (have_folds) {
        rule(o->folds >= 2 && o->folds <= LGC_MAX_FOLDS, "--folds wants 2..%d folds (got %ld)", LGC_MAX_FOLDS, o->folds);
        rule(ridge_cv || n_path > 0, "--folds selects among the values of a lasso path: it needs --l1_ratios or several --l1 values");
        rule(ridge_cv || !n_lambdas, "--folds and --lambdas exclude each other");
        rule(!ridge_cv || n_lambdas <= LGC_MAX_RIDGE_CV_VALUES, "--folds cross-validates at most %d values of --lambdas (got %zu)", LGC_MAX_RIDGE_CV_VALUES, n_lambdas);
        rule(!ridge_cv || (!o->one_se && !o->reveal_curve), "--one_se and --reveal_curve are for the cross-validation of a lasso path");
        rule(!o->n_devices, "--folds and --devices exclude each other");
        rule(!o->fl.ti_ring, "--folds and --ti_ring exclude each other");
        rule(!o->fl.ot_ring, "--folds and --ot_ring exclude each other");
        rule(!o->input_ring, "--folds and --input_ring exclude each other");
    }
    /* --inference: standard errors, residual variance and R^2 from the Cholesky solve (include/linreg_gc_inference.h) */
    rule(o->inference || !o->no_se, "--no_se belongs to --inference");
    if (o->inference) {
        rule(is_algorithm(o, "cholesky"), "--inference is for Algorithm cholesky");
        rule(!have_folds, "--inference and --folds exclude each other");
        rule(!n_lambdas, "--inference and --lambdas exclude each other");
        rule(!o->n_devices, "--inference and --devices exclude each other");
        rule(!o->fl.ti_ring, "--inference and --ti_ring exclude each other");
        rule(!o->fl.ot_ring, "--inference and --ot_ring exclude each other");
        rule(!o->input_ring, "--inference and --input_ring exclude each other");
    }
    /* --scan: M candidate columns against the shared covariates in one solve (include/linreg_gc_scan.h) */
    rule(have_scan || !o->scan_se, "--scan_se belongs to --scan");
    if (have_scan) {
        rule(is_algorithm(o, "cholesky"), "--scan is for Algorithm cholesky");
        rule(!n_lambdas, "--scan and --lambdas exclude each other");
        rule(!have_folds, "--scan and --folds exclude each other");
        rule(!o->inference, "--scan and --inference exclude each other");
        rule(!o->n_devices, "--scan and --devices exclude each other");
        rule(!o->fl.ti_ring, "--scan and --ti_ring exclude each other");
        rule(!o->fl.ot_ring, "--scan and --ot_ring exclude each other");
        rule(!o->input_ring, "--scan and --input_ring exclude each other");
        rule((unsigned long)o->scan <= LGC_MAX_SCAN, "--scan takes at most %u candidate columns", (unsigned)LGC_MAX_SCAN);
    }
    if (o->n_devices)
        rule(n_lambdas > 0 && o->ring_slots > 0, "--devices shards a --lambdas sweep and needs --table_ring (CSP and Evaluator on this node)");
    return NULL;
}

int run_opts_blocks(const run_opts *o) {
    return (size_t)o->n_devices > o->lambdas.n ? (int)o->lambdas.n : o->n_devices;
}

void run_opts_free(run_opts *o) {
    free(o->lambdas.v);
    free(o->l1.v);
    for (int k = 0; k < 3; k++) free(o->box[k].v);
    free(o->err);
    memset(o, 0, sizeof *o);
}

/* ---------------------------------------------------------------------------------------------------------------- the plan */
const char *run_plan_build(run_plan *p, const run_opts *o, size_t n, size_t d, int num_parties, int device) {
    memset(p, 0, sizeof *p);
    char **err = &p->err;
    const int have_folds = o->fl.folds, have_scan = o->fl.scan, is_lasso = is_algorithm(o, "lasso");
    const size_t K = have_folds ? (size_t)o->folds : 0;
    for (int k = 0; k < 3; k++)                 /* (before any connection: d comes from the configuration) */
        rule(!o->box[k].v || o->box[k].n == d, "%s wants d = %zu entries (got %zu)", box_opt[k], d, o->box[k].n);
    rule(K <= n, "--folds=%zu: more folds than the %zu rows of the input", K, n);
    rule(!o->inference || n > d, "--inference needs more rows than columns: the residual has n - d degrees of freedom (n = %zu, d = %zu)", n, d);
    rule(!have_scan || (size_t)o->scan < d, "--scan needs at least one covariate column: M = %ld candidates of d = %zu feature columns", o->scan, d);
    rule(!o->scan_se || n > d - (size_t)o->scan + 1, "--scan_se needs more rows than columns: the residual has n - (c + 1) degrees of freedom (n = %zu, c = %zu)",
         n, d - (size_t)o->scan);

    p->o = o; p->n = n; p->d = d; p->providers = num_parties - 2; p->device = device; p->n_blocks = run_opts_blocks(o);
    p->n_lambdas = o->lambdas.n; p->lambdas = o->lambdas.v;
    p->n_path = o->have_ratios || o->l1.n > 1 ? o->l1.n : 0;
    p->l1_mode = o->have_ratios ? LGC_L1_RATIO : LGC_L1_ABSOLUTE;
    p->folds = K;
    p->scan_M = have_scan ? (size_t)o->scan : 0; p->scan_c = have_scan ? d - p->scan_M : 0;
    const int precision2 = o->prec_phase2 != -1 ? o->prec_phase2 : o->precision;
    const int cv_se = o->one_se || o->reveal_curve;
    p->job = (p1_job){o->precision, precision2, o->w1, o->w2, device, {p1_transport_of(&o->fl), p->scan_M, K},
                      cv_se || o->inference || have_scan};      /* (want_yy: the calls that take K more words, or one, per share) */

    /* the phase-2 system: known from the configuration before any protocol message */
    lgc_system *sys = &p->sys;
    sys->d = d; sys->width = o->w2; sys->precision = precision2;
    sys->algorithm = is_algorithm(o, "cholesky") ? LGC_ALG_CHOLESKY : is_algorithm(o, "ldlt") ? LGC_ALG_LDLT : is_lasso ? LGC_ALG_LASSO : LGC_ALG_CGD;
    sys->num_iterations = is_algorithm(o, "cgd") || is_lasso ? atoi(o->iterations) : 0;
    sys->lambda = o->lambda; sys->nshares = (size_t)p->providers;
    sys->normalize = 1; sys->reveal_inputs = 1; sys->trace = !is_lasso;    /* (lasso prints what cholesky / ldlt print: no per-iteration rows) */
    if (p->n_lambdas) { sys->reveal_inputs = 0; sys->trace = 0; }    /* merged program of n_lambdas circuits: results only */
    if (K) sys->reveal_inputs = 0;                                   /* a cross-validation reveals the refit (and l*), never its K fold systems */
    if (o->inference) sys->trace = sys->reveal_inputs = 0;           /* Y = y^T y / (n d) stays a garbled word, and with it A and b */
    if (have_scan) { sys->d = p->scan_c + 1; sys->trace = sys->reveal_inputs = 0; }   /* each fitted system: the covariates and one candidate */
    p->table_chunk = o->ring_slots > 0 ? (size_t)64 << 30 : (size_t)64 << 20;

    /* which call creates the phase-2 object, and what it is told */
    const int boxed = o->positive || o->box[0].v || o->box[1].v || o->box[2].v;
    p->create = have_scan ? RUN_CREATE_SCAN : o->inference ? RUN_CREATE_INFERENCE
              : p->n_lambdas && K ? RUN_CREATE_RIDGE_CV             /* --lambdas with --folds: the ridge sweep cross-validated in-circuit */
              : p->n_blocks ? RUN_CREATE_SWEEP_BLOCKS : p->n_lambdas ? RUN_CREATE_SWEEP
              : K && cv_se ? RUN_CREATE_LASSO_CV_SE : K ? RUN_CREATE_LASSO_CV : boxed ? RUN_CREATE_LASSO_OPTS
              : p->n_path ? RUN_CREATE_LASSO_PATH : is_lasso ? RUN_CREATE_LASSO : RUN_CREATE_PLAIN;
    if (p->create == RUN_CREATE_LASSO_CV_SE || p->create == RUN_CREATE_LASSO_CV || p->create == RUN_CREATE_LASSO_OPTS) {
        lgc_lasso_opts *l = &p->lasso_store;
        if (o->positive) {
            p->zeros = calloc(d ? d : 1, sizeof *p->zeros);
            rule(p->zeros != NULL, "out of memory");
        }
        l->l1_count = p->n_path ? p->n_path : 1;
        l->l1 = o->l1.v;
        l->l1_mode = p->l1_mode;
        l->lower = o->positive ? p->zeros : o->box[RUN_BOX_LOWER].v; l->upper = o->box[RUN_BOX_UPPER].v; l->penalty_factors = o->box[RUN_BOX_PENALTY].v;
        p->lasso = l;
    }
    p->reveal = (o->reveal_index ? LGC_SELECT_REVEAL_INDEX : 0) | (o->reveal_curve ? LGC_SELECT_REVEAL_CURVE : 0);
    p->rule = o->one_se ? LGC_CV_RULE_ONE_SE : LGC_CV_RULE_MIN;
    p->infer = o->inference ? (o->no_se ? 0 : LGC_INFER_SE) | LGC_INFER_FIT : 0;
    p->scan_bits = o->scan_se ? LGC_SCAN_SE : 0;
    p->resid_scale = o->scan_se ? (double)n / (double)(n - (p->scan_c + 1)) : o->inference ? (double)n / (double)(n - d) : 0;

    /* a share: [A (T)] [b (d)] per system and then the words yy, or the scan's layout (run_share_word) */
    const size_t T = d * (d + 1) / 2, systems = K ? K : 1;
    p->share_words = have_scan ? p->scan_c * (p->scan_c + 1) / 2 + p->scan_c + 1 + p->scan_M * p->scan_c + 2 * p->scan_M
                               : systems * (T + d) + (p->job.want_yy ? systems : 0);

    /* what the Evaluator prints, and where lgc_party_finish leaves it */
    p->output = p->n_lambdas && !K ? RUN_OUT_SWEEP : K ? RUN_OUT_CV : have_scan ? RUN_OUT_SCAN : RUN_OUT_FULL;
    p->result.n_results = p->output == RUN_OUT_SWEEP ? p->n_lambdas : p->output == RUN_OUT_FULL && p->n_path ? p->n_path : 1;
    p->result.result_len = have_scan ? p->scan_M : d;
    p->result.words = (p->n_lambdas ? p->n_lambdas : p->n_path ? p->n_path : 1) * d + 2 * p->n_path + 4 + (o->inference ? d + 2 : 0) + 2 * p->scan_M;
    p->result.off_se = o->scan_se ? p->scan_M : o->inference && !o->no_se ? d : RUN_NO_OFFSET;
    p->result.off_fit = o->inference ? d + (o->no_se ? 0 : d) : RUN_NO_OFFSET;
    p->result.off_index = K && o->reveal_index ? d : RUN_NO_OFFSET;
    p->result.off_curve = K && o->reveal_curve ? d + (o->reveal_index ? (o->one_se ? 2 : 1) : 0) : RUN_NO_OFFSET;
    return NULL;
}

void run_plan_free(run_plan *p) {
    free(p->zeros);
    free(p->err);
    memset(p, 0, sizeof *p);
}

static size_t tri(size_t i, size_t j) { return i * (i + 1) / 2 + j; }        /* entry (i, j), j <= i, of a packed lower triangle */

uint64_t run_share_word(const run_plan *p, const uint64_t *A, const uint64_t *b, const uint64_t *yy, size_t i) {
    const size_t d = p->d, T = d * (d + 1) / 2;
    if (p->scan_M) {
        /* [A (T_c)] [b (c)] [yy] [h_0 (c)] .. [h_{M-1} (c)] [gg (M)] [gy (M)] (linreg_gc_scan.h), read out of the triangle phase 1
         * filled: the rows of the candidates against the covariates, their diagonals, their entries of b */
        const size_t c = p->scan_c, M = p->scan_M, sT = c * (c + 1) / 2, sH = sT + c + 1, sGG = sH + M * c, sGY = sGG + M;
        if (i < sT) return A[i];
        if (i < sT + c) return b[i - sT];
        if (i == sT + c) return yy[0];
        if (i < sGG) return A[tri(c + (i - sH) / c, (i - sH) % c)];
        if (i < sGY) return A[tri(c + i - sGG, c + i - sGG)];
        return b[c + i - sGY];
    }
    /* K share systems [A_0][b_0] ... [A_{K-1}][b_{K-1}] with --folds (linreg_gc_lasso_cv.h), else the one [A][b]; then the K
     * words yy_k with --one_se / --reveal_curve (linreg_gc_lasso_cv_se.h): zeros but for the provider that holds y; or the one
     * word yy with --inference (linreg_gc_inference.h) */
    const size_t per = T + d, nsys = (p->folds ? p->folds : 1) * per;
    if (i >= nsys) return yy[i - nsys];
    return i % per < T ? A[i / per * T + i % per] : b[i / per * d + i % per - T];
}
