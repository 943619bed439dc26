/* linreg_run.h -- the pure-host description of one run of bin/linreg: what the command line said (run_opts), the rule book that
 * says which options go together, and what the options mean once n, d and the number of parties are known (run_plan): the
 * phase-2 system and which lgc_party_create* call builds it, phase 1's job, the words of a data provider's share and the layout
 * of the result the Evaluator reads back.  No GPU, no sockets, no globals, no OpenSSL: tests/test_linreg_run_cpu.py checks it
 * through libhosttest.so, tests/tools/asan_linreg_run.c runs it under the sanitizers. */
#ifndef LINREG_RUN_H
#define LINREG_RUN_H
#include <stddef.h>
#include <stdint.h>
#include "phase1_plan.h"
#include "../../include/linreg_gc.h"
#include "../../include/linreg_gc_lasso_opts.h"

enum { kMaxDevices = 16 };
typedef struct { double *v; size_t n; } run_list;       /* a comma-separated list of numbers; v is malloc'd */
enum { RUN_BOX_LOWER, RUN_BOX_UPPER, RUN_BOX_PENALTY };

/* ---------------------------------------------------------------- what the command line said, and nothing derived from it */
typedef struct {
    const char *input, *algorithm, *iterations;         /* argv[1], argv[4], argv[5] (read as a number only by cgd and lasso) */
    int precision, party, party_read;                   /* argv[2], argv[3]; party_read: the scan got as far as the party */
    double lambda;                                      /* argv[6] */
    p1_flags fl;                                        /* phase 1's switches; fl.scan / fl.folds: --scan / --folds was given */
    int w1, w2, prec_phase2;                            /* --width_phase1, --width_phase2 (64), --prec_phase2 (-1: as phase 1) */
    int ring_slots, table_lanes, input_ring;            /* --table_ring[=slots], --table_lanes=K, --input_ring */
    run_list lambdas;                                   /* --lambdas: the per-lambda sweep */
    run_list l1;                                        /* --l1 or --l1_ratios ... */
    int have_l1, have_ratios;                           /* ... and which of the two it was */
    int positive;                                       /* --positive, and the lists --lower, --upper, --penalty_factors */
    run_list box[3];
    long folds, scan;                                   /* --folds=K, --scan=M */
    int reveal_index, one_se, reveal_curve, inference, no_se, scan_se;
    int devices[kMaxDevices], n_devices;                /* --devices, as given */
    char *err;                                          /* the message the last failing call returned (run_opts_free) */
} run_opts;

extern const char run_usage[];                          /* the usage text; one %s: argv[0] */
/* argv into *o, with the checks a scan can make by itself: the positionals, "given twice", list syntax, the ratios' range, --l1
 * against --l1_ratios, the syntax of --scan, --folds and --devices.  Returns the first failing message as bin/linreg prints it
 * (owned by *o), or NULL.  *o is initialised here and is run_opts_free's afterwards, whatever was returned */
const char *run_opts_scan(run_opts *o, int argc, char **argv);
/* the rule book: which options go together, in the order bin/linreg has always said it (p1_mode_check among them).  Returns the
 * first failing message, or NULL */
const char *run_opts_check(run_opts *o);
void run_opts_free(run_opts *o);
/* --devices shards a sweep: no empty blocks, so at most one block per value of --lambdas; 0 without --devices */
int run_opts_blocks(const run_opts *o);

/* ---------------------------------------------------------------- what the options mean for n rows, d columns, P providers */
typedef enum {                                          /* the lgc_party_create* call of phase 2, in create's order of precedence */
    RUN_CREATE_SCAN, RUN_CREATE_INFERENCE, RUN_CREATE_RIDGE_CV, RUN_CREATE_SWEEP_BLOCKS, RUN_CREATE_SWEEP, RUN_CREATE_LASSO_CV_SE,
    RUN_CREATE_LASSO_CV, RUN_CREATE_LASSO_OPTS, RUN_CREATE_LASSO_PATH, RUN_CREATE_LASSO, RUN_CREATE_PLAIN
} run_create;
typedef enum { RUN_OUT_FULL, RUN_OUT_SWEEP, RUN_OUT_CV, RUN_OUT_SCAN } run_output;     /* what the Evaluator prints */
#define RUN_NO_OFFSET ((size_t)-1)
typedef struct {
    const run_opts *o;
    size_t n, d;
    int providers, device, n_blocks;                    /* n_blocks: run_opts_blocks */
    lgc_system sys;
    /* the phase-2 request: the call and its arguments beyond (device, &sys, role, seed, table_chunk) */
    run_create create;
    size_t n_lambdas; const double *lambdas;            /* sweep, sweep blocks, ridge cv */
    size_t n_path; int l1_mode;                         /* a lasso path: several --l1 values or --l1_ratios (LGC_L1_*); 0: none */
    const lgc_lasso_opts *lasso;                        /* opts, cv, cv_se: --positive, the box lists, the path; else NULL */
    size_t folds; int reveal, rule;                     /* cv, cv_se, ridge cv: K, LGC_SELECT_REVEAL_* bits, LGC_CV_RULE_* */
    int infer;                                          /* inference: LGC_INFER_* bits */
    size_t scan_M, scan_c; int scan_bits;               /* scan: candidates, covariates, LGC_SCAN_* bits */
    double resid_scale;                                 /* inference: n / (n - d); scan with --scan_se: n / (n - c - 1); else 0 */
    p1_job job;
    /* table bytes per launch: socket mode moves them through host buffers; ring mode keeps them in HBM (CSP and Evaluator on
     * one node), so launches are as large as the fused solver's: 2^25 gate steps = 64 GiB, i.e. a whole d = 500 matrix-vector
     * product is ONE launch (profiles/r5_timeline_d500_two_process.txt: 1.94 s at 16 GiB, 1.82 s at 64 GiB, co-located 1.81 s) */
    size_t table_chunk;
    size_t share_words;                                 /* words of one provider's share: run_share_word(.., i), i < share_words */
    /* the words lgc_party_finish writes to beta: n_results blocks of d coefficients (scan: one block of M), and behind them */
    struct {
        size_t words;                                   /* what to allocate */
        size_t n_results, result_len;
        size_t off_se;                                  /* inference without --no_se: d words u_j; --scan_se: M words w_m */
        size_t off_fit;                                 /* inference: s2, r2 */
        size_t off_index;                               /* --reveal_index: l+ (and with --one_se then l*), read through lgc_party_*_index */
        size_t off_curve;                               /* --reveal_curve: n_path means, then n_path standard errors */
    } result;                                           /* (an offset that the run does not have is RUN_NO_OFFSET) */
    run_output output;
    lgc_lasso_opts lasso_store; double *zeros;          /* what `lasso` points to; --positive's lower bounds */
    char *err;
} run_plan;
/* checks what needs the configuration, in bin/linreg's order (box-list lengths, K <= n, --inference's and --scan_se's rows,
 * M < d) and fills *p.  Returns the first failing message (owned by *p), or NULL.  *o must outlive *p; run_plan_free either way */
const char *run_plan_build(run_plan *p, const run_opts *o, size_t n, size_t d, int num_parties, int device);
void run_plan_free(run_plan *p);
/* word i of a provider's share, from what phase 1 returned (run_party): K systems [A_k][b_k] with --folds, else the one [A][b];
 * then the K (or one) words yy where job.want_yy; with --scan the layout of include/linreg_gc_scan.h, read out of the triangle */
uint64_t run_share_word(const run_plan *p, const uint64_t *A, const uint64_t *b, const uint64_t *yy, size_t i);
#endif
