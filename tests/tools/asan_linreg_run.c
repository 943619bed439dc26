/* The pure-host description of a run of bin/linreg (host/linreg_run.c) as a program of its own, for the sanitizers:
 *     asan_linreg_run n d num_parties linreg [Input_file] [Precision] ... [Options]
 * scans and checks the command line behind the three numbers as bin/linreg does and builds the plan for n rows, d columns and
 * num_parties parties (CSP and Evaluator included).  Prints "message: <text>" for the first rule the line breaks, else the plan,
 * one "name value" per line, and every word of a share whose A, b and yy are filled with 1000 + i, 2000 + i, 3000 + i; frees
 * everything; exit status 0 either way.
 *   gcc -fsanitize=address,undefined -I linreg-mpc_amd/host tests/tools/asan_linreg_run.c linreg-mpc_amd/host/linreg_run.c \
 *       linreg-mpc_amd/host/phase1_plan.c linreg-mpc_amd/host/sweep_plan.c */
#include <stdio.h>
#include <stdlib.h>
#include <sys/types.h>
#include "linreg_run.h"

int main(int argc, char **argv) {
    if (argc < 5) { fprintf(stderr, "usage: %s n d num_parties linreg [arguments of bin/linreg]\n", argv[0]); return 2; }
    const size_t n = (size_t)strtoull(argv[1], NULL, 10), d = (size_t)strtoull(argv[2], NULL, 10);
    const int parties = atoi(argv[3]);
    run_opts o;
    run_plan p;
    int planned = 0;
    const char *msg = run_opts_scan(&o, argc - 4, argv + 4);
    if (!msg) msg = run_opts_check(&o);
    if (!msg) { msg = run_plan_build(&p, &o, n, d, parties, 0); planned = 1; }
    if (msg) printf("message: %s\n", msg);
    else {
        printf("create %d\noutput %d\nsys_d %zu\ntrace %d\nreveal_inputs %d\nnum_iterations %d\n", (int)p.create, (int)p.output, p.sys.d, p.sys.trace,
               p.sys.reveal_inputs, p.sys.num_iterations);
        printf("n_blocks %d\nn_lambdas %zu\nn_path %zu\nl1_mode %d\nfolds %zu\nreveal %d\nrule %d\ninfer %d\nscan_M %zu\nscan_bits %d\nresid_scale %.17g\n",
               p.n_blocks, p.n_lambdas, p.n_path, p.l1_mode, p.folds, p.reveal, p.rule, p.infer, p.scan_M, p.scan_bits, p.resid_scale);
        printf("transport %d\nwant_yy %d\ntable_chunk %zu\nshare_words %zu\n", (int)p.job.mode.transport, p.job.want_yy, p.table_chunk, p.share_words);
        printf("result_words %zu\nn_results %zu\nresult_len %zu\noff_se %zd\noff_fit %zd\noff_index %zd\noff_curve %zd\n", p.result.words, p.result.n_results,
               p.result.result_len, (ssize_t)p.result.off_se, (ssize_t)p.result.off_fit, (ssize_t)p.result.off_index, (ssize_t)p.result.off_curve);
        if (p.lasso) {
            printf("lasso_l1");
            for (size_t i = 0; i < p.lasso->l1_count; i++) printf(" %.17g", p.lasso->l1[i]);
            printf("\nlasso_lower");
            for (size_t i = 0; p.lasso->lower && i < d; i++) printf(" %.17g", p.lasso->lower[i]);
            printf("\n");
        }
        /* the share, from buffers of exactly the sizes phase 1 returns: an index that leaves them is an overrun the run reports */
        const size_t K = p.folds ? p.folds : 1, T = d * (d + 1) / 2;
        uint64_t *A = malloc(K * T * 8 + 1), *b = malloc(K * d * 8 + 1), *yy = p.job.want_yy ? malloc(K * 8) : NULL;
        if (!A || !b || (p.job.want_yy && !yy)) return 1;
        for (size_t i = 0; i < K * T; i++) A[i] = 1000 + i;
        for (size_t i = 0; i < K * d; i++) b[i] = 2000 + i;
        for (size_t i = 0; yy && i < K; i++) yy[i] = 3000 + i;
        printf("share");
        for (size_t i = 0; i < p.share_words; i++) printf(" %llu", (unsigned long long)run_share_word(&p, A, b, yy, i));
        printf("\n");
        free(A); free(b); free(yy);
    }
    if (planned) run_plan_free(&p);
    run_opts_free(&o);
    printf("all ok\n");
    return 0;
}
