/* The pure-host plan of phase 1 (host/phase1_plan.c) as a program of its own, for the sanitizers: one column layout per run,
 *     asan_phase1_plan d M start_of_provider_0 start_of_provider_1 ...
 * prints, from lists allocated at exactly their sizes,
 *     ti pa pb ci cj                    every cross pair in the initializer's loop order
 *     view me peer is_a col             every provider's view of its pairs, in that order
 *     ot sender receiver ri rj          every provider pair's pairs in the OT modes' block order
 * and "all ok".  Party indices are 0-based with the providers from 2, as everywhere in the host.
 *   gcc -fsanitize=address,undefined -I linreg-mpc_amd/host tests/tools/asan_phase1_plan.c linreg-mpc_amd/host/phase1_plan.c */
#include <stdio.h>
#include <stdlib.h>
#include "phase1_plan.h"

int main(int argc, char **argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s d M start [start ...]\n", argv[0]); return 2; }
    const size_t d = (size_t)strtoull(argv[1], NULL, 10), M = (size_t)strtoull(argv[2], NULL, 10);
    const int P = argc - 3, NP = P + 2, last = NP - 1;
    size_t *start = malloc((size_t)NP * sizeof *start);
    int *owner = malloc((d + 1) * sizeof *owner);
    if (!start || !owner) return 1;
    for (int k = 2; k < NP; k++) start[k] = (size_t)strtoull(argv[k + 1], NULL, 10);
    for (size_t i = 0; i <= d; i++) {                                /* config_owner: the last provider that starts at or before i */
        owner[i] = 2;
        for (int k = 3; k < NP; k++) if (start[k] <= i) owner[i] = k;
    }
    p1_pair *plan = NULL;
    const size_t np = p1_plan_ti(owner, d, M, &plan);
    if (np == (size_t)-1) return 1;
    for (size_t q = 0; q < np; q++) printf("ti %d %d %u %u\n", plan[q].pa, plan[q].pb, plan[q].ci, plan[q].cj);
    for (int me = 2; me < NP; me++)
        for (size_t q = 0; q < np; q++) {
            p1_view v;
            if (p1_pair_view(&plan[q], me, &v)) printf("view %d %d %d %u\n", me, v.peer, v.is_a, v.col);
        }
    free(plan);
    for (int lo = 2; lo < NP; lo++)
        for (int hi = lo + 1; hi < NP; hi++) {
            const int s = p1_ot_i_am_sender(lo, hi) ? lo : hi, r = s == lo ? hi : lo;
            const size_t i0 = start[s], i1 = s < last ? start[s + 1] : d, j0 = start[r], j1 = r < last ? start[r + 1] : d;
            size_t *ri = NULL, *rj = NULL;
            const size_t n = p1_plan_ot(d, M, i0, i1, s == last, j0, j1, r == last, &ri, &rj);
            if (n == (size_t)-1) return 1;
            for (size_t q = 0; q < n; q++) printf("ot %d %d %zu %zu\n", s, r, ri[q], rj[q]);
            free(ri); free(rj);
        }
    free(start); free(owner);
    printf("all ok\n");
    return 0;
}
