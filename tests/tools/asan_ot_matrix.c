/* The pure-host part of --ot_matrix (host/ot_matrix_plan.c) as a program of its own, for the sanitizers: prints
 * otm_batch_rows(r, s, w) for every "r s w" triple on the command line, one per line, and checks the rule's two bounds itself.
 *   gcc -fsanitize=address,undefined -I linreg-mpc_amd/host tests/tools/asan_ot_matrix.c linreg-mpc_amd/host/ot_matrix_plan.c */
#include <stdio.h>
#include <stdlib.h>
#include "ot_matrix_plan.h"

int main(int argc, char **argv) {
    if ((argc - 1) % 3) { fprintf(stderr, "usage: %s r s w [r s w ...]\n", argv[0]); return 2; }
    for (int i = 1; i + 2 < argc; i += 3) {
        const size_t r = (size_t)strtoull(argv[i], NULL, 10), s = (size_t)strtoull(argv[i + 1], NULL, 10);
        const int w = atoi(argv[i + 2]);
        const size_t rows = otm_batch_rows(r, s, w);
        const uint64_t ots = (uint64_t)rows * r * (uint64_t)w, y = ots * s * (uint64_t)(w / 8);
        if (!rows) { fprintf(stderr, "no row in a batch\n"); return 1; }
        if (rows > 1 && (ots > OTM_MAX_OTS || y > OTM_MAX_Y_BYTES)) { fprintf(stderr, "a batch of %zu rows is too large\n", rows); return 1; }
        /* one more row would break a bound */
        if (ots + (uint64_t)r * (uint64_t)w <= OTM_MAX_OTS && y + (uint64_t)r * (uint64_t)w * s * (uint64_t)(w / 8) <= OTM_MAX_Y_BYTES) {
            fprintf(stderr, "a batch of %zu rows could hold another\n", rows); return 1;
        }
        printf("%zu\n", rows);
    }
    printf("all ok\n");
    return 0;
}
