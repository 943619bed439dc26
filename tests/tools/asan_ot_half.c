/* The pure-host part of --ot_half (host/ot_matrix_plan.c) as a program of its own, for the sanitizers: prints
 * otm_half_batch_rows(r, s, w) for every "r s w" triple on the command line, one per line, and checks the rule's two bounds itself
 * on the half y of a row, r (w / 2 + 1) s w / 8 bytes.
 *   gcc -fsanitize=address,undefined -I linreg-mpc_amd/host tests/tools/asan_ot_half.c linreg-mpc_amd/host/ot_matrix_plan.c */
#include <stdio.h>
#include <stdlib.h>
#include "ot_matrix_plan.h"

int main(int argc, char **argv) {
    if ((argc - 1) % 3) { fprintf(stderr, "usage: %s r s w [r s w ...]\n", argv[0]); return 2; }
    for (int i = 1; i + 2 < argc; i += 3) {
        const size_t r = (size_t)strtoull(argv[i], NULL, 10), s = (size_t)strtoull(argv[i + 1], NULL, 10);
        const int w = atoi(argv[i + 2]);
        const size_t rows = otm_half_batch_rows(r, s, w);
        const uint64_t row_ots = (uint64_t)r * (uint64_t)w, row_y = (uint64_t)r * (uint64_t)(w / 2 + 1) * s * (uint64_t)(w / 8);
        const uint64_t ots = (uint64_t)rows * row_ots, y = (uint64_t)rows * row_y;
        if (!rows) { fprintf(stderr, "no row in a batch\n"); return 1; }
        if (rows > 1 && (ots > OTM_MAX_OTS || y > OTM_MAX_Y_BYTES)) { fprintf(stderr, "a batch of %zu rows is too large\n", rows); return 1; }
        /* one more row would break a bound */
        if (ots + row_ots <= OTM_MAX_OTS && y + row_y <= OTM_MAX_Y_BYTES) { fprintf(stderr, "a batch of %zu rows could hold another\n", rows); return 1; }
        /* never fewer rows than the matrix mode's rule gives */
        if (rows < otm_batch_rows(r, s, w)) { fprintf(stderr, "fewer rows than the full-payload rule\n"); return 1; }
        printf("%zu\n", rows);
    }
    printf("all ok\n");
    return 0;
}
