/* ot_matrix_plan.c -- see ot_matrix_plan.h */
#include "ot_matrix_plan.h"

/* as many whole rows as keep both the OTs and the bytes of y of a batch within their limits, and at least one */
static size_t batch_rows(uint64_t row_ots, uint64_t row_y) {
    uint64_t a = OTM_MAX_OTS / row_ots;
    const uint64_t b = OTM_MAX_Y_BYTES / row_y;
    if (b < a) a = b;
    return a ? (size_t)a : 1;
}

size_t otm_batch_rows(size_t r, size_t s, int w) {
    return batch_rows((uint64_t)r * (uint64_t)w, (uint64_t)r * (uint64_t)w * (uint64_t)s * (uint64_t)(w / 8));
}

size_t otm_half_batch_rows(size_t r, size_t s, int w) {
    return batch_rows((uint64_t)r * (uint64_t)w, (uint64_t)r * (uint64_t)(w / 2 + 1) * (uint64_t)s * (uint64_t)(w / 8));
}
