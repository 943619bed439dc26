/* ti_matrix_plan.c -- see ti_matrix_plan.h */
#include <stdlib.h>
#include <string.h>
#include "ti_matrix_plan.h"

size_t tm_plan(const int *owner, size_t d, int num_parties, tm_inst **out) {
    size_t count = 0, cap = 0;
    tm_inst *v = NULL;
    uint64_t u = 0;
    for (int lo = 2; lo < num_parties; lo++)
        for (int hi = lo + 1; hi < num_parties; hi++, u++) {
            size_t a = 0, b = 0;
            for (size_t i = 0; i <= d; i++) { a += owner[i] == hi; b += i < d && owner[i] == lo; }
            if (!a || !b) continue;
            if (count == cap) {
                cap = cap ? 2 * cap : 8;
                tm_inst *nv = realloc(v, cap * sizeof *v);
                if (!nv) { tm_plan_free(v, count); return (size_t)-1; }
                v = nv;
            }
            tm_inst t = {lo, hi, u, malloc(a * sizeof(uint32_t)), malloc(b * sizeof(uint32_t)), 0, 0};
            if (!t.cols_a || !t.cols_b) { free(t.cols_a); free(t.cols_b); tm_plan_free(v, count); return (size_t)-1; }
            for (size_t i = 0; i <= d; i++) {
                if (owner[i] == hi) t.cols_a[t.a++] = (uint32_t)i;
                else if (i < d && owner[i] == lo) t.cols_b[t.b++] = (uint32_t)i;
            }
            v[count++] = t;
        }
    *out = v;
    return count;
}
void tm_plan_free(tm_inst *v, size_t count) {
    for (size_t k = 0; v && k < count; k++) { free(v[k].cols_a); free(v[k].cols_b); }
    free(v);
}
static size_t tm_idx(size_t i, size_t j) { if (j > i) { size_t t = i; i = j; j = t; } return i * (i + 1) / 2 + j; }
void tm_scatter(const tm_inst *t, const uint64_t *blk, size_t d, uint64_t *share_A, uint64_t *share_b) {
    for (size_t i = 0; i < t->a; i++)
        for (size_t j = 0; j < t->b; j++) {
            const size_t ci = t->cols_a[i], cj = t->cols_b[j];
            if (ci < d) share_A[tm_idx(ci, cj)] = blk[i * t->b + j];
            else share_b[cj] = blk[i * t->b + j];
        }
}
size_t tm_msg_b_bytes(const tm_inst *t, int width) { return 16 + t->a * t->b * (size_t)(width / 8); }
void tm_msg_a(const uint8_t seed_a[16], const uint8_t seed_s[16], uint8_t out[TM_MSG_A_BYTES]) {
    memcpy(out, seed_a, 16);
    memcpy(out + 16, seed_s, 16);
}
uint8_t *tm_msg_b(const tm_inst *t, int width, const uint8_t seed_b[16], const void *T, size_t *len) {
    *len = tm_msg_b_bytes(t, width);
    uint8_t *m = malloc(*len);
    if (!m) return NULL;
    memcpy(m, seed_b, 16);
    memcpy(m + 16, T, *len - 16);
    return m;
}
