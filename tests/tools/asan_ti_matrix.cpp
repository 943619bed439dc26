/* asan_ti_matrix.cpp -- the host-only pieces of the matrix-triple mode under AddressSanitizer + UBSan, as a stand-alone program:
 * the seed derivation (csrc/p1_matrix_seeds.h), the plan of instances, the scatter of a share block into share_A / share_b and the
 * initializer's messages (host/ti_matrix_plan.c).  Every buffer is a heap block of exactly its size.
 *   gcc -O1 -g -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=all -c linreg-mpc_amd/host/ti_matrix_plan.c -o plan.o
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I linreg-mpc_amd/host -I linreg-mpc_amd/csrc \
 *       tests/tools/asan_ti_matrix.cpp plan.o -o asan_ti_matrix && ./asan_ti_matrix */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "p1_matrix_seeds.h"
extern "C" {
#include "ti_matrix_plan.h"
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static void hex(const uint8_t *b, char *out) { for (int i = 0; i < 16; i++) sprintf(out + 2 * i, "%02x", b[i]); }

static void seeds() {
    uint8_t *master = (uint8_t *)malloc(16), *sa = (uint8_t *)malloc(16), *sb = (uint8_t *)malloc(16), *ss = (uint8_t *)malloc(16);
    char h[33];
    for (int i = 0; i < 16; i++) master[i] = (uint8_t)i;
    gc::p1_matrix_seeds(master, 0, sa, sb, ss);
    hex(sa, h); CHECK(!strcmp(h, "c6a13b37878f5b826f4f8162a1c8d879"));      /* FIPS-197: key 00..0f on the zero block */
    hex(sb, h); CHECK(!strcmp(h, "e37cd363dd7c87a09aff0e3e60e09c82"));
    hex(ss, h); CHECK(!strcmp(h, "fb8ae31ba5db9cad97364d8722d47326"));
    for (int i = 0; i < 16; i++) master[i] = (uint8_t)(15 - i);
    gc::p1_matrix_seeds(master, 5, sa, sb, ss);
    hex(sa, h); CHECK(!strcmp(h, "84fd42fa6e626114623c491b85166ae5"));
    hex(ss, h); CHECK(!strcmp(h, "2a3b32cb2c73f29476f3277a05888ea0"));
    gc::p1_matrix_seeds(master, (~0ull - 2) / 3, sa, sb, ss);                /* the largest instance number: 3u + 2 does not wrap */
    free(master); free(sa); free(sb); free(ss);
}

/* providers hold the columns from first[k] on (party index k + 2); column d is y, the last provider's */
static void plan(size_t d, std::vector<size_t> first, int width) {
    const int NP = (int)first.size() + 2;
    int *owner = (int *)malloc((d + 1) * sizeof(int));
    for (size_t i = 0; i <= d; i++) {
        owner[i] = 2;
        for (int k = 1; k < NP - 2; k++) if (first[(size_t)k] <= i) owner[i] = k + 2;
    }
    tm_inst *v = NULL;
    const size_t count = tm_plan(owner, d, NP, &v);
    CHECK(count != (size_t)-1);
    const size_t T = d * (d + 1) / 2;
    uint64_t *share_A = (uint64_t *)calloc(T ? T : 1, 8), *share_b = (uint64_t *)calloc(d, 8);
    uint64_t last_u = 0;
    size_t cross = 0;
    for (size_t q = 0; q < count; q++) {
        const tm_inst *t = &v[q];
        CHECK(t->lo < t->hi && t->a && t->b && (q == 0 || t->u > last_u));
        last_u = t->u;
        /* u is the rank of (lo, hi) among all provider pairs, whether listed or not */
        uint64_t rank = 0;
        for (int lo = 2; lo < NP; lo++) for (int hi = lo + 1; hi < NP; hi++) { if (lo == t->lo && hi == t->hi) goto found; rank++; }
    found:
        CHECK(rank == t->u);
        for (size_t i = 0; i < t->a; i++) CHECK(owner[t->cols_a[i]] == t->hi && (i == 0 || t->cols_a[i] > t->cols_a[i - 1]));
        for (size_t j = 0; j < t->b; j++) CHECK(owner[t->cols_b[j]] == t->lo && t->cols_b[j] < d);
        uint64_t *blk = (uint64_t *)malloc(t->a * t->b * 8);
        for (size_t k = 0; k < t->a * t->b; k++) blk[k] = 1;
        /* the scatter of both sides adds up to one per cross entry: every entry written, none twice */
        uint64_t *tA = (uint64_t *)calloc(T ? T : 1, 8), *tb = (uint64_t *)calloc(d, 8);
        tm_scatter(t, blk, d, tA, tb);
        for (size_t k = 0; k < T; k++) { share_A[k] += tA[k]; cross += tA[k]; }
        for (size_t k = 0; k < d; k++) { share_b[k] += tb[k]; cross += tb[k]; }
        CHECK(cross > 0);
        /* the initializer's messages */
        uint8_t sa[16], sb[16], ss[16], ma[TM_MSG_A_BYTES];
        memset(sa, 1, 16); memset(sb, 2, 16); memset(ss, 3, 16);
        tm_msg_a(sa, ss, ma);
        CHECK(ma[0] == 1 && ma[15] == 1 && ma[16] == 3 && ma[31] == 3);
        const size_t tbytes = t->a * t->b * (size_t)(width / 8);
        uint8_t *Tm = (uint8_t *)malloc(tbytes);
        memset(Tm, 7, tbytes);
        size_t len = 0;
        uint8_t *mb = tm_msg_b(t, width, sb, Tm, &len);
        CHECK(mb && len == 16 + tbytes && len == tm_msg_b_bytes(t, width) && mb[0] == 2 && mb[15] == 2 && mb[16] == 7 && mb[len - 1] == 7);
        free(mb); free(Tm); free(blk); free(tA); free(tb);
    }
    /* exactly the entries whose two columns lie with different providers, once each */
    size_t want = 0;
    for (size_t i = 0; i <= d; i++)
        for (size_t j = 0; j <= i && j < d; j++) {
            const int x = owner[i] != owner[j];
            want += (size_t)x;
            CHECK((i < d ? share_A[i * (i + 1) / 2 + j] : share_b[j]) == (uint64_t)x);
        }
    CHECK(cross == want);
    tm_plan_free(v, count);
    free(owner); free(share_A); free(share_b);
}

int main() {
    seeds();
    for (int width = 32; width <= 64; width += 32) {
        plan(5, {0, 1, 2}, width);            /* the README example */
        plan(7, {0, 1, 5}, width);            /* 1, 4 and 2 columns */
        plan(4, {0}, width);                  /* one provider: no instance */
        plan(6, {0, 3}, width);
        plan(6, {0, 0, 4}, width);            /* the first provider holds no column: its pairs are numbered, not listed */
        plan(9, {0, 2, 2, 7, 9}, width);      /* a provider without columns in the middle; the last one holds y alone */
        plan(1, {0, 1}, width);               /* y alone against one column */
    }
    puts("all ok");
    return 0;
}
