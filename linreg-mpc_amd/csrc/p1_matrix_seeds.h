// p1_matrix_seeds.h -- the seed derivation of the matrix-triple mode (include/linreg_gc_p1_matrix.h), host only: the seeds of
// instance u are blocks 3u, 3u + 1, 3u + 2 of the AES-128-CTR keystream of the master seed (block c = AES_master(c as a
// little-endian 128-bit number), the counter convention of ti_prg_kernel).  No device code: lgc_ti_matrix_seeds is this, and a
// plain host compiler builds it too (tests/tools/asan_ti_matrix.cpp).
#pragma once
#include <stdint.h>
#include "gc_aes.h"

namespace gc {
inline void p1_matrix_seeds(const uint8_t master[16], uint64_t u, uint8_t seed_a[16], uint8_t seed_b[16], uint8_t seed_s[16]) {
    AesTables t;
    aes_build_tables(t, master);
    HostTab ht = {t.te0};
    uint8_t *dst[3] = {seed_a, seed_b, seed_s};
    for (int k = 0; k < 3; k++) {
        const uint64_t c = 3 * u + (uint64_t)k;
        uint32_t s[1][4] = {{(uint32_t)c, (uint32_t)(c >> 32), 0u, 0u}};
        aes_encrypt_n<1, HostTab>(ht, t.rk, s);
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) dst[k][4 * i + j] = (uint8_t)(s[0][i] >> (8 * j));
    }
}
}  // namespace gc
