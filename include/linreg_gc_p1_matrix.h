/*
 * linreg_gc_p1_matrix.h -- phase 1 under the trusted initializer with ONE matrix triple per pair of data providers
 * (bin/linreg --ti_matrix; liblinreg_gc.so), instead of one vector triple per pair of columns.
 *
 * The cross block between provider A (a columns cols_a, the provider with the higher columns: y, column d, can only be
 * on its side) and provider B (b columns cols_b) is the matrix product X_a^T X_b over the n rows of the window.  With
 * W the phase-1 width and m = 2^W - 1:
 *
 *   randomness   three AES-128-CTR keystreams (block c = AES_seed(c as a little-endian 128-bit number), W-bit
 *                little-endian words, from block 0): R_a is n x a from seed_a, R_b is n x b from seed_b, S is a x b from
 *                seed_s; word k * cols + i of a stream is entry [k][i].  All matrices are row-major.
 *   initializer  sends (seed_a, seed_s) to A; seed_b and T = (R_a^T R_b - S) & m to B
 *   A            sends E = (X_a - R_a) & m to B; its share is (R_a^T F + S) & m
 *   B            sends F = (X_b - R_b) & m to A; its share is (E^T X_b + T) & m
 *
 * The two shares sum to X_a^T X_b mod 2^W: entry [i][j] is <column cols_a[i], column cols_b[j]>.
 *
 * Wire form.  E, F and T are what travels: W-bit little-endian words back to back (uint32_t at W = 32, uint64_t at W = 64),
 * n * ncols of them for E and F, a * b for T.  The shares (`out`) are a x b uint64_t words, masked to W bits.
 *
 * The calls act on the row window of the handle (lgc_p1_set_rows: n is the window's row count) and follow
 * lgc_p1_set_device_io: with device I/O on, the blocks E and F (out_E, F, E below) are device memory; seeds, column lists,
 * T and the shares stay on the host.  They take turns on the device like lgc_p1_mask and may be called from several
 * threads on one handle.  A call with ncols, a or b equal to 0 launches nothing and writes nothing.
 *
 * LGC_EINVAL, before any device work: a null argument, a column index past d, column d when y is not set, a width other
 * than 32 or 64 (lgc_ti_matrix_generate), n == 0 there.
 *
 * Seeds.  The initializer derives the three seeds of instance u as blocks 3u, 3u + 1, 3u + 2 of the keystream of its master
 * seed: lgc_ti_matrix_seeds is the one statement of that rule, on the host alone.  Instances are numbered over the provider
 * pairs (lo, hi), lo ascending, then hi ascending, pairs without a cross block included: every party derives the same u.
 */
#ifndef LINREG_GC_P1_MATRIX_H
#define LINREG_GC_P1_MATRIX_H
#include "linreg_gc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out_E: the n x ncols block (X[:, cols] - R) & m in wire form, R the keystream of `seed` */
int lgc_p1_matrix_mask(lgc_p1 *h, const uint32_t *cols, size_t ncols, const uint8_t seed[16], void *out_E);
/* A's share: out[i][j] = (R_a^T F + S)[i][j] & m; F is B's n x ncols_b block in wire form */
int lgc_p1_matrix_share_a(lgc_p1 *h, size_t ncols_a, const uint8_t seed_a[16], const uint8_t seed_s[16], const void *F, size_t ncols_b,
                          uint64_t *out);
/* B's share: out[i][j] = (E^T X[:, cols_b] + T)[i][j] & m; E is A's n x ncols_a block, T the initializer's a x b words */
int lgc_p1_matrix_share_b(lgc_p1 *h, const uint32_t *cols_b, size_t ncols_b, const void *E, size_t ncols_a, const void *T, uint64_t *out);
/* the initializer: out_T = (R_a^T R_b - S) & m, a x b words in wire form */
int lgc_ti_matrix_generate(int device, const uint8_t seed_a[16], const uint8_t seed_b[16], const uint8_t seed_s[16], size_t n, size_t a,
                           size_t b, int width, void *out_T);
/* the seeds of instance u from the master seed (host only) */
int lgc_ti_matrix_seeds(const uint8_t master[16], uint64_t u, uint8_t seed_a[16], uint8_t seed_b[16], uint8_t seed_s[16]);

#ifdef __cplusplus
}
#endif
#endif
