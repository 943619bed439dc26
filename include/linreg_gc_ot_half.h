/*
 * linreg_gc_ot_half.h -- the half-payload form of the matrix Gilboa product (bin/linreg --use_ot --ot_matrix --ot_half;
 * liblinreg_gc.so).  In OT i of bit `bit` the sender's correlation Xs[k][j] << bit has `bit` zero low bits, so only W - bit bits of
 * y carry information: Gilboa's product runs modulo 2^(W - bit) for that bit and is shifted afterwards.  Over the W bits of a word
 * y shrinks to a little over half, with the OTs, the extension and the pads of linreg_gc_ot_matrix.h.
 *
 * Everything of linreg_gc_ot_matrix.h stands unless said otherwise here: the block is between a sender that holds Xs (rows x s
 * words, row-major) and a receiver that holds Xr (rows x r), W is the width (32 or 64), the calls act on the sessions of
 * linreg_gc.h and may be mixed with matrix batches, per-pair batches and label transfers on one session.
 *
 *   OT index     i = (k * r + ir) * W + bit, M = rows * r * W; the choice bits and the extension are the matrix mode's: u is byte
 *                for byte what lgc_ot_gilboa_matrix_recv_start writes for the same session state and Xr
 *   pads         nblk = ceil(s * W / 128) blocks per OT, block c = H(row_i, tweak0 + i * nblk + c), word e of block c belongs to
 *                sender column j = c * (128 / W) + e
 *   counters     the tweak counter advances by M * nblk, the PRG counter by ceil(M / 128), as in the matrix mode
 *   with n_b = W - bit and m_b = 2^(n_b) - 1, for OT i of bit `bit` and sender column j:
 *   sender       x0, x1 = the pad words of q_i and q_i ^ delta,
 *                y'[i][j] = (x0 + Xs[k][j] - x1) & m_b,  share_s[ir][j] -= (x0 & m_b) << bit
 *   receiver     share_r[ir][j] += ((pad(t_i)[j] + c_i * y'[i][j]) & m_b) << bit
 *   sum          both sums mod 2^W; share_s + share_r = (Xr^T Xs)[ir][j] mod 2^W, the word the matrix mode and the per-pair mode
 *                share for that pair of columns (the individual shares differ from the matrix mode's)
 *
 * Wire form.  The W fields y' of one (k, ir, j) have W, W - 1, ..., 1 bits and pack into H = W / 2 + 1 words of W bits, no field
 * straddling a word:
 *   word 0               y' of bit 0, all W bits
 *   word p, 1 <= p < W/2 y' of bit p in bits [0, W - p), y' of bit W - p (p bits) in bits [W - p, W)
 *   word W / 2           y' of bit W / 2 in the low W / 2 bits; the high half is zero
 * y is (k, ir)-major, then p, then j: word ((k * r + ir) * H + p) * s + j, uint32_t at W = 32 and uint64_t at W = 64,
 * rows * r * H * s * W / 8 bytes (lgc_ot_gilboa_half_y_bytes): 33/64 of the matrix mode's at W = 64 and 17/32 at W = 32.  Operands,
 * shares, device I/O (lgc_ot_*_set_device_io; whole 16-byte accesses to y when s * W is a multiple of 128 and y is 16-byte
 * aligned, word accesses otherwise) and the lifetime of xr are as in linreg_gc_ot_matrix.h.
 *
 * Up to four receives of any kind may be in flight on a receiver; a half receive is a kind of its own: finishing the oldest
 * receive through a call of another kind is LGC_ESTATE and leaves it in flight, both ways.  LGC_EINVAL, before any device work: a
 * null argument, a width other than 32 or 64, rows, r or s equal to 0, a batch of 2^32 OTs or more, r * nblk of 2^31 or more, a y
 * of 2^63 bytes or more.
 */
#ifndef LINREG_GC_OT_HALF_H
#define LINREG_GC_OT_HALF_H
#include "linreg_gc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of y for one batch: rows * r * (W / 2 + 1) * s words of W bits; 0 for a width other than 32 or 64 or a size of 2^63 or more */
size_t lgc_ot_gilboa_half_y_bytes(size_t rows, size_t r, size_t s, int width);
/* receiver: extends M OTs on the bits of xr (rows x r) and writes u (lgc_ot_u_bytes(M) bytes) */
int lgc_ot_gilboa_half_recv_start(lgc_ot_receiver *R, const uint64_t *xr, size_t rows, size_t r, size_t s, int width, uint8_t *u_out);
/* sender: xs is rows x s; writes y (wire form) and its r x s share block */
int lgc_ot_gilboa_half_send(lgc_ot_sender *S, const uint64_t *xs, size_t rows, size_t r, size_t s, int width, const uint8_t *u_in,
                            void *y_out, uint64_t *shares);
/* receiver: completes the oldest receive in flight, which must be a half one; writes its r x s share block */
int lgc_ot_gilboa_half_recv_finish(lgc_ot_receiver *R, const void *y_in, uint64_t *shares);

#ifdef __cplusplus
}
#endif
#endif
