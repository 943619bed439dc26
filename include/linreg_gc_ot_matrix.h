/*
 * linreg_gc_ot_matrix.h -- Gilboa products of a whole block X_r^T X_s over IKNP OT extension with ONE vector OT per bit of
 * the receiver's operand (bin/linreg --use_ot --ot_matrix; liblinreg_gc.so), instead of one scalar correlated OT per bit of
 * every pair of columns (lgc_ot_gilboa_*, linreg_gc.h).
 *
 * One block is between a sender that holds Xs (rows x s words, row-major) and a receiver that holds Xr (rows x r).  W is the
 * width (32 or 64), m = 2^W - 1.  The calls act on the sessions of linreg_gc.h (lgc_ot_sender / lgc_ot_receiver) and may be
 * mixed with the per-pair Gilboa and label transfers on one session.
 *
 *   OT index     i = (k * r + ir) * W + bit, least significant bit first: M = rows * r * W OTs.  The choice c_i is bit `bit`
 *                of Xr[k][ir] (the packing of the dense rows x r block, as lgc_ot_gilboa_recv_start packs its operand).
 *   extension    as for every transfer: u is lgc_ot_u_bytes(M) bytes, the session's PRG counter advances by ceil(M / 128).
 *   pads         nblk = ceil(s * W / 128).  Block c of OT i is H(row_i, tweak0 + i * nblk + c), the fixed-key gate hash of
 *                the other transfers; its 16 bytes are 128 / W little-endian W-bit words, word e of block c belongs to
 *                sender column j = c * (128 / W) + e, words with j >= s are discarded.  The session's tweak counter advances
 *                by M * nblk on both sides.
 *   sender       x0[i][j] = pad word of q_i, x1[i][j] = pad word of q_i ^ delta,
 *                y[i][j] = (x0 + (Xs[k][j] << bit) - x1) & m, share_s[ir][j] = (-sum over (k, bit) of x0[i][j]) & m
 *   receiver     share_r[ir][j] = (sum over (k, bit) of pad(t_i)[j] + c_i * y[i][j]) & m
 *   sum          share_s + share_r = (Xr^T Xs)[ir][j] mod 2^W: the word the per-pair protocol shares for that pair of columns
 *
 * Wire form.  y is OT-major, s words per OT back to back: word i * s + j, uint32_t at W = 32 and uint64_t at W = 64,
 * M * s * W / 8 bytes (lgc_ot_gilboa_matrix_y_bytes).  The operands are uint64_t words of which the low W bits count.  The
 * shares are r x s uint64_t words, row-major: masked to W bits with host pointers; with device I/O on
 * (lgc_ot_*_set_device_io: every pointer argument is device memory) only their low W bits are defined, as for
 * lgc_ot_gilboa_*.  Under device I/O the receiver does not copy xr: lgc_ot_gilboa_matrix_recv_finish reads it again, so it must
 * stay valid and unchanged from the start of a receive to its finish (with host pointers the start takes a copy).
 *
 * Up to four receives of any kind may be in flight on a receiver; finishes complete the oldest, and a finish of another kind
 * than the oldest start is LGC_ESTATE (that receive stays in flight).  LGC_EINVAL, before any device work: a null argument, a
 * width other than 32 or 64, rows, r or s equal to 0, a batch of 2^32 OTs or more, a y of 2^63 bytes or more.
 */
#ifndef LINREG_GC_OT_MATRIX_H
#define LINREG_GC_OT_MATRIX_H
#include "linreg_gc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of y for one batch: rows * r * W OTs of s W-bit words; 0 for a width other than 32 or 64 or a size of 2^63 or more */
size_t lgc_ot_gilboa_matrix_y_bytes(size_t rows, size_t r, size_t s, int width);
/* receiver: extends M OTs on the bits of xr (rows x r) and writes u (lgc_ot_u_bytes(M) bytes) */
int lgc_ot_gilboa_matrix_recv_start(lgc_ot_receiver *R, const uint64_t *xr, size_t rows, size_t r, size_t s, int width, uint8_t *u_out);
/* sender: xs is rows x s; writes y (wire form) and its r x s share block */
int lgc_ot_gilboa_matrix_send(lgc_ot_sender *S, const uint64_t *xs, size_t rows, size_t r, size_t s, int width, const uint8_t *u_in,
                              void *y_out, uint64_t *shares);
/* receiver: completes the oldest receive in flight, which must be a matrix one; writes its r x s share block */
int lgc_ot_gilboa_matrix_recv_finish(lgc_ot_receiver *R, const void *y_in, uint64_t *shares);

#ifdef __cplusplus
}
#endif
#endif
