/* phase1_ot_matrix.c -- the OT mode of phase 1 with one vector OT per bit of the receiver's operand (--use_ot --ot_matrix;
 * include/linreg_gc_ot_matrix.h): the block between two data providers is one Gilboa product X_r^T X_s, not one scalar product
 * per pair of columns.  The sender rule, the base OTs, the session and the buffers are phase1_ot.c's.  Per provider pair:
 *   both      after the base OTs, OTM_MAGIC (8 bytes) each way: a peer in another mode is refused, not waited for
 *   receiver  gathers its columns (with y if it is the last provider) into dense row-major batches of whole rows
 *             (otm_batch_rows, which both sides call); per batch a blob u one way, a blob y back
 *   sender    gathers its columns alike; its share block and the receiver's are summed over the batches and scattered
 * Two batches are in flight (ot_pipe.h).
 * --ot_half (include/linreg_gc_ot_half.h) is the same pair function and the same callbacks on another form (struct
 * ot_block_form): the half-payload calls, y of lgc_ot_gilboa_half_y_bytes, batches of otm_half_batch_rows and OTM_HALF_MAGIC in
 * place of OTM_MAGIC. */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include "../../include/linreg_gc.h"
#include "../../include/linreg_gc_ot_matrix.h"
#include "../../include/linreg_gc_ot_half.h"
#include "config.h"
#include "net.h"
#include "ot_matrix_plan.h"
#include "protocol.h"
#include "protocol_int.h"

void otm_hint_if_magic(uint64_t prefix) {
    if (prefix == OTM_MAGIC) fprintf(stderr, "the peer runs --ot_matrix (this party was started without it): run every party in the same mode\n");
    if (prefix == OTM_HALF_MAGIC) fprintf(stderr, "the peer runs --ot_matrix --ot_half (this party was started without them): run every party in the same mode\n");
}

/* batch k: rows [k per, ...) of the own columns, gathered row-major into vals; its r x s share block (part) is added to shares */
static int gather(void *pair, size_t k) {
    ot_pair *o = pair;
    const size_t row0 = k * o->per, rows = ot_pair_batch(o, k);
    for (size_t i = 0; i < rows; i++)
        for (size_t q = 0; q < o->ncols; q++)
            o->vals[i * o->ncols + q] = (uint64_t)(o->cols[q] < o->d ? o->Xq[(row0 + i) * o->d + o->cols[q]] : o->yq[row0 + i]);
    return 0;
}
static int add_part(ot_pair *o, int rc) {
    if (!lgc_said(rc)) for (size_t q = 0; q < o->r * o->s; q++) o->shares[q] += o->part[q];
    return rc;
}
/* what tells the mode's two forms apart: the library calls, the size of y, the batch rule, the magic word, the words of its messages */
struct ot_block_form {
    int (*recv_start)(lgc_ot_receiver *, const uint64_t *, size_t, size_t, size_t, int, uint8_t *);
    int (*send)(lgc_ot_sender *, const uint64_t *, size_t, size_t, size_t, int, const uint8_t *, void *, uint64_t *);
    int (*recv_finish)(lgc_ot_receiver *, const void *, uint64_t *);
    size_t (*y_bytes)(size_t, size_t, size_t, int);
    size_t (*batch_rows)(size_t, size_t, int);
    uint64_t magic;
    const char *flag, *mode, *other_form;       /* other_form: said when the peer sends the other form's magic word */
};
static const struct ot_block_form form_matrix = {
    lgc_ot_gilboa_matrix_recv_start, lgc_ot_gilboa_matrix_send, lgc_ot_gilboa_matrix_recv_finish, lgc_ot_gilboa_matrix_y_bytes,
    otm_batch_rows, OTM_MAGIC, "--ot_matrix", "matrix",
    "the peer runs --ot_matrix with --ot_half (this party was started without it): run every party in the same mode"};
static const struct ot_block_form form_half = {
    lgc_ot_gilboa_half_recv_start, lgc_ot_gilboa_half_send, lgc_ot_gilboa_half_recv_finish, lgc_ot_gilboa_half_y_bytes,
    otm_half_batch_rows, OTM_HALF_MAGIC, "--ot_half", "matrix, half payload",
    "the peer runs --ot_matrix without --ot_half (this party was started with it): run every party in the same mode"};

static int otm_start(void *pair, size_t k, void *u) {
    ot_pair *o = pair;
    return lgc_said(o->form->recv_start(o->R, o->vals, ot_pair_batch(o, k), o->r, o->s, o->w1, u));
}
static int otm_send(void *pair, size_t k, const void *u, void *y) {
    ot_pair *o = pair;
    return add_part(o, o->form->send(o->S, o->vals, ot_pair_batch(o, k), o->r, o->s, o->w1, u, y, o->part));
}
static int otm_finish(void *pair, size_t k, const void *y) {
    ot_pair *o = pair;
    (void)k;
    return add_part(o, o->form->recv_finish(o->R, y, o->part));
}
static size_t otm_u_bytes(void *pair, size_t k) {
    const ot_pair *o = pair;
    return lgc_ot_u_bytes((uint64_t)ot_pair_batch(o, k) * o->r * (uint64_t)o->w1);
}
static size_t otm_y_bytes(void *pair, size_t k) {
    const ot_pair *o = pair;
    return o->form->y_bytes(ot_pair_batch(o, k), o->r, o->s, o->w1);
}
static int otm_get(void *pair, void *buf, size_t len) {
    ot_pair *o = pair;
    return recv_blob(o->self, o->peer, buf, len);
}
static const ot_pipe otm_pipe = {.prepare = gather, .start = otm_start, .finish = otm_finish, .send = otm_send,
                                 .u_bytes = otm_u_bytes, .y_bytes = otm_y_bytes, .put = ot_put_blob, .get = otm_get};

/* One provider pair: the block of the sender's columns [i0, i1) against the receiver's [j0, j1), each with y (column d) where that
 * side is the last provider, as one product; word (receiver column ir, sender column j) is added where the per-pair mode puts that
 * pair's */
int run_party_ot_matrix_pair(ot_pair *o, int half, size_t i0, size_t i1, int y_on_sender, size_t j0, size_t j1, int y_on_receiver,
                             uint64_t *share_A, uint64_t *share_b) {
    const size_t d = o->d, s = (i1 - i0) + (y_on_sender != 0), r = (j1 - j0) + (y_on_receiver != 0);
    if (!s || !r) return 0;                                                  /* (both sides count alike) */
    size_t *cs = malloc(s * sizeof *cs), *cr = malloc(r * sizeof *cr);
    int rc = 1;
    o->shares = calloc(r * s, 8); o->part = malloc(r * s * 8);
    check(cs && cr && o->shares && o->part, "out of memory");
    for (size_t j = 0; j < s; j++) cs[j] = i0 + j < i1 ? i0 + j : d;
    for (size_t j = 0; j < r; j++) cr[j] = j0 + j < j1 ? j0 + j : d;
    o->cols = o->i_am_sender ? cs : cr; o->ncols = o->i_am_sender ? s : r; o->r = r; o->s = s;
    const struct ot_block_form *f = o->form = half ? &form_half : &form_matrix;
    o->total = o->n; o->per = f->batch_rows(r, s, o->w1);
    if (o->per > o->n) o->per = o->n;
    if (ot_pair_open(o)) goto error;
    uint64_t magic = f->magic, theirs = 0;
    check(!net_send(o->self, o->peer, &magic, sizeof magic), "Could not send to party %d", o->peer);
    const int got = !net_recv(o->self, o->peer, &theirs, sizeof theirs);
    if (got && theirs != magic && (theirs == OTM_MAGIC || theirs == OTM_HALF_MAGIC)) fprintf(stderr, "%s\n", f->other_form);
    check(got && theirs == magic, "party %d does not speak %s (this party was started with it): run every party in the same mode", o->peer, f->flag);
    check(!ot_pair_run(o, &otm_pipe, o->per * o->ncols * 8, lgc_ot_u_bytes((uint64_t)o->per * r * (uint64_t)o->w1), f->y_bytes(o->per, r, s, o->w1)),
          "OT-mode aggregation (%s) failed", f->mode);
    for (size_t ir = 0; ir < r; ir++)
        for (size_t j = 0; j < s; j++)
            *(cs[j] < d && cr[ir] < d ? share_A + idx(cs[j], cr[ir]) : share_b + (cs[j] < d ? cs[j] : cr[ir])) += o->shares[ir * s + j];
    rc = 0;
error:
    ot_pair_close(o);
    free(cs); free(cr);
    return rc;
}
