/* phase1_ot.c -- the OT mode of phase 1 on a data provider (--use_ot; src/phase1.c:353-450): the provider pairs in a global order
 * and the sender rule, what both modes do per provider pair (base OTs, the session, the page-locked buffers: ot_pair_*), and the
 * per-pair mode itself: Gilboa products of column pairs over the IKNP extension, in batches through ot_pipe or, with --ot_ring,
 * through device rings.  The matrix mode's batches are phase1_ot_matrix.c's. */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include "../../include/linreg_gc.h"
#include "baseot.h"
#include "config.h"
#include "net.h"
#include "protocol.h"
#include "protocol_int.h"

/* ---------------------------------------------------------------- one provider pair, either mode */
int ot_pair_open(ot_pair *o) {
    if (o->i_am_sender) {
        uint8_t delta[16], seeds[128][16];
        check(!baseot_ext_sender(o->self, o->peer, delta, seeds), "base OT failed");
        LGC(lgc_ot_sender_create(&o->S, o->device, delta, seeds));
    } else {
        uint8_t s0[128][16], s1[128][16];
        check(!baseot_ext_receiver(o->self, o->peer, s0, s1), "base OT failed");
        LGC(lgc_ot_receiver_create(&o->R, o->device, s0, s1));
    }
    return 0;
error:
    return 1;
}
int ot_pair_run(ot_pair *o, const ot_pipe *calls, size_t vals_bytes, size_t u_bytes, size_t y_bytes) {
    o->pipe = *calls; o->pipe.arg = o; o->pipe.nbatch = (o->total + o->per - 1) / o->per;
    o->vals = lgc_host_alloc(vals_bytes);
    check(o->vals != NULL, "%s", lgc_last_error());
    for (int k = 0; k < (o->i_am_sender ? 2 : 1); k++) {
        o->pipe.u[k] = lgc_host_alloc(u_bytes); o->pipe.y[k] = lgc_host_alloc(y_bytes);
        check(o->pipe.u[k] && o->pipe.y[k], "%s", lgc_last_error());
    }
    return (o->i_am_sender ? ot_pipe_send : ot_pipe_receive)(&o->pipe);
error:
    return 1;
}
void ot_pair_close(ot_pair *o) {
    if (o->S) lgc_ot_sender_destroy(o->S);
    if (o->R) lgc_ot_receiver_destroy(o->R);
    for (int k = 0; k < 2; k++) { lgc_host_free(o->pipe.u[k]); lgc_host_free(o->pipe.y[k]); }
    lgc_host_free(o->vals);
    free(o->shares); free(o->part);
}
int ot_put_blob(void *pair, const void *buf, size_t len) {
    ot_pair *o = pair;
    return send_blob(o->self, o->peer, buf, len);
}

/* ---------------------------------------------------------------- the per-pair mode */
static void column_of(const int64_t *Xq, const int64_t *yq, size_t n, size_t d, size_t row, uint64_t *out) {
    for (size_t k = 0; k < n; k++) out[k] = (uint64_t)(row < d ? Xq[k * d + row] : yq[k]);
}

/* batch k: pairs [k per, ...), this party's column of each gathered into vals, their words to shares + k per */
static int pp_prepare(void *pair, size_t k) {
    ot_pair *o = pair;
    for (size_t q = 0, nb = ot_pair_batch(o, k); q < nb; q++) column_of(o->Xq, o->yq, o->n, o->d, o->cols[k * o->per + q], o->vals + q * o->n);
    return 0;
}
static int pp_start(void *pair, size_t k, void *u) {
    ot_pair *o = pair;
    return lgc_said(lgc_ot_gilboa_recv_start(o->R, o->vals, ot_pair_batch(o, k), o->n, o->w1, u));
}
static int pp_send(void *pair, size_t k, const void *u, void *y) {
    ot_pair *o = pair;
    return lgc_said(lgc_ot_gilboa_send(o->S, o->vals, ot_pair_batch(o, k), o->n, o->w1, u, y, o->shares + k * o->per));
}
static int pp_finish(void *pair, size_t k, const void *y) {
    ot_pair *o = pair;
    return lgc_said(lgc_ot_gilboa_recv_finish(o->R, y, o->shares + k * o->per));
}
static size_t pp_ots(const ot_pair *o, size_t k) { return ot_pair_batch(o, k) * o->n * (size_t)o->w1; }
static size_t pp_u_bytes(void *pair, size_t k) { return lgc_ot_u_bytes(pp_ots(pair, k)); }
static size_t pp_y_bytes(void *pair, size_t k) { return pp_ots(pair, k) * 8; }
static int pp_get(void *pair, void *buf, size_t len) {
    ot_pair *o = pair;
    uint64_t prefix = 0;
    const int bad = recv_blob_prefix(o->self, o->peer, buf, len, &prefix);
    if (bad) otm_hint_if_magic(prefix);
    return bad;
}
static const ot_pipe pp_pipe = {.prepare = pp_prepare, .start = pp_start, .finish = pp_finish, .send = pp_send,
                                .u_bytes = pp_u_bytes, .y_bytes = pp_y_bytes, .put = ot_put_blob, .get = pp_get};

/* OT mode with both data providers on one node (--ot_ring): u and y of the OT extension stay in HBM.  The
 * receiver owns a two-slot device ring for u, the sender one for y; each maps the other's through hipIpc
 * and only one-byte tokens cross the socket: receiver -> sender 'U' (u of the next batch is complete) and
 * 'A' (batch finished: its y slot and u slot are free again), sender -> receiver 'Y'.  Two batches in
 * flight.  Same OT transcripts as the socket path (the bytes just do not travel). */
static int ot_ring_token_send(node *self, int to, char t) { return net_send(self, to, &t, 1); }
static int ot_ring_token_recv(node *self, int from, char *t) { return net_recv(self, from, t, 1); }
static int ot_pair_ring(node *self, int peer_party, int i_am_sender, lgc_ot_sender *S, lgc_ot_receiver *R, int device,
                        const int64_t *Xq, const int64_t *yq, size_t n, size_t d, int w1,
                        const size_t *rows, size_t npairs, size_t per, uint64_t *shares) {
    const uint64_t mmax = (uint64_t)per * n * (uint64_t)w1;
    const size_t ub = lgc_ot_u_bytes(mmax), yb = (size_t)mmax * 8, vb = per * n * 8;
    const size_t nbatch = (npairs + per - 1) / per;
    void *mine = 0, *theirs = 0, *dvals = 0, *dsh = 0;
    uint8_t hmine[64], htheirs[64];
    uint64_t *vals = lgc_host_alloc(vb);
    int rc = 1;
    if (!vals) goto out;
    if (lgc_dev_alloc(device, 2 * (i_am_sender ? yb : ub), &mine, hmine) || lgc_dev_alloc(device, 2 * vb, &dvals, NULL) ||
        lgc_dev_alloc(device, per * 8 + 8, &dsh, NULL)) { fprintf(stderr, "%s\n", lgc_last_error()); goto out; }
    if (send_blob(self, peer_party, hmine, 64) || recv_blob(self, peer_party, htheirs, 64)) goto out;
    if (lgc_dev_open(device, htheirs, &theirs)) { fprintf(stderr, "%s\n", lgc_last_error()); goto out; }
    if (i_am_sender) {
        if (lgc_ot_sender_set_device_io(S, 1)) goto out;
        size_t have_u = 0, have_a = 0;
        for (size_t k = 0; k < nbatch; k++) {
            const size_t q0 = k * per, nb = npairs - q0 < per ? npairs - q0 : per;
            for (size_t q = 0; q < nb; q++) column_of(Xq, yq, n, d, rows[q0 + q], vals + q * n);
            if (lgc_dev_upload((char *)dvals + (k & 1) * vb, vals, nb * n * 8)) goto out;
            while (have_u <= k || (k >= 2 && have_a + 2 <= k)) {        /* u of batch k is there, y slot of batch k - 2 is free */
                char t = 0;
                if (ot_ring_token_recv(self, peer_party, &t)) goto out;
                if (t == 'U') have_u++; else if (t == 'A') have_a++; else goto out;
            }
            if (lgc_ot_gilboa_send(S, (const uint64_t *)((char *)dvals + (k & 1) * vb), nb, n, w1, (const uint8_t *)theirs + (k & 1) * ub,
                                   (uint64_t *)((char *)mine + (k & 1) * yb), (uint64_t *)dsh)) { fprintf(stderr, "%s\n", lgc_last_error()); goto out; }
            if (lgc_dev_download(shares + q0, dsh, nb * 8)) goto out;
            if (ot_ring_token_send(self, peer_party, 'Y')) goto out;
        }
        while (have_a < nbatch) {                                        /* the receiver is done with every y slot */
            char t = 0;
            if (ot_ring_token_recv(self, peer_party, &t)) goto out;
            if (t == 'A') have_a++; else if (t != 'U') goto out;
        }
    } else {
        if (lgc_ot_receiver_set_device_io(R, 1)) goto out;
        size_t started = 0;
        for (size_t k = 0; k < nbatch + 2; k++) {
            if (k >= 2) {                                                /* finish batch k - 2 */
                const size_t f = k - 2, q0 = f * per, nb = npairs - q0 < per ? npairs - q0 : per;
                char t = 0;
                if (ot_ring_token_recv(self, peer_party, &t) || t != 'Y') goto out;
                if (lgc_ot_gilboa_recv_finish(R, (const uint64_t *)((char *)theirs + (f & 1) * yb), (uint64_t *)dsh)) { fprintf(stderr, "%s\n", lgc_last_error()); goto out; }
                if (lgc_dev_download(shares + q0, dsh, nb * 8)) goto out;
                    if (ot_ring_token_send(self, peer_party, 'A')) goto out;
            }
            if (started < nbatch) {                                      /* start the next batch: its slots are free now */
                const size_t q0 = started * per, nb = npairs - q0 < per ? npairs - q0 : per;
                for (size_t q = 0; q < nb; q++) column_of(Xq, yq, n, d, rows[q0 + q], vals + q * n);
                if (lgc_dev_upload((char *)dvals + (started & 1) * vb, vals, nb * n * 8)) goto out;
                if (lgc_ot_gilboa_recv_start(R, (const uint64_t *)((char *)dvals + (started & 1) * vb), nb, n, w1,
                                             (uint8_t *)mine + (started & 1) * ub)) { fprintf(stderr, "%s\n", lgc_last_error()); goto out; }
                if (ot_ring_token_send(self, peer_party, 'U')) goto out;
                started++;
            }
        }
    }
    rc = 0;
out:
    if (theirs) lgc_dev_close(theirs);
    lgc_dev_free(mine); lgc_dev_free(dvals); lgc_dev_free(dsh);
    lgc_host_free(vals);
    return rc;
}

/* One provider pair: the sender's columns [i0, i1) and the receiver's [j0, j1), each with y (row d) where that side is the last
 * provider.  One scalar product per pair of columns; its share is added where that pair lives in share_A / share_b. */
static int run_pair_columns(ot_pair *o, int ring, size_t M, size_t i0, size_t i1, int y_on_sender, size_t j0, size_t j1, int y_on_receiver,
                            uint64_t *share_A, uint64_t *share_b) {
    const size_t n = o->n, d = o->d;
    /* rows of the sender / receiver per pair (and with them where the share goes), in the block order both sides derive */
    size_t *ri = NULL, *rj = NULL, q;
    const size_t npairs = p1_plan_ot(d, M, i0, i1, y_on_sender, j0, j1, y_on_receiver, &ri, &rj);
    if (!npairs) return 0;                                                   /* (both sides count alike) */
    int rc = 1;
    check(npairs != (size_t)-1, "out of memory");
    o->shares = malloc(npairs * 8);
    check(o->shares != NULL, "out of memory");
    const size_t per = p1_ot_batch_pairs(n, o->w1, npairs);
    const uint64_t mmax = (uint64_t)per * n * (uint64_t)o->w1;
    o->cols = o->i_am_sender ? ri : rj; o->total = npairs; o->per = per;
    if (ot_pair_open(o)) goto error;
    check(!(ring ? ot_pair_ring(o->self, o->peer, o->i_am_sender, o->S, o->R, o->device, o->Xq, o->yq, n, d, o->w1, o->cols, npairs, per, o->shares)
                 : ot_pair_run(o, &pp_pipe, per * n * 8, lgc_ot_u_bytes(mmax), mmax * 8)), "OT-mode aggregation failed");
    for (q = 0; q < npairs; q++) {
        if (ri[q] < d && rj[q] < d) share_A[idx(ri[q], rj[q])] += o->shares[q];
        else share_b[ri[q] < d ? ri[q] : rj[q]] += o->shares[q];
    }
    rc = 0;
error:
    ot_pair_close(o);
    free(ri); free(rj);
    return rc;
}

/* one Gilboa exchange per peer, peers in a global order */
int run_party_ot(node *self, config *c, int device, size_t n, const int64_t *Xq, const int64_t *yq, int w1, const p1_mode *mode,
                 uint64_t *share_A, uint64_t *share_b) {
    const size_t d = c->d;
    const int me = c->party - 1, last = c->num_parties - 1;
    const int matrix = mode->transport == P1_OT_MATRIX || mode->transport == P1_OT_HALF;
    for (int lo = 2; lo < c->num_parties; lo++)
        for (int hi = lo + 1; hi < c->num_parties; hi++) {
            if (me != lo && me != hi) continue;
            int peer = me == lo ? hi : lo;
            int i_am_sender = p1_ot_i_am_sender(me, peer);
            int pi = i_am_sender ? me : peer, pj = i_am_sender ? peer : me;
            size_t i0 = (size_t)c->index_owned[pi], i1 = pi < last ? (size_t)c->index_owned[pi + 1] : d;
            size_t j0 = (size_t)c->index_owned[pj], j1 = pj < last ? (size_t)c->index_owned[pj + 1] : d;
            ot_pair o = {.self = self, .peer = peer + 1, .i_am_sender = i_am_sender, .device = device, .Xq = Xq, .yq = yq, .n = n, .d = d, .w1 = w1};
            if (!matrix) { if (run_pair_columns(&o, mode->transport == P1_OT_RING, mode->scan, i0, i1, pi == last, j0, j1, pj == last, share_A, share_b)) return 1; }
            else if (run_party_ot_matrix_pair(&o, mode->transport == P1_OT_HALF, i0, i1, pi == last, j0, j1, pj == last, share_A, share_b)) { fprintf(stderr, "OT-mode aggregation failed\n"); return 1; }
        }
    return 0;
}
