/* phase1_ot_matrix.c -- the OT mode of phase 1 with one vector OT per bit of the receiver's operand (--use_ot --ot_matrix;
 * include/linreg_gc_ot_matrix.h): the block between two data providers is one Gilboa product X_r^T X_s, not one scalar product
 * per pair of columns.  The sender rule and the base OTs are the per-pair mode's (phase1_party.c).  Per provider pair:
 *   both      after the base OTs, OTM_MAGIC (8 bytes) each way: a peer in another mode is refused, not waited for
 *   receiver  gathers its columns (with y if it is the last provider) into dense row-major batches of whole rows
 *             (otm_batch_rows, which both sides call); per batch a blob u one way, a blob y back
 *   sender    gathers its columns alike; its share block and the receiver's are summed over the batches and scattered
 * Two batches are in flight: on the receiver a helper thread extends batch k + 1 and sends its u while the main thread waits for
 * y of batch k; on the sender u arrives on one helper thread and y leaves on another while the main thread runs the kernels. */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/linreg_gc.h"
#include "../../include/linreg_gc_ot_matrix.h"
#include "baseot.h"
#include "config.h"
#include "net.h"
#include "ot_matrix_plan.h"
#include "protocol.h"
#include "protocol_int.h"

int g_ot_matrix = 0;
void protocol_set_ot_matrix(int on) { g_ot_matrix = on; }

void otm_hint_if_magic(uint64_t prefix) {
    if (prefix == OTM_MAGIC) fprintf(stderr, "the peer runs --ot_matrix (this party was started without it): run every party in the same mode\n");
}

typedef struct {
    node *self; int peer;                       /* peer: 1-based party number */
    lgc_ot_receiver *R;
    const int64_t *Xq, *yq; size_t n, d; int w;
    const size_t *cols; size_t ncols, other;    /* the own columns (d: y) and how many the peer holds */
    size_t per, nbatch;
    uint8_t *u[2]; void *y[2];                  /* sender: two of each; receiver: u[0], y[0] */
    size_t started, finished, recvd, gpu_done, sent;
    int failed;
    pthread_mutex_t mu;
    pthread_cond_t cv;
} otm_ctx;

static size_t batch_rows(const otm_ctx *c, size_t k) { return c->n - k * c->per < c->per ? c->n - k * c->per : c->per; }
static void gather(const otm_ctx *c, size_t row0, size_t rows, uint64_t *out) {
    for (size_t k = 0; k < rows; k++)
        for (size_t q = 0; q < c->ncols; q++)
            out[k * c->ncols + q] = (uint64_t)(c->cols[q] < c->d ? c->Xq[(row0 + k) * c->d + c->cols[q]] : c->yq[row0 + k]);
}
static void mark(otm_ctx *c, size_t *field, size_t value, int bad) {
    pthread_mutex_lock(&c->mu);
    if (bad) c->failed = 1; else if (field) *field = value;
    pthread_cond_broadcast(&c->cv);
    pthread_mutex_unlock(&c->mu);
}

/* receiver, helper thread: starts batches and sends their u; at most two ahead of the finishing thread */
static void *recv_starter(void *arg) {
    otm_ctx *c = arg;
    uint64_t *vals = lgc_host_alloc(c->per * c->ncols * 8);
    int bad = !vals;
    for (size_t k = 0; k < c->nbatch && !bad; k++) {
        const size_t rows = batch_rows(c, k);
        pthread_mutex_lock(&c->mu);
        while (k >= c->finished + 2 && !c->failed) pthread_cond_wait(&c->cv, &c->mu);
        bad = c->failed;
        pthread_mutex_unlock(&c->mu);
        if (bad) break;
        gather(c, k * c->per, rows, vals);
        if (lgc_ot_gilboa_matrix_recv_start(c->R, vals, rows, c->ncols, c->other, c->w, c->u[0])) { fprintf(stderr, "%s\n", lgc_last_error()); bad = 1; }
        else if (send_blob(c->self, c->peer, c->u[0], lgc_ot_u_bytes((uint64_t)rows * c->ncols * (uint64_t)c->w))) { fprintf(stderr, "OT: could not send u\n"); bad = 1; }
        mark(c, &c->started, k + 1, bad);
    }
    if (bad) mark(c, NULL, 0, 1);
    lgc_host_free(vals);
    return NULL;
}
/* sender, helper threads: u in, y out */
static void *send_recv_u(void *arg) {
    otm_ctx *c = arg;
    for (size_t k = 0; k < c->nbatch; k++) {
        pthread_mutex_lock(&c->mu);
        while (k >= c->gpu_done + 2 && !c->failed) pthread_cond_wait(&c->cv, &c->mu);
        int bad = c->failed;
        pthread_mutex_unlock(&c->mu);
        if (bad) break;
        bad = recv_blob(c->self, c->peer, c->u[k & 1], lgc_ot_u_bytes((uint64_t)batch_rows(c, k) * c->other * (uint64_t)c->w));
        if (bad) fprintf(stderr, "OT: could not receive u\n");
        mark(c, &c->recvd, k + 1, bad);
        if (bad) break;
    }
    return NULL;
}
static void *send_send_y(void *arg) {
    otm_ctx *c = arg;
    for (size_t k = 0; k < c->nbatch; k++) {
        pthread_mutex_lock(&c->mu);
        while (c->gpu_done <= k && !c->failed) pthread_cond_wait(&c->cv, &c->mu);
        int bad = c->failed;
        pthread_mutex_unlock(&c->mu);
        if (bad) break;
        bad = send_blob(c->self, c->peer, c->y[k & 1], lgc_ot_gilboa_matrix_y_bytes(batch_rows(c, k), c->other, c->ncols, c->w));
        if (bad) fprintf(stderr, "OT: could not send y\n");
        mark(c, &c->sent, k + 1, bad);
        if (bad) break;
    }
    return NULL;
}

/* One provider pair.  cols_s / cols_r: the sender's and the receiver's columns, d standing for y.  blk_dst[ir * s + j] is where
 * the word of (receiver column ir, sender column j) is added. */
int run_party_ot_matrix_pair(node *self, int peer, int i_am_sender, int device, const int64_t *Xq, const int64_t *yq, size_t n, size_t d,
                             int w1, const size_t *cols_s, size_t s, const size_t *cols_r, size_t r, uint64_t **blk_dst) {
    lgc_ot_sender *S = 0;
    lgc_ot_receiver *R = 0;
    uint64_t *blk = calloc(r * s, 8), *part = malloc(r * s * 8), *vals = 0;
    otm_ctx c;
    int rc = 1, inited = 0;
    memset(&c, 0, sizeof c);
    check(blk && part, "out of memory");
    if (i_am_sender) {
        uint8_t delta[16], seeds[128][16];
        check(!baseot_ext_sender(self, peer, delta, seeds), "base OT failed");
        LGC(lgc_ot_sender_create(&S, device, delta, seeds));
    } else {
        uint8_t s0[128][16], s1[128][16];
        check(!baseot_ext_receiver(self, peer, s0, s1), "base OT failed");
        LGC(lgc_ot_receiver_create(&R, device, s0, s1));
    }
    uint64_t magic = OTM_MAGIC, theirs = 0;
    check(!net_send(self, peer, &magic, sizeof magic), "Could not send to party %d", peer);
    check(!net_recv(self, peer, &theirs, sizeof theirs) && theirs == OTM_MAGIC,
          "party %d does not speak --ot_matrix (this party was started with it): run every party in the same mode", peer);
    c.self = self; c.peer = peer; c.R = R; c.Xq = Xq; c.yq = yq; c.n = n; c.d = d; c.w = w1;
    c.cols = i_am_sender ? cols_s : cols_r; c.ncols = i_am_sender ? s : r; c.other = i_am_sender ? r : s;
    c.per = otm_batch_rows(r, s, w1);
    if (c.per > n) c.per = n;
    c.nbatch = (n + c.per - 1) / c.per;
    const size_t ub = lgc_ot_u_bytes((uint64_t)c.per * r * (uint64_t)w1), yb = lgc_ot_gilboa_matrix_y_bytes(c.per, r, s, w1);
    for (int k = 0; k < (i_am_sender ? 2 : 1); k++) {
        c.u[k] = lgc_host_alloc(ub); c.y[k] = lgc_host_alloc(yb);
        check(c.u[k] && c.y[k], "%s", lgc_last_error());
    }
    pthread_mutex_init(&c.mu, NULL); pthread_cond_init(&c.cv, NULL);
    inited = 1;
    int bad = 0;
    if (i_am_sender) {
        vals = lgc_host_alloc(c.per * s * 8);
        check(vals != NULL, "%s", lgc_last_error());
        pthread_t tin, tout;
        check(!pthread_create(&tin, NULL, send_recv_u, &c), "pthread_create failed");
        if (pthread_create(&tout, NULL, send_send_y, &c)) { mark(&c, NULL, 0, 1); pthread_join(tin, NULL); check(0, "pthread_create failed"); }
        for (size_t k = 0; k < c.nbatch && !bad; k++) {
            const size_t rows = batch_rows(&c, k);
            gather(&c, k * c.per, rows, vals);
            pthread_mutex_lock(&c.mu);                  /* u of batch k is here, and the y buffer it will fill is free */
            while ((c.recvd <= k || k >= c.sent + 2) && !c.failed) pthread_cond_wait(&c.cv, &c.mu);
            bad = c.failed;
            pthread_mutex_unlock(&c.mu);
            if (bad) break;
            if (lgc_ot_gilboa_matrix_send(S, vals, rows, r, s, w1, c.u[k & 1], c.y[k & 1], part)) { fprintf(stderr, "%s\n", lgc_last_error()); bad = 1; }
            else for (size_t q = 0; q < r * s; q++) blk[q] += part[q];
            mark(&c, &c.gpu_done, k + 1, bad);
        }
        if (bad) mark(&c, NULL, 0, 1);
        pthread_join(tin, NULL); pthread_join(tout, NULL);
    } else {
        pthread_t th;
        check(!pthread_create(&th, NULL, recv_starter, &c), "pthread_create failed");
        for (size_t k = 0; k < c.nbatch && !bad; k++) {
            const size_t rows = batch_rows(&c, k);
            pthread_mutex_lock(&c.mu);
            while (c.started <= k && !c.failed) pthread_cond_wait(&c.cv, &c.mu);
            bad = c.failed;
            pthread_mutex_unlock(&c.mu);
            if (bad) break;
            if (recv_blob(self, peer, c.y[0], lgc_ot_gilboa_matrix_y_bytes(rows, r, s, w1))) { fprintf(stderr, "OT: could not receive y\n"); bad = 1; }
            else if (lgc_ot_gilboa_matrix_recv_finish(R, c.y[0], part)) { fprintf(stderr, "%s\n", lgc_last_error()); bad = 1; }
            else for (size_t q = 0; q < r * s; q++) blk[q] += part[q];
            mark(&c, &c.finished, k + 1, bad);
        }
        if (bad) mark(&c, NULL, 0, 1);
        pthread_join(th, NULL);
    }
    check(!bad && !c.failed, "OT-mode aggregation (matrix) failed");
    for (size_t q = 0; q < r * s; q++) *blk_dst[q] += blk[q];
    rc = 0;
error:
    if (inited) { pthread_mutex_destroy(&c.mu); pthread_cond_destroy(&c.cv); }
    if (S) lgc_ot_sender_destroy(S);
    if (R) lgc_ot_receiver_destroy(R);
    for (int k = 0; k < 2; k++) { lgc_host_free(c.u[k]); lgc_host_free(c.y[k]); }
    lgc_host_free(vals);
    free(blk); free(part);
    return rc;
}
