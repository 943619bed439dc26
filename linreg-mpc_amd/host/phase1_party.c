/* phase1_party.c -- phase 1, data-provider side (run_party, src/phase1.c:453-656): TI mode over sockets with per-peer workers,
 * the 64 -> 32 bit conversion of the shares; the OT mode is phase1_ot.c's.  Split from protocol.c in round 4. */
#define _GNU_SOURCE
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <sys/mman.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "../../include/linreg_gc.h"
#include "../../include/linreg_gc_folds.h"
#include "../../include/linreg_gc_folds_yy.h"
#include "../../include/linreg_gc_inference.h"
#include "../../include/linreg_gc_scan.h"
#include "config.h"
#include "net.h"
#include "pmsg.h"
#include "protocol.h"
#include "protocol_int.h"

/* ---------------------------------------------------------------- phase 1: data provider */
/* TI-mode plumbing: a bounded queue of TI messages per peer, and the per-peer worker */
typedef struct { uint8_t *raw; size_t len; uint64_t val; } ti_item;   /* raw: undecoded message (decoded by the worker) */
typedef struct {
    ti_item *items;
    size_t cap, head, count;
    int closed;                 /* no more pushes (reader done) or no more pops (worker failed) */
    pthread_mutex_t mu;
    pthread_cond_t cv;
} ti_queue;
static void ti_queue_init(ti_queue *q, size_t cap) {
    q->items = calloc(cap, sizeof *q->items); q->cap = cap; q->head = q->count = 0; q->closed = 0;
    pthread_mutex_init(&q->mu, NULL); pthread_cond_init(&q->cv, NULL);
}
static void ti_queue_destroy(ti_queue *q) {
    for (size_t i = 0; i < q->count; i++) free(q->items[(q->head + i) % q->cap].raw);
    free(q->items); pthread_mutex_destroy(&q->mu); pthread_cond_destroy(&q->cv);
}
static void ti_queue_close(ti_queue *q) {
    pthread_mutex_lock(&q->mu); q->closed = 1; pthread_cond_broadcast(&q->cv); pthread_mutex_unlock(&q->mu);
}
static int ti_queue_push(ti_queue *q, ti_item it) {
    pthread_mutex_lock(&q->mu);
    while (q->count == q->cap && !q->closed) pthread_cond_wait(&q->cv, &q->mu);
    if (q->closed) { pthread_mutex_unlock(&q->mu); return 1; }
    q->items[(q->head + q->count++) % q->cap] = it;
    pthread_cond_broadcast(&q->cv);
    pthread_mutex_unlock(&q->mu);
    return 0;
}
/* wait: block until an item or the close; else 1 at once when the queue is empty right now */
static int ti_queue_pop(ti_queue *q, ti_item *it, int wait) {
    pthread_mutex_lock(&q->mu);
    while (wait && q->count == 0 && !q->closed) pthread_cond_wait(&q->cv, &q->mu);
    if (q->count == 0) { pthread_mutex_unlock(&q->mu); return 1; }
    *it = q->items[q->head]; q->head = (q->head + 1) % q->cap; q->count--;
    pthread_cond_broadcast(&q->cv);
    pthread_mutex_unlock(&q->mu);
    return 0;
}
/* a provider's view of one of its pairs (phase1_plan.h) and where the pair's share goes */
typedef struct { p1_view v; uint64_t *dst; } ti_pair;
typedef struct {
    node *self; lgc_p1 *p1; size_t n; int peer;
    const ti_pair *pairs; size_t npairs;
    ti_queue *q;
    int failed;
} ti_worker;
static double now_s(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }
/* one message from a peer data provider, decoded straight into `dst` (n words, page-locked); raw / rawcap:
 * the caller's reusable receive buffer.  Timed like the reference's wait_total. */
static int recv_pmsg_into_timed(node *self, int from, uint8_t **raw, size_t *rawcap, uint64_t *dst, size_t n, uint64_t *value) {
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    size_t sz = 0, got = 0;
    int rc = net_recv(self, from, &sz, sizeof sz) || sz > g_pmsg_limit;
    if (!rc && sz > *rawcap) { free(*raw); *raw = malloc(sz + sz / 8); *rawcap = *raw ? sz + sz / 8 : 0; rc = !*raw; }
    if (!rc) rc = net_recv(self, from, *raw, sz);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    self->wait_ns[from - 1] += (uint64_t)((t1.tv_sec - t0.tv_sec) * 1000000000ll + (t1.tv_nsec - t0.tv_nsec));
    if (!rc) rc = pmsg_unpack_into(*raw, sz, dst, n, &got, value) || got != n;
    return rc;
}
/* The per-peer workers batch: a run of pairs with one peer is one device call (lgc_p1_mask / lgc_p1_dot /
 * lgc_p1_ti_a_batch over up to kTiBatch pairs) on page-locked buffers the messages are decoded into, instead
 * of one call per pair from pageable memory.  A batch is whatever has arrived (at least one pair), so
 * nothing waits for a batch to fill.  Same bytes, same order on every socket. */
enum { kTiBatch = 16, kTiSlots = 32 };

/* Party b of a run of pairs with one peer, pipelined.  b's first message (b + x) depends only on
 * the TI's message, so this thread sends the masks of successive pairs back to back, while a second
 * thread receives party a's replies and finishes the shares (<a - y, b> - r): party b then never
 * idles for a round trip, and party a always finds its next input waiting. */
typedef struct {
    ti_worker *w;
    const ti_pair **pr;        /* this worker's pairs, in order */
    uint64_t *r;               /* the TI's r of each pair (filled by the sender side) */
    size_t total;
    size_t sent;               /* pairs whose mask has been sent (published under mu) */
    int stop;
    pthread_mutex_t mu;
    pthread_cond_t cv;
} ti_b_pipe;
static void *ti_b_finisher(void *arg) {
    ti_b_pipe *bp = arg;
    ti_worker *w = bp->w;
    const size_t n = w->n;
    const int to = w->peer + 1;
    uint64_t *in = lgc_host_alloc(kTiBatch * n * 8);
    uint8_t *raw = NULL; size_t rawcap = 0;
    uint32_t cols[kTiBatch]; uint64_t shares[kTiBatch];
    if (!in) w->failed = 1;
    for (size_t k = 0; k < bp->total && !w->failed;) {
        pthread_mutex_lock(&bp->mu);
        while (bp->sent <= k && !bp->stop) pthread_cond_wait(&bp->cv, &bp->mu);
        size_t avail = bp->sent - k;
        pthread_mutex_unlock(&bp->mu);
        if (!avail) break;
        size_t nb = avail < kTiBatch ? avail : kTiBatch;
        for (size_t i = 0; i < nb && !w->failed; i++) {
            uint64_t inval = 0;
            cols[i] = bp->pr[k + i]->v.col;
            if (recv_pmsg_into_timed(w->self, to, &raw, &rawcap, in + i * n, n, &inval)) { fprintf(stderr, "Could not receive message from party A (%d)\n", w->peer); w->failed = 1; }
        }
        if (w->failed) break;
        if (lgc_p1_dot(w->p1, in, 0, cols, nb, bp->r + k, shares)) { fprintf(stderr, "%s\n", lgc_last_error()); w->failed = 1; break; }   /* <a-y, b> - r */
        for (size_t i = 0; i < nb; i++) *bp->pr[k + i]->dst = shares[i];
        k += nb;
    }
    free(raw); lgc_host_free(in);
    return NULL;
}
static int ti_worker_b_pipelined(ti_worker *w, const ti_pair **mine, size_t total) {
    const size_t n = w->n;
    const int to = w->peer + 1;
    ti_b_pipe bp;
    memset(&bp, 0, sizeof bp);
    bp.w = w; bp.pr = mine; bp.total = total;
    bp.r = malloc((total + 1) * sizeof *bp.r);
    uint64_t *x = lgc_host_alloc(kTiBatch * n * 8), *m = lgc_host_alloc(kTiBatch * n * 8);
    uint32_t cols[kTiBatch];
    pthread_mutex_init(&bp.mu, NULL); pthread_cond_init(&bp.cv, NULL);
    pthread_t fin;
    int have_fin = bp.r && x && m && !pthread_create(&fin, NULL, ti_b_finisher, &bp);
    if (!have_fin) w->failed = 1;
    for (size_t k = 0; k < total && !w->failed;) {
        size_t nb = 0;
        while (nb < kTiBatch && k + nb < total) {
            ti_item it = {0, 0, 0};
            size_t ti_n = 0;
            if (ti_queue_pop(w->q, &it, nb == 0)) { if (nb == 0) w->failed = 1; break; }
            if (pmsg_unpack_into(it.raw, it.len, x + nb * n, n, &ti_n, &it.val) || ti_n != n) { fprintf(stderr, "Could not decode message from TI\n"); w->failed = 1; }
            free(it.raw);
            if (w->failed) break;
            cols[nb] = mine[k + nb]->v.col;
            bp.r[k + nb] = it.val;
            nb++;
        }
        if (w->failed || !nb) break;
        if (lgc_p1_mask(w->p1, cols, nb, x, +1, m)) { fprintf(stderr, "%s\n", lgc_last_error()); w->failed = 1; break; }        /* b + x */
        for (size_t i = 0; i < nb && !w->failed; i++)
            if (send_pmsg(w->self, to, m + i * n, n, 0)) { fprintf(stderr, "Could not send message to party A (%d)\n", w->peer); w->failed = 1; }
        if (w->failed) break;
        k += nb;
        pthread_mutex_lock(&bp.mu); bp.sent = k; pthread_cond_broadcast(&bp.cv); pthread_mutex_unlock(&bp.mu);
    }
    pthread_mutex_lock(&bp.mu); bp.stop = 1; pthread_cond_broadcast(&bp.cv); pthread_mutex_unlock(&bp.mu);
    if (have_fin) pthread_join(fin, NULL);
    pthread_mutex_destroy(&bp.mu); pthread_cond_destroy(&bp.cv);
    free(bp.r); lgc_host_free(x); lgc_host_free(m);
    return w->failed;
}

/* Party a of a run of pairs with one peer, as two stages: a prefetch thread takes the TI's message
 * and party b's message off the queue / socket and decodes both into a ring of page-locked slots, while
 * this thread runs the fused device step over the slots that are ready and sends the replies. */
typedef struct {
    ti_worker *w;
    size_t total;
    uint64_t *y, *in;          /* kTiSlots x n words each, page-locked */
    uint64_t sub[kTiSlots];
    size_t produced, consumed;
    int stop;
    pthread_mutex_t mu;
    pthread_cond_t cv;
} ti_a_pipe;
static void *ti_a_prefetch(void *arg) {
    ti_a_pipe *ap = arg;
    ti_worker *w = ap->w;
    const size_t n = w->n;
    const int to = w->peer + 1;
    uint8_t *raw = NULL; size_t rawcap = 0;
    for (size_t k = 0; k < ap->total; k++) {
        pthread_mutex_lock(&ap->mu);
        while (ap->produced - ap->consumed == kTiSlots && !ap->stop) pthread_cond_wait(&ap->cv, &ap->mu);
        int stop = ap->stop;
        pthread_mutex_unlock(&ap->mu);
        if (stop) break;
        const size_t slot = k % kTiSlots;
        ti_item it = {0, 0, 0};
        size_t ti_n = 0;
        uint64_t inval = 0;
        int bad = 0;
        if (ti_queue_pop(w->q, &it, 1)) bad = 1;
        else if (pmsg_unpack_into(it.raw, it.len, ap->y + slot * n, n, &ti_n, &it.val) || ti_n != n) { fprintf(stderr, "Could not decode message from TI\n"); bad = 1; }
        else if (recv_pmsg_into_timed(w->self, to, &raw, &rawcap, ap->in + slot * n, n, &inval)) { fprintf(stderr, "Could not receive message from party B (%d)\n", w->peer); bad = 1; }
        free(it.raw);
        pthread_mutex_lock(&ap->mu);
        if (bad) { ap->stop = 1; w->failed = 1; }
        else { ap->sub[slot] = it.val; ap->produced++; }
        pthread_cond_broadcast(&ap->cv);
        pthread_mutex_unlock(&ap->mu);
        if (bad) break;
    }
    free(raw);
    return NULL;
}
static int ti_worker_a_pipelined(ti_worker *w, const ti_pair **mine, size_t total) {
    const size_t n = w->n;
    const int to = w->peer + 1;
    ti_a_pipe ap;
    memset(&ap, 0, sizeof ap);
    ap.w = w; ap.total = total;
    ap.y = lgc_host_alloc((size_t)kTiSlots * n * 8); ap.in = lgc_host_alloc((size_t)kTiSlots * n * 8);
    uint64_t *out = lgc_host_alloc((size_t)kTiBatch * n * 8);
    uint32_t cols[kTiBatch]; uint64_t shares[kTiBatch], sub[kTiBatch];
    pthread_mutex_init(&ap.mu, NULL); pthread_cond_init(&ap.cv, NULL);
    pthread_t pre;
    int have = ap.y && ap.in && out && !pthread_create(&pre, NULL, ti_a_prefetch, &ap);
    if (!have) w->failed = 1;
    for (size_t k = 0; k < total && !w->failed;) {
        pthread_mutex_lock(&ap.mu);
        while (ap.produced == ap.consumed && !ap.stop) pthread_cond_wait(&ap.cv, &ap.mu);
        size_t avail = ap.produced - ap.consumed;
        pthread_mutex_unlock(&ap.mu);
        if (!avail) { w->failed = 1; break; }
        const size_t slot = k % kTiSlots;
        size_t nb = avail < kTiBatch ? avail : kTiBatch;
        if (nb > kTiSlots - slot) nb = kTiSlots - slot;          /* a batch is contiguous in the ring */
        for (size_t i = 0; i < nb; i++) { cols[i] = mine[k + i]->v.col; sub[i] = ap.sub[slot + i]; }
        /* a - y and <b+x, y> - (xy - r) for the whole batch */
        if (lgc_p1_ti_a_batch(w->p1, cols, nb, ap.y + slot * n, ap.in + slot * n, sub, out, shares)) { fprintf(stderr, "%s\n", lgc_last_error()); w->failed = 1; break; }
        for (size_t i = 0; i < nb && !w->failed; i++)
            if (send_pmsg(w->self, to, out + i * n, n, 0)) { fprintf(stderr, "Could not send message to party B (%d)\n", w->peer); w->failed = 1; }
        if (w->failed) break;
        for (size_t i = 0; i < nb; i++) *mine[k + i]->dst = shares[i];
        k += nb;
        pthread_mutex_lock(&ap.mu); ap.consumed = k; pthread_cond_broadcast(&ap.cv); pthread_mutex_unlock(&ap.mu);
    }
    pthread_mutex_lock(&ap.mu); ap.stop = 1; pthread_cond_broadcast(&ap.cv); pthread_mutex_unlock(&ap.mu);
    if (w->failed) ti_queue_close(w->q);                         /* the prefetch thread may be blocked in a pop */
    if (have) pthread_join(pre, NULL);
    pthread_mutex_destroy(&ap.mu); pthread_cond_destroy(&ap.cv);
    lgc_host_free(ap.y); lgc_host_free(ap.in); lgc_host_free(out);
    return w->failed;
}

/* The role towards one peer is fixed by the column ownership (the party with the later columns is party a of every pair they
 * share: phase1_plan.h), so a worker runs the pipelined form of its one role. */
static void *ti_worker_main(void *arg) {
    ti_worker *w = arg;
    const ti_pair **mine = malloc(w->npairs * sizeof *mine);
    size_t cnt = 0, as_a = 0;
    for (size_t k = 0; mine && k < w->npairs; k++) if (w->pairs[k].v.peer == w->peer) { mine[cnt++] = &w->pairs[k]; as_a += w->pairs[k].v.is_a != 0; }
    if (!mine) { fprintf(stderr, "out of memory\n"); w->failed = 1; }
    else if (as_a && as_a != cnt) {
        fprintf(stderr, "phase 1: party a of %zu and party b of %zu pairs with party %d, where the pair plan promises one role per peer\n", as_a, cnt - as_a, w->peer + 1);
        w->failed = 1;
    } else if (as_a) ti_worker_a_pipelined(w, mine, cnt);
    else ti_worker_b_pipelined(w, mine, cnt);
    free(mine);
    if (w->failed) ti_queue_close(w->q);                  /* unblock the reader */
    return NULL;
}

/* The cross-party part of phase 1 for n rows -- all rows, or one row fold behind lgc_p1_set_rows: Xq / yq point at the first
 * of them, p1's window holds exactly them, share_A / share_b already hold this party's local block for them. */
static int party_cross(node *self, config *c, lgc_p1 *p1, const p1_job *job, size_t n, const int64_t *Xq, const int64_t *yq,
                       uint64_t *share_A, uint64_t *share_b, double t_start) {
    const size_t d = c->d, T = d * (d + 1) / 2;
    const int me = c->party - 1, w1 = job->w1;
    const int timing = getenv("LINREG_TIMING") != NULL;
    switch (job->mode.transport) {
    case P1_TI_MATRIX:      /* one matrix triple per peer (include/linreg_gc_p1_matrix.h) */
        check(!run_party_ti_matrix(self, c, p1, n, w1, share_A, share_b), "TI-mode aggregation (matrix triples) failed");
        if (timing) fprintf(stderr, "party %d: TI-mode aggregation (matrix triples) done after %.2fs\n", c->party, wall_clock() - t_start);
        break;
    case P1_TI_RING:
        check(!run_party_ti_ring(self, c, p1, job->device, share_A, share_b), "TI-mode aggregation (device rings) failed");
        if (timing) fprintf(stderr, "party %d: TI-mode aggregation (rings) done after %.2fs\n", c->party, wall_clock() - t_start);
        break;
    case P1_TI_SOCKETS: {
        /* TI mode.  The pairs are those of the loops at src/phase1.c:534-586 and every socket
         * carries its messages in that order (the TI socket: this party's pairs in loop order; a
         * peer socket: the pairs shared with that peer in loop order), so the byte streams are the
         * reference's.  Pairs with different peers are independent: one worker thread per peer runs
         * inner_product_ti for its pairs, fed by a reader thread that takes the TI messages off the
         * TI socket in loop order and hands each to the worker of the pair's peer. */
        const int np_all = c->num_parties;
        p1_pair *plan = NULL;
        const size_t nplan = p1_plan_of(c, job->mode.scan, &plan);
        check(nplan != (size_t)-1, "out of memory");
        ti_pair *pairs = malloc((nplan + 1) * sizeof *pairs);      /* this party's pairs of the plan, in its order */
        size_t npairs = 0;
        for (size_t q = 0; pairs && q < nplan; q++)
            if (p1_pair_view(&plan[q], me, &pairs[npairs].v)) {
                pairs[npairs].dst = plan[q].ci < d ? share_A + idx(plan[q].ci, plan[q].cj) : share_b + plan[q].cj;
                npairs++;
            }
        free(plan);
        /* The TI socket delivers this party's messages in loop order, i.e. in runs of consecutive pairs with
         * the SAME peer (a whole row against one peer's columns).  The queues must hold more than such a
         * run, or the reader blocks on one worker's full queue while the other workers starve. */
        size_t qcap = ((size_t)256 << 20) / (n * 8 + 64);
        if (qcap < 64) qcap = 64;
        if (qcap > 4096) qcap = 4096;
        ti_queue *queues = calloc((size_t)np_all, sizeof *queues);
        ti_worker *workers = calloc((size_t)np_all, sizeof *workers);
        pthread_t *tids = calloc((size_t)np_all, sizeof *tids);
        int started[64] = {0}, failed = !pairs || !queues || !workers || !tids;
        check(np_all <= 64, "too many parties");
        for (int k = 2; k < np_all && !failed; k++) {
            if (k == me) continue;
            size_t cnt = 0;
            for (size_t q = 0; q < npairs; q++) cnt += pairs[q].v.peer == k;
            if (!cnt) continue;
            ti_queue_init(&queues[k], qcap);
            ti_worker w = {self, p1, n, k, pairs, npairs, &queues[k], 0};
            workers[k] = w;
            if (pthread_create(&tids[k], NULL, ti_worker_main, &workers[k])) { failed = 1; break; }
            started[k] = 1;
        }
        /* reader: this thread */
        double rd_hdr = 0, rd_body = 0, rd_push = 0;
        for (size_t q = 0; q < npairs && !failed; q++) {
            ti_item it = {0, 0, 0};
            size_t sz = 0;
            double r0 = timing ? now_s() : 0, r1 = 0, r2 = 0;
            int bad = net_recv(self, 1, &sz, sizeof sz) || sz > g_pmsg_limit;
            if (timing) r1 = now_s();
            bad = bad || !(it.raw = malloc(sz ? sz : 1)) || net_recv(self, 1, it.raw, sz);
            if (timing) r2 = now_s();
            if (bad) { fprintf(stderr, "Could not receive message from TI\n"); failed = 1; free(it.raw); break; }
            it.len = sz;
            if (ti_queue_push(&queues[pairs[q].v.peer], it)) { failed = 1; free(it.raw); break; }   /* the worker gave up */
            if (timing) { rd_hdr += r1 - r0; rd_body += r2 - r1; rd_push += now_s() - r2; }
        }
        if (timing) fprintf(stderr, "reader: %zu TI messages: waiting for header %.2fs, body %.2fs, queue push %.2fs\n", npairs, rd_hdr, rd_body, rd_push);
        for (int k = 2; k < np_all; k++) if (started[k]) ti_queue_close(&queues[k]);
        for (int k = 2; k < np_all; k++)
            if (started[k]) { pthread_join(tids[k], NULL); failed |= workers[k].failed; ti_queue_destroy(&queues[k]); }
        free(pairs); free(queues); free(workers); free(tids);
        check(!failed, "TI-mode aggregation failed");
        if (timing) fprintf(stderr, "party %d: TI-mode aggregation done after %.2fs\n", c->party, wall_clock() - t_start);
        break;
    }
    default:                /* the OT transports: phase1_ot.c */
        if (run_party_ot(self, c, job->device, n, Xq, yq, w1, &job->mode, share_A, share_b)) goto error;
    }
    /* every transport's words as w1-bit words (most come so already) */
    if (w1 == 32) { for (size_t k = 0; k < T; k++) share_A[k] &= 0xffffffffull; for (size_t k = 0; k < d; k++) share_b[k] &= 0xffffffffull; }
    return 0;
error:
    return 1;
}

int run_party(node *self, config *c, const p1_job *job, uint64_t **res_A, uint64_t **res_b, uint64_t **res_yy) {
    const int precision = job->precision, precision_p2 = job->precision_p2, w1 = job->w1, w2 = job->w2;
    const size_t folds = job->mode.folds, scan = job->mode.scan;
    if (!job->want_yy) res_yy = NULL;
    tune_malloc();
    pmsg_set_limit(c->n);
    const double t_start = wall_clock();
    const size_t n = c->n, d = c->d, T = d * (d + 1) / 2;
    const size_t K = folds ? folds : 1;                             /* share systems: [A_0][b_0] ... as K x T and K x d words */
    const int me = c->party - 1, last = c->num_parties - 1;
    int64_t *Xq = malloc(n * d * 8), *yq = malloc(n * 8);
    /* 200 MB at config 4, touched for the first time by the parser's threads while the HIP runtime comes up on another
     * thread: huge pages mean hundreds of page faults instead of 50 000 fighting that thread for the address-space lock */
    if (Xq && n * d * 8 >= ((size_t)8 << 20)) {
        const uintptr_t a = ((uintptr_t)Xq + 4095) & ~(uintptr_t)4095, e = ((uintptr_t)Xq + n * d * 8) & ~(uintptr_t)4095;
        (void)madvise((void *)a, (size_t)(e - a), MADV_HUGEPAGE);
    }
    uint64_t *share_A = calloc(K * T, 8), *share_b = calloc(K * d, 8);
    size_t *fr = calloc(K + 1, sizeof *fr);                         /* fold k is rows [fr[k], fr[k + 1]) */
    uint64_t *share_yy = res_yy ? calloc(K, 8) : NULL;              /* the folds' y^T y: zeros but for the provider that holds y */
    double *row_norm = NULL;
    lgc_p1 *p1 = 0;
    int rc = 1;
    check(Xq && yq && share_A && share_b && fr && (share_yy || !res_yy), "out of memory");
    check(!p1_mode_refuses(&job->mode), "%s", p1_mode_refuses(&job->mode));
    check(scan < d, "--scan needs at least one covariate column");
    fr[K] = n;
    for (size_t k = 0; k < folds; k++) check(lgc_fold_rows(n, folds, k, &fr[k], &fr[k + 1]) == LGC_OK, "--folds: %s", lgc_last_error());
    double normalizer = sqrt(pow(2, precision) * (double)n);      /* src/phase1.c:473 */
    {
        const size_t oc0 = (size_t)c->index_owned[me], oc1 = me < last ? (size_t)c->index_owned[me + 1] : d;
        if (folds) {                                                /* every row with its own fold's normalizer: n_k where a plain run has n */
            row_norm = malloc(n * sizeof *row_norm);
            check(row_norm != NULL, "out of memory");
            for (size_t k = 0; k < K; k++) {
                const double nk = sqrt(pow(2, precision) * (double)(fr[k + 1] - fr[k]));
                for (size_t r = fr[k]; r < fr[k + 1]; r++) row_norm[r] = nk;
            }
            check(!read_own_columns_rows(c->input, n, d, oc0, oc1, me == last, precision, row_norm, w2, Xq, yq), "Could not read data (dimensions or numbers invalid)");
        } else
            check(!read_own_columns(c->input, n, d, oc0, oc1, me == last, precision, normalizer, w2, Xq, yq), "Could not read data (dimensions or numbers invalid)");
    }
    if (getenv("LINREG_TIMING")) fprintf(stderr, "party %d: input parsed after %.2fs\n", c->party, wall_clock() - t_start);
    lgc_trace_mark("own columns parsed and quantised");
    LGC(lgc_p1_create(&p1, job->device, n, d, w1, precision));
    LGC(lgc_p1_set_data(p1, Xq, yq));
    lgc_trace_mark("phase-1 data on the device");
    const size_t c0 = (size_t)c->index_owned[me], c1 = me < last ? (size_t)c->index_owned[me + 1] : d;
    /* everything this party can do alone: its own block, incl. the floating-point diagonal -- of every fold, from one pass */
    if (scan) {
        /* --scan: the own covariates [cc0, cc1) as a plain run has them, the diagonal divided by c + 1 (the size of each fitted
         * system); the own candidates [s0, s1) against them and y, and their diagonals: no candidate meets another */
        const size_t cv = d - scan, cc0 = c0 < cv ? c0 : cv, cc1 = c1 < cv ? c1 : cv, s0 = c0 > cv ? c0 : cv, s1 = c1 > cv ? c1 : cv;
        const size_t nc = cc1 - cc0, ns = s1 - s0, Tb = nc * (nc + 1) / 2;
        uint64_t *blk = malloc((Tb + 2) * 8), *bb = malloc((nc + 2) * 8), *H = malloc((ns * nc + 1) * 8), *gg = malloc((ns + 1) * 8), *gy = malloc((ns + 1) * 8);
        check(blk && bb && H && gg && gy, "out of memory");
        LGC(lgc_p1_set_divisor(p1, cv + 1));
        if (nc) {
            if (res_yy && me == last) LGC(lgc_p1_local_yy(p1, cc0, cc1, blk, bb, share_yy));
            else LGC(lgc_p1_local(p1, cc0, cc1, me == last, blk, bb));
            for (size_t i = 0; i < nc; i++) {
                for (size_t j = 0; j <= i; j++) share_A[idx(cc0 + i, cc0 + j)] = blk[i * (i + 1) / 2 + j];
                if (me == last) share_b[cc0 + i] = bb[i];
            }
        } else if (res_yy && me == last) LGC(lgc_p1_local_yy(p1, s0, s0 + 1, blk, bb, share_yy));      /* (y^T y alone: the rest is dropped) */
        if (ns) {
            LGC(lgc_p1_local_scan(p1, cc0, cc1, s0, s1, me == last, H, gg, gy));
            for (size_t m = 0; m < ns; m++) {
                for (size_t i = 0; i < nc; i++) share_A[idx(s0 + m, cc0 + i)] = H[m * nc + i];
                share_A[idx(s0 + m, s0 + m)] = gg[m];
                if (me == last) share_b[s0 + m] = gy[m];
            }
        }
        free(blk); free(bb); free(H); free(gg); free(gy);
    } else {
        size_t own = c1 - c0, Tb = own * (own + 1) / 2;
        uint64_t *blk = malloc((K * Tb + 1) * 8), *bb = malloc((K * own + 1) * 8);
        check(blk && bb, "out of memory");
        if (folds && res_yy && me == last) LGC(lgc_p1_local_folds_yy(p1, c0, c1, folds, blk, bb, share_yy));   /* the same launch */
        else if (folds) LGC(lgc_p1_local_folds(p1, c0, c1, me == last, folds, blk, bb));
        else if (res_yy && me == last) LGC(lgc_p1_local_yy(p1, c0, c1, blk, bb, share_yy));                    /* --inference: the one word y^T y */
        else LGC(lgc_p1_local(p1, c0, c1, me == last, blk, bb));
        for (size_t k = 0; k < K; k++)
            for (size_t i = 0; i < own; i++) {
                for (size_t j = 0; j <= i; j++) share_A[k * T + idx(c0 + i, c0 + j)] = blk[k * Tb + i * (i + 1) / 2 + j];
                if (me == last) share_b[k * d + c0 + i] = bb[k * own + i];
            }
        free(blk); free(bb);
    }
    for (size_t k = 0; k < K; k++) {                                /* fold order, on the same sockets */
        if (folds) LGC(lgc_p1_set_rows(p1, fr[k], fr[k + 1]));
        check(!party_cross(self, c, p1, job, fr[k + 1] - fr[k], Xq + fr[k] * d, yq + fr[k], share_A + k * T, share_b + k * d, t_start),
              "phase-1 aggregation failed");
    }
    /* different widths in the two phases: every share is shifted on its own (src/phase1.c:609-638) */
    if (w1 == 64 && w2 == 32) {
        for (size_t k = 0; k < K * T; k++) share_A[k] = (uint64_t)(uint32_t)(uint64_t)(((int64_t)share_A[k]) >> (precision - precision_p2));
        for (size_t k = 0; k < K * d; k++) share_b[k] = (uint64_t)(uint32_t)(uint64_t)(((int64_t)share_b[k]) >> (precision - precision_p2));
        for (size_t k = 0; k < (share_yy ? K : 0); k++) share_yy[k] = (uint64_t)(uint32_t)(uint64_t)(((int64_t)share_yy[k]) >> (precision - precision_p2));
    }
    *res_A = share_A; *res_b = share_b;
    if (res_yy) *res_yy = share_yy;                                 /* (want_yy) */
    share_A = share_b = share_yy = 0;
    rc = 0;
error:
    if (p1) lgc_p1_destroy(p1);
    free(Xq); free(yq); free(share_A); free(share_b); free(fr); free(row_norm); free(share_yy);
    return rc;
}
