/* phase1_matrix.c -- phase 1 under the trusted initializer with one matrix triple per pair of data providers (--ti_matrix;
 * include/linreg_gc_p1_matrix.h): the initializer's side and a provider's side.  The plan of instances is ti_matrix_plan.c's.
 *   TI  : 8 bytes TM_MAGIC to every provider with an instance; per instance, in plan order: blob (seed_a, seed_s) to A,
 *         blob (seed_b, T) to B
 *   DP  : the main thread reads its messages off the TI socket in plan order and starts one worker per peer as each arrives;
 *         a worker masks its block, sends it on a helper thread while it receives the peer's (blocking sockets: neither side
 *         waits for the other's block before its own is on the way), then forms its share block and scatters it.
 * Raw blobs throughout (send_blob / recv_blob): W / 8 bytes per word, no protobuf. */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/linreg_gc.h"
#include "../../include/linreg_gc_p1_matrix.h"
#include "config.h"
#include "net.h"
#include "protocol.h"
#include "protocol_int.h"
#include "ti_matrix_plan.h"

static size_t plan_of(config *c, tm_inst **plan) {
    int *owner = config_owners(c);
    if (!owner) return (size_t)-1;
    const size_t count = tm_plan(owner, c->d, c->num_parties, plan);
    free(owner);
    return count;
}

int run_trusted_initializer_matrix(node *self, config *c, size_t n, int w1, int device, const uint8_t master[16]) {
    tm_inst *plan = NULL;
    const size_t count = plan_of(c, &plan);
    void *T = NULL;
    uint8_t *mb = NULL;
    int rc = 1, has[64] = {0};
    const int timing = getenv("LINREG_TIMING") != NULL;
    double t_gen = 0, t_all = wall_clock();
    check(count != (size_t)-1, "out of memory");
    check(c->num_parties <= 64, "too many parties");
    for (size_t q = 0; q < count; q++) { has[plan[q].lo] = 1; has[plan[q].hi] = 1; }
    for (int k = 2; k < c->num_parties; k++) {
        const uint64_t magic = TM_MAGIC;
        if (has[k]) check(!net_send(self, k + 1, &magic, sizeof magic), "Could not send message to a data provider");
    }
    for (size_t q = 0; q < count; q++) {
        const tm_inst *t = &plan[q];
        uint8_t sa[16], sb[16], ss[16], ma[TM_MSG_A_BYTES];
        size_t len = 0;
        LGC(lgc_ti_matrix_seeds(master, t->u, sa, sb, ss));
        T = malloc(t->a * t->b * (size_t)(w1 / 8));
        check(T != NULL, "out of memory");
        double t0 = wall_clock();
        LGC(lgc_ti_matrix_generate(device, sa, sb, ss, n, t->a, t->b, w1, T));
        t_gen += wall_clock() - t0;
        tm_msg_a(sa, ss, ma);
        mb = tm_msg_b(t, w1, sb, T, &len);
        check(mb != NULL, "out of memory");
        check(!send_blob(self, t->hi + 1, ma, sizeof ma) && !send_blob(self, t->lo + 1, mb, len), "Could not send message to a data provider");
        free(T); T = NULL; free(mb); mb = NULL;
    }
    if (timing) fprintf(stderr, "TI: %zu matrix triples: generate %.2fs, total %.2fs\n", count, t_gen, wall_clock() - t_all);
    rc = 0;
error:
    free(T); free(mb);
    if (count != (size_t)-1) tm_plan_free(plan, count);
    return rc;
}

typedef struct { node *self; int to; const void *buf; size_t len; int failed; } tm_send;
static void *tm_send_main(void *arg) {
    tm_send *s = arg;
    s->failed = send_blob(s->self, s->to, s->buf, s->len);
    return NULL;
}
typedef struct {
    node *self; lgc_p1 *p1; size_t n, d; int w, me;
    const tm_inst *t;
    uint8_t *msg;                 /* the initializer's message: (seed_a, seed_s) or (seed_b, T) */
    uint64_t *share_A, *share_b;
    int failed;
} tm_worker;
static void *tm_worker_main(void *arg) {
    tm_worker *w = arg;
    const tm_inst *t = w->t;
    const int is_a = t->hi == w->me, peer = is_a ? t->lo : t->hi;
    const size_t wb = (size_t)(w->w / 8), nown = is_a ? t->a : t->b, nother = is_a ? t->b : t->a;
    const uint32_t *own = is_a ? t->cols_a : t->cols_b;
    void *mine = malloc(w->n * nown * wb), *theirs = malloc(w->n * nother * wb);
    uint64_t *blk = malloc(t->a * t->b * 8);
    w->failed = 1;
    if (!mine || !theirs || !blk) { fprintf(stderr, "out of memory\n"); goto out; }
    if (lgc_p1_matrix_mask(w->p1, own, nown, w->msg, mine)) { fprintf(stderr, "%s\n", lgc_last_error()); goto out; }
    tm_send snd = {w->self, peer + 1, mine, w->n * nown * wb, 0};
    pthread_t th;
    if (pthread_create(&th, NULL, tm_send_main, &snd)) { fprintf(stderr, "pthread_create failed\n"); goto out; }
    const int bad = recv_blob(w->self, peer + 1, theirs, w->n * nother * wb);
    pthread_join(th, NULL);
    if (bad || snd.failed) { fprintf(stderr, "Could not exchange the masked blocks with party %d\n", peer + 1); goto out; }
    if (is_a ? lgc_p1_matrix_share_a(w->p1, t->a, w->msg, w->msg + 16, theirs, t->b, blk)
             : lgc_p1_matrix_share_b(w->p1, t->cols_b, t->b, theirs, t->a, w->msg + 16, blk)) { fprintf(stderr, "%s\n", lgc_last_error()); goto out; }
    tm_scatter(t, blk, w->d, w->share_A, w->share_b);
    w->failed = 0;
out:
    free(mine); free(theirs); free(blk);
    return NULL;
}

int run_party_ti_matrix(node *self, config *c, lgc_p1 *p1, size_t n, int w1, uint64_t *share_A, uint64_t *share_b) {
    const int me = c->party - 1;
    tm_inst *plan = NULL;
    const size_t count = plan_of(c, &plan);
    tm_worker *workers = NULL;
    pthread_t *tids = NULL;
    size_t mine = 0, started = 0;
    int rc = 1;
    check(count != (size_t)-1, "out of memory");
    for (size_t q = 0; q < count; q++) mine += plan[q].lo == me || plan[q].hi == me;
    if (!mine) { rc = 0; goto error; }
    workers = calloc(mine, sizeof *workers);
    tids = calloc(mine, sizeof *tids);
    check(workers && tids, "out of memory");
    uint64_t magic = 0;
    check(!net_recv(self, 1, &magic, sizeof magic), "Could not receive message from TI");
    check(magic == TM_MAGIC, "the trusted initializer does not speak --ti_matrix (this party was started with it): run every party in the same mode");
    for (size_t q = 0; q < count; q++) {
        const tm_inst *t = &plan[q];
        if (t->lo != me && t->hi != me) continue;
        const size_t len = t->hi == me ? (size_t)TM_MSG_A_BYTES : tm_msg_b_bytes(t, w1);
        uint8_t *msg = malloc(len);
        check(msg != NULL, "out of memory");
        if (recv_blob(self, 1, msg, len)) { free(msg); fprintf(stderr, "Could not receive message from TI\n"); break; }
        tm_worker w = {self, p1, n, c->d, w1, me, t, msg, share_A, share_b, 0};
        workers[started] = w;
        if (pthread_create(&tids[started], NULL, tm_worker_main, &workers[started])) { free(msg); fprintf(stderr, "pthread_create failed\n"); break; }
        started++;
    }
    rc = started == mine ? 0 : 1;
    for (size_t k = 0; k < started; k++) { pthread_join(tids[k], NULL); rc |= workers[k].failed; free(workers[k].msg); }
    started = 0;
error:
    for (size_t k = 0; k < started; k++) { pthread_join(tids[k], NULL); free(workers[k].msg); }
    free(workers); free(tids);
    if (count != (size_t)-1) tm_plan_free(plan, count);
    return rc;
}
