/* ot_pipe.c -- see ot_pipe.h.  One mutex, one condition variable and five counters of completed batches per role; every wait is
 * "counter + ahead > k, or somebody failed". */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>
#include "ot_pipe.h"

typedef struct {
    const ot_pipe *p;
    size_t started, finished;               /* receiver: batches whose u has left / whose shares are in */
    size_t recvd, gpu_done, sent;           /* sender: batches whose u is here / whose y is computed / whose y has left */
    int failed;
    double tt[3];                           /* LINREG_TIMING: the sender's calling thread, the receiver's helper thread */
    pthread_mutex_t mu;
    pthread_cond_t cv;
} pipe_state;

static double now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }
/* batch `value` of *field is complete, or (bad) the role has failed: either way every waiter looks again */
static void mark(pipe_state *s, size_t *field, size_t value, int bad) {
    pthread_mutex_lock(&s->mu);
    if (bad) s->failed = 1; else if (field) *field = value;
    pthread_cond_broadcast(&s->cv);
    pthread_mutex_unlock(&s->mu);
}
/* until *count + ahead > k; non-zero when the role has failed first.  A batch that is ready when the failure shows is still run:
 * the peer may need the y of a batch that was sent well before it sends the u that this role's get is blocked in, and a role
 * returns only when all its threads are back */
static int await(pipe_state *s, const size_t *count, size_t ahead, size_t k) {
    pthread_mutex_lock(&s->mu);
    while (*count + ahead <= k && !s->failed) pthread_cond_wait(&s->cv, &s->mu);
    const int bad = *count + ahead <= k;
    pthread_mutex_unlock(&s->mu);
    return bad;
}

/* receiver, helper thread: starts batches and sends their u */
static void *recv_starter(void *v) {
    pipe_state *s = v;
    const ot_pipe *p = s->p;
    for (size_t k = 0; k < p->nbatch; k++) {
        if (await(s, &s->finished, 2, k)) break;
        const double t0 = now();
        int bad = p->prepare(p->arg, k);
        double t1 = now(), t2 = t1;
        if (!bad) bad = p->start(p->arg, k, p->u[0]);
        if (!bad && (t2 = now(), bad = p->put(p->arg, p->u[0], p->u_bytes(p->arg, k)))) fprintf(stderr, "OT: could not send u\n");
        s->tt[0] += t1 - t0; s->tt[1] += t2 - t1; s->tt[2] += now() - t2;
        mark(s, &s->started, k + 1, bad);
        if (bad) break;
    }
    return NULL;
}
static int recv_step(pipe_state *s, size_t k) {
    const ot_pipe *p = s->p;
    if (await(s, &s->started, 0, k)) return 1;
    int bad = p->get(p->arg, p->y[0], p->y_bytes(p->arg, k));
    if (bad) fprintf(stderr, "OT: could not receive y\n");
    else bad = p->finish(p->arg, k, p->y[0]);
    mark(s, &s->finished, k + 1, bad);
    return bad;
}

/* sender, helper threads: u in, y out */
static void *send_get_u(void *v) {
    pipe_state *s = v;
    const ot_pipe *p = s->p;
    for (size_t k = 0; k < p->nbatch; k++) {
        if (await(s, &s->gpu_done, 2, k)) break;
        const int bad = p->get(p->arg, p->u[k & 1], p->u_bytes(p->arg, k));
        if (bad) fprintf(stderr, "OT: could not receive u\n");
        mark(s, &s->recvd, k + 1, bad);
        if (bad) break;
    }
    return NULL;
}
static void *send_put_y(void *v) {
    pipe_state *s = v;
    const ot_pipe *p = s->p;
    for (size_t k = 0; k < p->nbatch; k++) {
        if (await(s, &s->gpu_done, 0, k)) break;
        const int bad = p->put(p->arg, p->y[k & 1], p->y_bytes(p->arg, k));
        if (bad) fprintf(stderr, "OT: could not send y\n");
        mark(s, &s->sent, k + 1, bad);
        if (bad) break;
    }
    return NULL;
}
static int send_step(pipe_state *s, size_t k) {
    const ot_pipe *p = s->p;
    const double t0 = now();
    int bad = p->prepare(p->arg, k);
    const double t1 = now();
    /* u of batch k is here, and the y buffer it will fill is free */
    if (!bad) bad = await(s, &s->recvd, 0, k) || await(s, &s->sent, 2, k);
    const double t2 = now();
    if (!bad) bad = p->send(p->arg, k, p->u[k & 1], p->y[k & 1]);
    mark(s, &s->gpu_done, k + 1, bad);
    s->tt[0] += t1 - t0; s->tt[1] += t2 - t1; s->tt[2] += now() - t2;
    return bad;
}

/* the role's helper threads around its calling thread's steps; whatever fails, a pthread_create included, every helper that was
 * started is woken and joined before this returns */
static int run_role(pipe_state *s, int nhelper, void *(*const helper[])(void *), int (*step)(pipe_state *, size_t)) {
    pthread_t th[2];
    int n = 0;
    pthread_mutex_init(&s->mu, NULL); pthread_cond_init(&s->cv, NULL);
    while (n < nhelper && !pthread_create(&th[n], NULL, helper[n], s)) n++;
    int bad = n < nhelper;
    for (size_t k = 0; k < s->p->nbatch && !bad; k++) bad = step(s, k);
    if (bad) mark(s, NULL, 0, 1);
    for (int i = 0; i < n; i++) pthread_join(th[i], NULL);
    bad |= s->failed;
    pthread_mutex_destroy(&s->mu); pthread_cond_destroy(&s->cv);
    return bad;
}

int ot_pipe_receive(const ot_pipe *p) {
    static void *(*const helper[])(void *) = {recv_starter};
    pipe_state s = {.p = p};
    const int bad = run_role(&s, 1, helper, recv_step);
    if (getenv("LINREG_TIMING")) fprintf(stderr, "OT receiver (start thread): columns %.2fs, gpu %.2fs, send u %.2fs\n", s.tt[0], s.tt[1], s.tt[2]);
    return bad;
}
int ot_pipe_send(const ot_pipe *p) {
    static void *(*const helper[])(void *) = {send_get_u, send_put_y};
    pipe_state s = {.p = p};
    const int bad = run_role(&s, 2, helper, send_step);
    if (getenv("LINREG_TIMING")) fprintf(stderr, "OT sender: columns %.2fs, waiting for u / a free y buffer %.2fs, gpu %.2fs\n", s.tt[0], s.tt[1], s.tt[2]);
    return bad;
}
