/* ot_pipe_program.c -- host/ot_pipe.c alone, in a program of its own (tests/test_ot_pipe_cpu.py builds it under ThreadSanitizer and
 * under ASan + UBSan): the sender role and the receiver role as two threads of one process, joined by a socketpair, with fake
 * callbacks that fill u and y with a pattern of the batch number and check the ordering rules of ot_pipe.h as they run.
 *    ot_pipe_program             every case: nbatch 1, 2, 3, 5 clean; then each callback of each side failing at k = 0, 1, 2 of 3
 * A role that returns closes its end of the socket pair, as a dying process would.  Prints "all ok" at the end; any broken rule
 * aborts with a message; an alarm of 20 s ends a run that hangs. */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdatomic.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/socket.h>
#include <unistd.h>
#include "ot_pipe.h"

#define MUST(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s does not hold (%s)\n", __FILE__, __LINE__, #cond, g_case); abort(); } } while (0)
enum { PREPARE, START, FINISH, SEND, PUT, GET, NCALLS };
static const char *const kCall[NCALLS] = {"prepare", "start", "finish", "send", "put", "get"};
static char g_case[96];

typedef struct side {
    int sender, fd;
    size_t nbatch;
    int fail_call; size_t fail_k;             /* fail_call < 0: nothing fails on this side */
    atomic_size_t calls[NCALLS], done[NCALLS];  /* entered / returned well, per callback */
    ot_pipe pipe;
    int rc;
} side;

/* the last batch is shorter than the others */
static size_t u_len(void *arg, size_t k) { side *s = arg; return k + 1 == s->nbatch ? 40 : 64; }
static size_t y_len(void *arg, size_t k) { side *s = arg; return k + 1 == s->nbatch ? 56 : 96; }
static uint8_t pattern(int what, size_t k, size_t i) { return (uint8_t)(what * 101 + k * 37 + i * 3 + 1); }
static void fill(uint8_t *buf, size_t len, int what, size_t k) { for (size_t i = 0; i < len; i++) buf[i] = pattern(what, k, i); }
static int holds(const uint8_t *buf, size_t len, int what, size_t k) {
    for (size_t i = 0; i < len; i++) if (buf[i] != pattern(what, k, i)) return 0;
    return 1;
}
/* every callback of a side runs once per k, in order; 1 when this is the call that is to fail */
static int enter(side *s, int call, size_t k) {
    MUST(atomic_fetch_add(&s->calls[call], 1) == k && k < s->nbatch);
    if (s->fail_call != call || s->fail_k != k) return 0;
    if (call == PUT || call == GET) shutdown(s->fd, SHUT_RDWR);     /* what makes a transport call fail: the connection is gone */
    return 1;
}
static int leave(side *s, int call) { atomic_fetch_add(&s->done[call], 1); return 0; }

static int cb_prepare(void *arg, size_t k) {
    side *s = arg;
    if (enter(s, PREPARE, k)) return 1;
    return leave(s, PREPARE);
}
static int cb_start(void *arg, size_t k, void *u) {
    side *s = arg;
    MUST(!s->sender && u == s->pipe.u[0]);
    MUST(k < 2 || atomic_load(&s->done[FINISH]) >= k - 1);            /* finish(k - 2) has returned */
    MUST(atomic_load(&s->done[PREPARE]) == k + 1);
    if (enter(s, START, k)) return 1;
    fill(u, u_len(s, k), 'u', k);
    return leave(s, START);
}
static int cb_send(void *arg, size_t k, const void *u, void *y) {
    side *s = arg;
    MUST(s->sender && u == s->pipe.u[k & 1] && y == s->pipe.y[k & 1]);
    MUST(atomic_load(&s->done[PREPARE]) == k + 1);
    MUST(atomic_load(&s->done[GET]) >= k + 1);                        /* u of batch k is here */
    MUST(k < 2 || atomic_load(&s->done[PUT]) >= k - 1);               /* y of batch k - 2 has left its buffer */
    if (enter(s, SEND, k)) return 1;
    MUST(holds(u, u_len(s, k), 'u', k));                              /* what start(k) wrote */
    fill(y, y_len(s, k), 'y', k);
    return leave(s, SEND);
}
static int cb_finish(void *arg, size_t k, const void *y) {
    side *s = arg;
    MUST(!s->sender && y == s->pipe.y[0]);
    MUST(atomic_load(&s->done[GET]) == k + 1);
    if (enter(s, FINISH, k)) return 1;
    MUST(holds(y, y_len(s, k), 'y', k));                              /* what send(k) wrote */
    return leave(s, FINISH);
}
static int cb_put(void *arg, const void *buf, size_t len) {
    side *s = arg;
    const size_t k = atomic_load(&s->calls[PUT]);
    if (s->sender) {
        MUST(atomic_load(&s->done[SEND]) >= k + 1);                   /* send(k) has returned */
        MUST(buf == s->pipe.y[k & 1] && len == y_len(s, k));
    } else
        MUST(atomic_load(&s->done[START]) == k + 1 && buf == s->pipe.u[0] && len == u_len(s, k));
    if (enter(s, PUT, k)) return 1;
    for (size_t off = 0; off < len;) {
        const ssize_t n = send(s->fd, (const char *)buf + off, len - off, MSG_NOSIGNAL);
        if (n <= 0) return 1;
        off += (size_t)n;
    }
    return leave(s, PUT);
}
static int cb_get(void *arg, void *buf, size_t len) {
    side *s = arg;
    const size_t k = atomic_load(&s->calls[GET]);
    if (s->sender) {
        MUST(k < 2 || atomic_load(&s->done[SEND]) >= k - 1);          /* send(k - 2) has returned: u[k & 1] is free */
        MUST(buf == s->pipe.u[k & 1] && len == u_len(s, k));
    } else
        MUST(buf == s->pipe.y[0] && len == y_len(s, k) && atomic_load(&s->done[PUT]) >= k + 1);
    if (enter(s, GET, k)) return 1;
    for (size_t off = 0; off < len;) {
        const ssize_t n = recv(s->fd, (char *)buf + off, len - off, 0);
        if (n <= 0) return 1;
        off += (size_t)n;
    }
    return leave(s, GET);
}

static void *role(void *arg) {
    side *s = arg;
    s->rc = s->sender ? ot_pipe_send(&s->pipe) : ot_pipe_receive(&s->pipe);
    shutdown(s->fd, SHUT_RDWR);
    close(s->fd);
    return NULL;
}

/* fail_sender < 0: a clean run */
static void run_case(size_t nbatch, int fail_sender, int fail_call, size_t fail_k) {
    int fds[2];
    side sd[2];
    pthread_t th[2];
    snprintf(g_case, sizeof g_case, "nbatch %zu, %s %s fails at k = %zu", nbatch, fail_sender < 0 ? "nobody's" : fail_sender ? "the sender's" : "the receiver's",
             fail_sender < 0 ? "call" : kCall[fail_call], fail_k);
    MUST(!socketpair(AF_UNIX, SOCK_STREAM, 0, fds));
    memset(sd, 0, sizeof sd);
    for (int i = 0; i < 2; i++) {                                    /* sd[1] is the sender */
        side *s = &sd[i];
        s->sender = i; s->fd = fds[i]; s->nbatch = nbatch;
        s->fail_call = fail_sender == i ? fail_call : -1; s->fail_k = fail_k;
        const ot_pipe p = {.nbatch = nbatch, .arg = s, .prepare = cb_prepare, .start = cb_start, .finish = cb_finish, .send = cb_send,
                           .u_bytes = u_len, .y_bytes = y_len, .put = cb_put, .get = cb_get};
        s->pipe = p;
        for (int b = 0; b < (i ? 2 : 1); b++) { s->pipe.u[b] = malloc(64); s->pipe.y[b] = malloc(96); MUST(s->pipe.u[b] && s->pipe.y[b]); }
    }
    for (int i = 0; i < 2; i++) MUST(!pthread_create(&th[i], NULL, role, &sd[i]));
    for (int i = 0; i < 2; i++) MUST(!pthread_join(th[i], NULL));
    side *rcv = &sd[0], *snd = &sd[1];
    const int mine_r[] = {PREPARE, START, PUT, GET, FINISH}, mine_s[] = {PREPARE, GET, SEND, PUT};
    int whole_r = 1, whole_s = 1;
    for (int i = 0; i < 5; i++) whole_r &= atomic_load(&rcv->done[mine_r[i]]) == nbatch;
    for (int i = 0; i < 4; i++) whole_s &= atomic_load(&snd->done[mine_s[i]]) == nbatch;
    MUST(!atomic_load(&rcv->calls[SEND]) && !atomic_load(&snd->calls[START]) && !atomic_load(&snd->calls[FINISH]));
    if (fail_sender < 0) MUST(!rcv->rc && !snd->rc && whole_r && whole_s);
    else {
        MUST(sd[fail_sender].rc != 0);
        /* The other role fails as well whenever it still needs something from the one that failed.  Only the sender can be past
         * that point: the receiver may send u of the last batch as soon as batch nbatch - 3 is finished, and this wire has no
         * word from the receiver after that, so its get(y) or finish failing at batch nbatch - 2 or later is nothing the sender
         * ever hears of.  Then the sender must have run every callback for every batch. */
        const int sender_may_be_done = !fail_sender && (fail_call == GET || fail_call == FINISH) && fail_k + 2 >= nbatch;
        MUST(sd[1 - fail_sender].rc != 0 || (sender_may_be_done && whole_s));
    }
    for (int i = 0; i < 2; i++) for (int b = 0; b < 2; b++) { free(sd[i].pipe.u[b]); free(sd[i].pipe.y[b]); }
}

int main(void) {
    alarm(20);
    const size_t clean[] = {1, 2, 3, 5};
    int cases = 0;
    for (size_t i = 0; i < 4; i++, cases++) run_case(clean[i], -1, -1, 0);
    for (int sender = 0; sender < 2; sender++)
        for (int call = 0; call < NCALLS; call++) {
            if (sender ? (call == START || call == FINISH) : call == SEND) continue;      /* not a callback of that role */
            for (size_t k = 0; k < 3; k++, cases++) run_case(3, sender, call, k);
        }
    printf("%d cases\nall ok\n", cases);
    return 0;
}
