/* ot_pipe.h -- the batch pipeline of phase 1's OT modes (phase1_ot.c: batches of column pairs; phase1_ot_matrix.c: batches of whole
 * rows): one provider pair's batches 0 .. nbatch - 1 for one role, two in flight.  No GPU call, no socket call, no global: what a
 * batch is and how its bytes travel are the caller's callbacks, each returning 0 or, on failure, non-zero after printing its own
 * message.  The buffers are the caller's (page-locked, lgc_host_alloc) and hold the largest batch.
 *   receiver  a helper thread runs prepare(k), start(k, u) and put(u) for k = 0, 1, ..., never more than two batches ahead of the
 *             batch last finished; the calling thread runs get(y), then finish(k, y), in order.  Buffers u[0] and y[0].
 *   sender    one helper thread runs get(u) of batch k into u[k & 1] once send(k - 2) is done, another put(y[k & 1]) once send(k)
 *             is done; the calling thread runs prepare(k), waits for u of batch k and for y of batch k - 2 to have left, then
 *             runs send(k, u[k & 1], y[k & 1]).
 *   failure   anywhere: every thread of the role is woken and joined, then the role returns non-zero.  Nothing of the caller's is
 *             touched after that. */
#ifndef LINREG_OT_PIPE_H
#define LINREG_OT_PIPE_H
#include <stddef.h>

typedef struct {
    size_t nbatch;
    void *arg;                                                     /* first argument of every callback */
    int (*prepare)(void *arg, size_t k);                           /* gather the own operand of batch k */
    int (*start)(void *arg, size_t k, void *u);                    /* receiver: *_recv_start, fills u */
    int (*finish)(void *arg, size_t k, const void *y);             /* receiver: *_recv_finish, adds up the shares */
    int (*send)(void *arg, size_t k, const void *u, void *y);      /* sender: *_send, fills y, adds up the shares */
    size_t (*u_bytes)(void *arg, size_t k), (*y_bytes)(void *arg, size_t k);
    int (*put)(void *arg, const void *buf, size_t len);            /* to the peer */
    int (*get)(void *arg, void *buf, size_t len);                  /* from the peer */
    void *u[2], *y[2];
} ot_pipe;

int ot_pipe_receive(const ot_pipe *p);
int ot_pipe_send(const ot_pipe *p);
#endif
