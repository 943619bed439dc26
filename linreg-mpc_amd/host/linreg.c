/* linreg.c -- `bin/linreg`: the reference's command line, roles, input file and stdout
 * contract (src/cmd/linreg.c:44-212), with every compute step on the MI355X through the C ABI
 * of liblinreg_gc (include/linreg_gc.h).  Host code stays C; this file only moves bytes.
 *
 *   linreg [Input_file] [Precision] [Party] [Algorithm] [Num. iterations CGD] [Lambda] [Options]
 *   Options: --use_ot, --prec_phase2=<p>, and (new; compile-time in the reference, Makefile:8-9)
 *            --width_phase1=<32|64>, --width_phase2=<32|64>
 *
 *   party 1 = CSP (trusted initializer in phase 1, garbler in phase 2)
 *   party 2 = Evaluator, parties >= 3 = data providers (README.md:41-45)
 *
 * What a run is -- the options, the rules between them, the phase-2 request, the share and result layouts -- is linreg_run.h's
 * to say; here main() is the order of the steps and run_csp / run_evaluator / run_provider are the three roles of phase 2.
 */
#define _GNU_SOURCE
#include <errno.h>
#include <math.h>
#include <openssl/crypto.h>
#include <openssl/rand.h>
#include <poll.h>
#include <pthread.h>
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "baseot.h"
#include "protocol.h"
#include "linreg_run.h"
#include "../../include/linreg_gc_lasso.h"
#include "../../include/linreg_gc_lasso_path.h"
#include "../../include/linreg_gc_lasso_opts.h"
#include "../../include/linreg_gc_folds.h"
#include "../../include/linreg_gc_lasso_cv_se.h"
#include "../../include/linreg_gc_ridge_cv.h"
#include "../../include/linreg_gc_inference.h"
#include "../../include/linreg_gc_scan.h"

/* LINREG_TRACE=1: wall-clock marks on stderr (where an end-to-end run of a small configuration spends its time) */
/* (LGCT lines on the system-wide monotonic clock, shared with the library's own marks: lgc_trace_mark) */
#define TRACE(what) host_trace_mark(what)

/* what a role works with: the mesh, the configuration, the plan of the run and the phase-2 object(s) of party 1 / 2 */
typedef struct {
    node *self; config *c; const run_plan *plan; int device;
    lgc_party *party_obj, **blocks;             /* --devices: plan->n_blocks blocks, blocks[0] == party_obj */
    double time;                                /* the wall clock when the configuration was read */
    uint64_t *share_A, *share_b, *share_yy;     /* a data provider's share from phase 1 */
} run_ctx;

typedef struct { size_t n, next; const uint32_t *launch; double *time; double t0; } iter_marks;
static void note_launch(size_t i, void *ctx) {
    iter_marks *m = ctx;
    if (i == 0) host_trace_mark("first table evaluated");
    while (m->next < m->n && m->launch[m->next] == i) m->time[m->next++] = wall_clock() - m->t0;
}

/* --devices: one block of the sweep per GPU, one thread and one table link per block */
typedef struct { table_link link; size_t lo, hi; int sending, rc; pthread_t th; } block_job;
static void *block_main(void *arg) {
    block_job *b = arg;
    b->rc = b->sending ? table_link_send_range(&b->link, b->lo, b->hi) : table_link_recv_range(&b->link, b->lo, b->hi, NULL, NULL);
    return NULL;
}
/* contiguous block [lo, hi) of block k out of K; sizes differ by at most one (python/sweep.py: partition) */
#define block_range sweep_block_range      /* host/sweep_plan.c */

/* The phase-2 object(s) of party 1 / 2: one, or with --devices one block of the sweep per entry (same seed: one set of
 * input labels, one label OT per data provider; block k starts at circuit lo_k, which keeps its gate ids disjoint), and for
 * the garbler its table ring(s).  A job, so that the CSP can run it on a thread while it is still the trusted initializer
 * of phase 1: lowering the program, the word file and -- above all -- a ring of several GB used to start after the barrier,
 * with every other party waiting.  Which call, and what it is told, is the plan's (run_plan.create). */
typedef struct {
    const run_plan *plan; int role;
    lgc_party **blocks, *party_obj; int rc; char err[256]; pthread_t th; int started;
} create_job;
static void *create_main(void *arg) {
    create_job *j = arg;
    const run_plan *p = j->plan;
    const lgc_system *sys = &p->sys;
    const size_t chunk = p->table_chunk;
    const int device = p->device, role = j->role;
    uint8_t seed[16];
    const uint8_t *seedp = NULL;
    j->rc = 1;
    if (role == LGC_ROLE_GARBLER) {
        if (RAND_bytes(seed, sizeof seed) != 1) { snprintf(j->err, sizeof j->err, "RAND_bytes failed"); return NULL; }
        seedp = seed;
    }
#define JLGC(x) do { if ((x) != LGC_OK) { snprintf(j->err, sizeof j->err, "%s", lgc_last_error()); OPENSSL_cleanse(seed, sizeof seed); return NULL; } } while (0)
    switch (p->create) {
    case RUN_CREATE_SCAN: JLGC(lgc_party_create_scan(&j->party_obj, device, sys, role, seedp, chunk, p->scan_M, p->resid_scale, p->scan_bits)); break;
    case RUN_CREATE_INFERENCE: JLGC(lgc_party_create_inference(&j->party_obj, device, sys, role, seedp, chunk, p->resid_scale, p->infer)); break;
    case RUN_CREATE_RIDGE_CV: JLGC(lgc_party_create_ridge_cv(&j->party_obj, device, sys, role, seedp, chunk, p->n_lambdas, p->lambdas, p->folds, p->reveal)); break;
    case RUN_CREATE_SWEEP_BLOCKS:
        for (int k = 0; k < p->n_blocks; k++) {
            size_t lo, hi;
            block_range(p->n_lambdas, (size_t)p->n_blocks, (size_t)k, &lo, &hi);
            JLGC(lgc_party_create_sweep_at(&j->blocks[k], p->o->devices[k], sys, role, seedp, chunk, hi - lo, p->lambdas + lo, lo));
        }
        j->party_obj = j->blocks[0];
        break;
    case RUN_CREATE_SWEEP: JLGC(lgc_party_create_sweep(&j->party_obj, device, sys, role, seedp, chunk, p->n_lambdas, p->lambdas)); break;
    case RUN_CREATE_LASSO_CV_SE: JLGC(lgc_party_create_lasso_cv_se(&j->party_obj, device, sys, role, seedp, chunk, p->lasso, p->folds, p->reveal, p->rule)); break;
    case RUN_CREATE_LASSO_CV: JLGC(lgc_party_create_lasso_cv(&j->party_obj, device, sys, role, seedp, chunk, p->lasso, p->folds, p->reveal)); break;
    case RUN_CREATE_LASSO_OPTS: JLGC(lgc_party_create_lasso_opts(&j->party_obj, device, sys, role, seedp, chunk, p->lasso)); break;
    case RUN_CREATE_LASSO_PATH: JLGC(lgc_party_create_lasso_path(&j->party_obj, device, sys, role, seedp, chunk, p->n_path, p->o->l1.v, p->l1_mode)); break;
    case RUN_CREATE_LASSO: JLGC(lgc_party_create_lasso(&j->party_obj, device, sys, role, seedp, chunk, p->o->l1.v[0])); break;
    case RUN_CREATE_PLAIN: JLGC(lgc_party_create(&j->party_obj, device, sys, role, seedp, chunk)); break;
    }
#undef JLGC
    OPENSSL_cleanse(seed, sizeof seed);
    /* (the table ring is NOT created here: hipIpcGetMemHandle on this thread, beside the initializer's own allocations and
     * exports on the main thread, failed with "invalid argument" in up to a third of the five-process runs on some boxes --
     * the main thread creates it after phase 1, create_rings below: a millisecond for a byte ring) */
    lgc_trace_mark(role == LGC_ROLE_GARBLER ? "garbler created" : "evaluator created");
    j->rc = 0;
    return NULL;
}
static int create_rings(create_job *j) {                            /* the garbler's ring(s), before the Evaluator asks for them */
    const int ring_slots = j->plan->o->ring_slots, n_blocks = j->plan->n_blocks;
    if (j->role != LGC_ROLE_GARBLER || ring_slots <= 0) return 0;
    for (int k = 0; k < (n_blocks ? n_blocks : 1); k++)
        if (tables_ring_prepare(n_blocks ? j->blocks[k] : j->party_obj, ring_slots)) {
            snprintf(j->err, sizeof j->err, "could not create table ring %d", k);
            return 1;
        }
    return 0;
}
/* The CSP and the Evaluator live until the end of the protocol.  When one of them is gone -- its connection hung up -- the
 * other normally notices in its next recv() and leaves through check(); but it may sit in a call that never returns once the
 * peer is dead (seen: hipIpcOpenMemHandle on the ring of a CSP killed a moment earlier; a test of tests/test_host.py hit that
 * window once in six runs).  A watchdog thread polls the connection and ends the process with the reference's exit code for
 * every failure (src/cmd/linreg.c:206-211) -- but only for a hang-up that is a FAILURE: the peer left before this party had
 * everything it needs from it (g_peer_finished: set when the decode bits are in / out and the ring has been released), and
 * the main thread has not moved for five seconds since (host_progress: every launch and every trace mark ticks).  A healthy
 * CSP leaves before the Evaluator has printed its results, and POLLRDHUP fires on its FIN: a watchdog that only counted five
 * seconds from the hang-up would kill a slow but healthy Evaluator (a shared GPU, a profiler, a blocked stdout). */
static volatile int g_protocol_over;      /* 1: results are out, cleaning up; 2: main is about to return */
static volatile int g_peer_finished;      /* nothing more is needed from the watched peer: its hang-up is not an event */
typedef struct { int fd, party, peer; } watchdog_arg;
static void *peer_watchdog(void *arg) {
    watchdog_arg *w = arg;
    struct pollfd pf = {w->fd, POLLRDHUP, 0};
    for (;;) {
        if (g_protocol_over >= 2 || g_peer_finished) return NULL;
        pf.revents = 0;
        int r = poll(&pf, 1, 250);
        if (r > 0 && (pf.revents & (POLLRDHUP | POLLHUP | POLLERR | POLLNVAL))) break;
    }
    unsigned long seen = host_progress();
    for (int quiet = 0; quiet < 20;) {                               /* 20 x 250 ms without a sign of life */
        if (g_protocol_over >= 2 || g_peer_finished) return NULL;
        usleep(250000);
        unsigned long now = host_progress();
        if (now != seen) { seen = now; quiet = 0; } else quiet++;
    }
    if (g_protocol_over >= 2 || g_peer_finished) return NULL;
    if (g_protocol_over == 1) { fflush(stdout); _exit(0); }          /* the protocol was through: only the clean-up is stuck */
    fprintf(stderr, "party %d: party %d is gone and this party is stuck in a call that does not return; giving up\n", w->party, w->peer);
    _exit(1);
}

/* the HIP runtime and the device context come up on a thread of their own while main parses, connects and reads */
static int g_warm_what;
static void *warm_main(void *arg) {
    int device = *(int *)arg;
    if (lgc_device_warm(device) == LGC_OK && g_warm_what) (void)lgc_preload(device, g_warm_what);
    return NULL;
}

/* One thread per data provider on the CSP: the base OTs (128 P-256 transfers, host work on both sides) and then the label
 * OT of that provider's share (dcrRecvBitArray, src/input.c:94-108) -- its own connection, its own OpenSSL objects, its own
 * OT session and page-locked buffers.  The providers are independent of each other; served one after the other, as in
 * rounds 1-3, the label OTs were 20-25 ms of latency EACH on the critical path of every run. */
typedef struct {
    node *self; int peer, device, rc, ring; lgc_party *po; size_t share, bits; char err[256]; pthread_t th;
} input_ot_job;
/* --input_ring (every party on this node): the messages of the label OT stay in HBM.  The provider owns a device buffer
 * [u | e] that the CSP maps (hipIpc): it holds what the socket would carry between those two -- the provider's masked columns u,
 * the CSP's ciphertexts e -- and nothing else; the label PAIRS stay in two device buffers private to the CSP; the chosen labels
 * go to the Evaluator through a second buffer of the provider's that only the Evaluator maps.  Sockets carry the 64-byte
 * handles and one-byte tokens.  (config 4: 256 MB per provider that used to cross a socket and PCIe twice.) */
static int input_ot_ring_csp(input_ot_job *j, lgc_ot_sender *S) {
    const size_t bits = j->bits, ub = lgc_ot_u_bytes(bits);
    void *d0 = NULL, *d1 = NULL, *ue = NULL;
    uint8_t h[64], tok = 1;
    int rc = 1;
    if (lgc_ot_sender_set_device_io(S, 1) != LGC_OK) goto out;
    if (lgc_dev_alloc(j->device, bits * 16, &d0, NULL) != LGC_OK || lgc_dev_alloc(j->device, bits * 16, &d1, NULL) != LGC_OK) goto out;
    if (lgc_party_input_pairs_dev(j->po, j->share, d0, d1) != LGC_OK) goto out;
    lgc_trace_mark("input OT: label pairs exported");
    if (recv_blob(j->self, j->peer, h, sizeof h)) { snprintf(j->err, sizeof j->err, "OT: no buffer handle from party %d", j->peer); goto out2; }
    if (lgc_dev_open(j->device, h, &ue) != LGC_OK) goto out;
    lgc_trace_mark("input OT: u received");
    if (lgc_ot_labels_send(S, d0, d1, bits, ue, (uint8_t *)ue + ub) != LGC_OK) goto out;
    lgc_trace_mark("input OT: ciphertexts computed");
    lgc_dev_close(ue); ue = NULL;
    if (send_blob(j->self, j->peer, &tok, 1)) { snprintf(j->err, sizeof j->err, "OT: could not signal party %d", j->peer); goto out2; }
    rc = 0;
    goto out2;
out:
    snprintf(j->err, sizeof j->err, "%s", lgc_last_error());
out2:
    if (ue) lgc_dev_close(ue);
    lgc_dev_free_secret(d0, bits * 16);                              /* both labels of every input bit: their XOR is R */
    lgc_dev_free_secret(d1, bits * 16);
    return rc;
}
static void *input_ot_main(void *arg) {
    input_ot_job *j = arg;
    uint8_t delta[16], seeds[128][16];
    uint8_t *m0 = NULL, *m1 = NULL, *u = NULL, *e = NULL;
    lgc_ot_sender *S = NULL;
    const size_t bits = j->bits;
    j->rc = 1;
#define JFAIL(...) do { snprintf(j->err, sizeof j->err, __VA_ARGS__); goto out; } while (0)
    if (baseot_ext_sender(j->self, j->peer, delta, seeds)) JFAIL("base OT with party %d failed", j->peer);
    lgc_trace_mark("base OTs done");
    if (j->ring) {
        if (lgc_ot_sender_create(&S, j->device, delta, seeds) != LGC_OK) JFAIL("%s", lgc_last_error());
        if (input_ot_ring_csp(j, S)) goto out;
        j->rc = 0;
        goto out;
    }
    m0 = lgc_host_alloc(bits * 16); m1 = lgc_host_alloc(bits * 16); u = lgc_host_alloc(lgc_ot_u_bytes(bits)); e = lgc_host_alloc(bits * 32);
    if (!m0 || !m1 || !u || !e) JFAIL("%s", lgc_last_error());
    lgc_trace_mark("input OT: page-locked buffers");
    if (lgc_ot_sender_create(&S, j->device, delta, seeds) != LGC_OK) JFAIL("%s", lgc_last_error());
    lgc_trace_mark("input OT: sender session");
    if (lgc_party_input_pairs(j->po, j->share, m0, m1) != LGC_OK) JFAIL("%s", lgc_last_error());
    lgc_trace_mark("input OT: label pairs exported");
    if (recv_blob(j->self, j->peer, u, lgc_ot_u_bytes(bits))) JFAIL("OT: could not receive u from party %d", j->peer);
    lgc_trace_mark("input OT: u received");
    if (lgc_ot_labels_send(S, m0, m1, bits, u, e) != LGC_OK) JFAIL("%s", lgc_last_error());
    lgc_trace_mark("input OT: ciphertexts computed");
    if (send_blob(j->self, j->peer, e, bits * 32)) JFAIL("OT: could not send to party %d", j->peer);
    j->rc = 0;
out:
#undef JFAIL
    if (S) lgc_ot_sender_destroy(S);
    if (m0) OPENSSL_cleanse(m0, bits * 16);                          /* both labels of every input bit: their XOR is R */
    if (m1) OPENSSL_cleanse(m1, bits * 16);
    lgc_host_free(m0); lgc_host_free(m1); lgc_host_free(u); lgc_host_free(e);
    OPENSSL_cleanse(delta, sizeof delta); OPENSSL_cleanse(seeds, sizeof seeds);   /* base-OT delta and seeds */
    return NULL;
}

/* ------------------------------------------------------------------------------------------------- the blocks of --devices
 * Both sides of a sharded sweep: one table link (hipIpc ring + token connection) and one thread per block.  Block 0 garbles /
 * evaluates the shared prefix first; its share sums go to the other GPUs over xGMI; then all blocks run side by side.  The CSP
 * (sending) offers the lanes, sends every block's decode bits and then waits for the Evaluator to release the rings; the
 * Evaluator accepts the lanes, releases the rings once every launch of every block is evaluated, and then takes the decode
 * bits: block k's results go to beta at its first lambda, and *gates counts the prefix once. */
static int run_blocks(const run_ctx *x, int sending, int64_t *beta, unsigned long long *gates) {
    const run_plan *p = x->plan;
    const int n = p->n_blocks, peer = sending ? 2 : 1, ring_slots = p->o->ring_slots;
    lgc_party **blocks = x->blocks;
    int fds[kMaxDevices], got = 0;
    block_job jb[kMaxDevices];
    memset(jb, 0, sizeof jb);
    for (int k = 0; k < n; k++) check(!programs_agree(x->self, peer, blocks[k], sending), "program check failed (block %d)", k);
    if (sending) check(!net_lanes_offer(x->self, 2, n, fds), "could not open %d token connections to the Evaluator", n);
    else check(!net_lanes_accept_offer(x->self, 1, kMaxDevices, &got, fds) && got == n, "the CSP offered %d table links, expected %d (same --devices on both?)", got, n);
    const size_t pre = lgc_party_prefix_launches(blocks[0]);
    for (int k = 0; k < n; k++)
        check(!table_link_open(&jb[k].link, x->self, peer, fds[k], blocks[k], sending, ring_slots, k ? pre : 0), "could not open table link %d", k);
    for (int k = 0; k < n; k++) jb[k].sending = sending;
    jb[0].lo = 0; jb[0].hi = pre;
    block_main(&jb[0]);
    check(!jb[0].rc, sending ? "could not stream the prefix tables" : "could not evaluate the prefix");
    for (int k = 1; k < n; k++) LGC(lgc_party_share_prefix(blocks[k], blocks[0]));
    TRACE(sending ? "prefix garbled and shared" : "prefix evaluated and shared");
    for (int k = 0; k < n; k++) {
        jb[k].lo = pre; jb[k].hi = lgc_party_num_launches(blocks[k]);
        check(!pthread_create(&jb[k].th, NULL, block_main, &jb[k]), "could not start a block thread");
    }
    int bad = 0;
    for (int k = 0; k < n; k++) { pthread_join(jb[k].th, NULL); bad |= jb[k].rc; }
    check(!bad, sending ? "could not stream the garbled tables" : "could not receive garbled tables");
    TRACE(sending ? "tables sent" : "tables evaluated");
    if (sending)
        for (int k = 0; k < n; k++) {
            size_t nr = lgc_party_num_reveal(blocks[k]);
            uint64_t *dec = malloc((nr + 1) * 8);
            LGC(lgc_party_decode_bits(blocks[k], dec));
            check(!send_blob(x->self, 2, dec, nr * 8), "could not send decode bits");
            free(dec);
        }
    /* the rings stay until the Evaluator has evaluated every launch of every block (table_link_finish) */
    for (int k = 0; k < n; k++)
        check(!table_link_finish(&jb[k].link, sending), sending ? "the Evaluator did not release table ring %d" : "could not release table ring %d", k);
    if (sending) {
        g_peer_finished = 1;
        for (int k = 0; k < n; k++) close(fds[k]);
        return 0;
    }
    for (int k = 0; k < n; k++) {
        size_t lo, hi, nr = lgc_party_num_reveal(blocks[k]);
        block_range(p->n_lambdas, (size_t)n, (size_t)k, &lo, &hi);
        uint64_t *dec = malloc((nr + 1) * 8);
        check(!recv_blob(x->self, 1, dec, nr * 8), "could not receive decode bits");
        LGC(lgc_party_finish(blocks[k], dec, beta + lo * p->d, NULL, NULL));
        free(dec);
        /* every block's program holds the prefix; it was garbled once */
        *gates += lgc_party_and_gates(blocks[k]) - (k ? lgc_party_prefix_and_gates(blocks[k]) : 0);
        close(fds[k]);
    }
    g_peer_finished = 1;                                             /* every block's decode bits are in: the CSP may go */
    return 0;
error:
    return 1;
}

/* ----------------------------------------------------------------------------------------------------------- CSP: garbler */
static int run_csp(run_ctx *x) {
    const run_plan *p = x->plan;
    const int P = p->providers, ring_slots = p->o->ring_slots;
    lgc_party *party_obj = x->party_obj;
    node *self = x->self;
    if (!p->n_blocks) {                                              /* the Evaluator maps the ring during the label OT */
        check(!programs_agree(self, 2, party_obj, 1), "program check failed");
        check(!tables_ring_meet(self, 2, party_obj, 1, ring_slots), "could not offer the table ring");
    }
    input_ot_job *jobs = calloc((size_t)P, sizeof *jobs);
    check(jobs != NULL, "out of memory");
    int started_ot = 0, bad_ot = 0;
    for (int k = 3; k <= x->c->num_parties; k++) {                   /* data providers: share k - 3 (linear.oc:31) */
        input_ot_job *j = &jobs[k - 3];
        j->self = self; j->peer = k; j->device = x->device; j->po = party_obj; j->share = (size_t)(k - 3);
        j->bits = lgc_party_input_bits(party_obj);
        j->ring = p->o->input_ring;
        if (pthread_create(&j->th, NULL, input_ot_main, j)) break;
        started_ot++;
    }
    for (int k = 0; k < started_ot; k++) {
        pthread_join(jobs[k].th, NULL);
        if (jobs[k].rc) { fprintf(stderr, "%s\n", jobs[k].err); bad_ot = 1; }
    }
    bad_ot |= started_ot != P;
    free(jobs);
    check(!bad_ot, "input sharing with the data providers failed");
    TRACE("input labels sent");
    if (p->n_blocks) return run_blocks(x, 1, NULL, NULL);
    check(!tables_send(self, 2, party_obj, ring_slots, p->table_chunk), "could not stream the garbled tables");
    TRACE("tables sent");
    size_t nr = lgc_party_num_reveal(party_obj);
    uint64_t *dec = malloc((nr + 1) * 8);
    LGC(lgc_party_decode_bits(party_obj, dec));
    TRACE("decode bits read");
    check(!send_blob(self, 2, dec, nr * 8), "could not send decode bits");
    free(dec);
    g_peer_finished = 1;                                             /* (ring mode: tables_send returned with the ring released) */
    return 0;
error:
    return 1;
}

/* ------------------------------------------------------------------------------------------------------------- Evaluator */
/* what the Evaluator reads back and prints: the one owner of its six buffers */
typedef struct {
    const run_ctx *x;
    int64_t *beta, *ab, *trace;                 /* the result words (plan->result), the revealed A and b, cgd's per-iteration rows */
    uint32_t *mark_launch; uint64_t *mark_gates; double *mark_time;     /* cgd: the launch that completes each iteration */
    double t_ot; unsigned long long gates;
} eval_out;
static void eval_out_free(eval_out *e) {
    free(e->beta); free(e->ab); free(e->trace); free(e->mark_launch); free(e->mark_gates); free(e->mark_time);
}
/* (div: 1, or sqrt(n) for the standard errors -- a division, as it has always been, so that the digits stay what they were) */
static void print_row(const char *label, const int64_t *v, size_t n, int precision, double div) {
    printf("%s", label);
    for (size_t i = 0; i < n; i++) printf("%20.15f ", fixed_to_double(v[i], precision) / div);
    printf("\n");
}
static void print_iterations(const eval_out *e) {                    /* src/cgd.oc:167-194 */
    const lgc_system *sys = &e->x->plan->sys;
    const size_t d = e->x->plan->d;
    const int precision = sys->precision;
    printf("Starting iterations.\n");
    for (int t = 0; t < sys->num_iterations; t++) {
        const int64_t *row = e->trace + (size_t)t * (d + 4);
        printf("Iteration %d (x):\n", t);
        for (size_t i = 0; i < d; i++) printf("%20.15f ", fixed_to_double(row[i], precision));
        printf("\nGamma: %30.20f ", fixed_to_double(row[d], precision));
        printf("\nEta: %30.20f ", fixed_to_double(row[d + 1], precision));
        printf("\nq: %30.20f ", fixed_to_double(row[d + 2], precision));
        printf("\nng: %30.20f ", fixed_to_double(row[d + 3], precision));
        printf("\nIteration %d gate count: %llu", t, (unsigned long long)e->mark_gates[t]);
        printf("\nIteration %d time: %f\n", t, e->mark_time[t]);
    }
}
/* the head of every output form (linreg.c:182-183); cgd's full form prints its iterations inside it, where cgd.oc does */
static void print_header(const eval_out *e, int iterations) {
    printf("Time taken for OT: %f\nOT time: %f\n", e->t_ot, e->t_ot);
    if (iterations) print_iterations(e);
    printf("Time elapsed: %f\n", wall_clock() - e->x->time);
    printf("Number of gates: %llu\n", e->gates);
}
static const char *l1_label(const run_plan *p) { return p->l1_mode == LGC_L1_RATIO ? "L1 ratio" : "L1"; }

static int print_sweep(const eval_out *e) {                          /* one Result line per lambda, in order */
    const run_plan *p = e->x->plan;
    print_header(e, 0);
    for (size_t t = 0; t < p->result.n_results; t++) {
        printf("Lambda: %.17g\n", p->lambdas[t]);
        print_row("Result: ", e->beta + t * p->d, p->result.result_len, p->sys.precision, 1);
    }
    return 0;
}
static int print_cv(const eval_out *e) {                             /* one model: the refit on all rows at the winning value */
    const run_plan *p = e->x->plan;
    const int precision = p->sys.precision, ridge_cv = p->create == RUN_CREATE_RIDGE_CV;
    const double *l1s = p->o->l1.v;
    print_header(e, 0);
    printf("Folds: %zu\n", p->folds);
    if (p->result.off_index != RUN_NO_OFFSET) {
        const int64_t best = lgc_party_selected_index(e->x->party_obj);
        check(best >= 0 && (size_t)best < (ridge_cv ? p->n_lambdas : p->n_path), "the selected index was not revealed");
        if (ridge_cv) printf("Selected index: %lld (lambda: %.17g)\n", (long long)best, p->lambdas[best]);
        else printf("Selected index: %lld (%s: %.17g)\n", (long long)best, l1_label(p), l1s[best]);
        if (p->rule == LGC_CV_RULE_ONE_SE) {                         /* l* beside the l+ the rule selected */
            const int64_t lmin = lgc_party_min_index(e->x->party_obj);
            check(lmin >= 0 && (size_t)lmin < p->n_path, "the minimum's index was not revealed");
            printf("Minimum index: %lld (%s: %.17g)\n", (long long)lmin, l1_label(p), l1s[lmin]);
        }
    }
    if (p->result.off_curve != RUN_NO_OFFSET) {                      /* mean_0 .., then se_0 .. */
        const int64_t *cur = e->beta + p->result.off_curve;
        for (size_t l = 0; l < p->n_path; l++)
            printf("CV curve %zu (%s: %.17g): mean %.15f se %.15f\n", l, l1_label(p), l1s[l], fixed_to_double(cur[l], precision),
                   fixed_to_double(cur[p->n_path + l], precision));
    }
    print_row("Result: ", e->beta, p->result.result_len, precision, 1);
    return 0;
error:
    return 1;
}
/* the M candidates' coefficients and, with --scan_se, behind them the words w_m: the standard error of beta_m is
 * w_m / sqrt(n), in double on the host (n is public), labelled and formatted as --inference prints its own */
static int print_scan(const eval_out *e) {
    const run_plan *p = e->x->plan;
    print_header(e, 0);
    print_row("Result: ", e->beta, p->result.result_len, p->sys.precision, 1);
    if (p->result.off_se != RUN_NO_OFFSET) print_row("Standard errors: ", e->beta + p->result.off_se, p->scan_M, p->sys.precision, sqrt((double)p->n));
    return 0;
}
static int print_full(const eval_out *e) {
    const run_plan *p = e->x->plan;
    const size_t d = p->d, T = d * (d + 1) / 2;
    const int precision = p->sys.precision;
    if (p->sys.reveal_inputs) {                                      /* debug reveal of A and b (src/linear.oc:68-88) */
        printf("A = \n");
        for (size_t i = 0; i < d; i++) {
            for (size_t j = 0; j <= i; j++) printf("%3.8f ", fixed_to_double(e->ab[idx(i, j)], precision));
            printf("\n");
        }
        printf("b = \n");
        for (size_t i = 0; i < d; i++) printf("%3.6f ", fixed_to_double(e->ab[T + i], precision));
        printf("\n");
    }
    print_header(e, p->sys.algorithm == LGC_ALG_CGD);
    for (size_t t = 0; t < p->result.n_results; t++) {               /* a lasso path: one Result line per value */
        if (p->n_path) printf("%s: %.17g\n", l1_label(p), p->o->l1.v[t]);
        print_row("Result: ", e->beta + t * d, p->result.result_len, precision, 1);      /* linreg.c:184-187 */
    }
    if (p->result.off_fit != RUN_NO_OFFSET) {
        /* behind beta: u_0 .. u_{d-1} (without --no_se), then s2 and r2.  The standard error of beta_j is u_j / sqrt(n), in
         * double on the host (n is public); the system is the input's divided by the public normaliser d, and so is s2 */
        const int64_t *fit = e->beta + p->result.off_fit;
        if (p->result.off_se != RUN_NO_OFFSET) print_row("Standard errors: ", e->beta + p->result.off_se, d, precision, sqrt((double)p->n));
        printf("Residual variance: %.15f R^2: %.15f\n", fixed_to_double(fit[0], precision) * (double)d, fixed_to_double(fit[1], precision));
    }
    return 0;
}

static int run_evaluator(run_ctx *x) {
    const run_plan *p = x->plan;
    const lgc_system *sys = &p->sys;
    const int P = p->providers, ring_slots = p->o->ring_slots;
    const size_t d = p->d, T = d * (d + 1) / 2;
    lgc_party *party_obj = x->party_obj;
    node *self = x->self;
    eval_out e;
    int status = 1;
    memset(&e, 0, sizeof e);
    e.x = x;
    double time_start = wall_clock();
    printf("\nAlgorithm: %s\n", p->o->algorithm);
    size_t bits = lgc_party_input_bits(party_obj);
    uint8_t *labels = malloc(bits * 16);
    if (!p->n_blocks) {                                              /* (see the CSP's side) */
        check(!programs_agree(self, 1, party_obj, 0), "program check failed");
        check(!tables_ring_meet(self, 1, party_obj, 0, ring_slots), "could not map the table ring");
    }
    printf("party %d listening for %d inputs", x->c->party, P);
    for (int k = 3; k <= x->c->num_parties; k++) {
        if (p->o->input_ring) {                                      /* the provider's label buffer, mapped; one byte back when it may go */
            uint8_t h[64], tok = 1;
            void *dl = NULL;
            check(!recv_blob(self, k, h, sizeof h), "could not receive the label buffer of party %d", k);
            LGC(lgc_dev_open(x->device, h, &dl));
            int rc_ = lgc_party_set_input_labels_dev(party_obj, (size_t)(k - 3), dl);
            lgc_dev_close(dl);
            check(rc_ == LGC_OK, "%s", lgc_last_error());
            check(!send_blob(self, k, &tok, 1), "could not release party %d", k);
            printf("Evaluator received A from party %d\nEvaluator received b from party %d\n", k, k);
            continue;
        }
        check(!recv_blob(self, k, labels, bits * 16), "could not receive labels from party %d", k);
        LGC(lgc_party_set_input_labels(party_obj, (size_t)(k - 3), labels));
        printf("Evaluator received A from party %d\nEvaluator received b from party %d\n", k, k);
    }
    free(labels);
    labels = NULL;
    TRACE("input labels received");
    e.t_ot = wall_clock() - time_start;
    /* where cgd.oc:190-194 prints yaoGateCount() and the running time: after the launch that
     * completes each iteration */
    size_t n_marks = (sys->algorithm == LGC_ALG_CGD && !p->n_lambdas) ? (size_t)sys->num_iterations : 0;
    e.mark_launch = malloc((n_marks + 1) * sizeof *e.mark_launch);
    e.mark_gates = malloc((n_marks + 1) * sizeof *e.mark_gates);
    e.mark_time = malloc((n_marks + 1) * sizeof *e.mark_time);
    if (n_marks) LGC(lgc_party_iteration_marks(party_obj, e.mark_launch, e.mark_gates, n_marks));
    iter_marks marks = {n_marks, 0, e.mark_launch, e.mark_time, time_start};
    e.beta = malloc(p->result.words * 8); e.ab = malloc((T + d) * 8);
    e.trace = malloc(((size_t)sys->num_iterations * (d + 4) + 1) * 8);
    if (p->n_blocks) {                                               /* the CSP's counterpart, block by block */
        if (run_blocks(x, 0, e.beta, &e.gates)) goto error;
    } else {
        check(!tables_recv(self, 1, party_obj, ring_slots, p->table_chunk, note_launch, &marks), "could not receive garbled tables");
        TRACE("tables evaluated");
        size_t nr = lgc_party_num_reveal(party_obj);
        uint64_t *dec = malloc((nr + 1) * 8);
        check(!recv_blob(self, 1, dec, nr * 8), "could not receive decode bits");
        g_peer_finished = 1;                                         /* the CSP may go: nothing more comes from it */
        LGC(lgc_party_finish(party_obj, dec, e.beta, p->n_lambdas || p->scan_M ? NULL : e.trace,
                             p->n_lambdas || p->folds || p->infer || p->scan_M ? NULL : e.ab));
        free(dec);
        e.gates = lgc_party_and_gates(party_obj);
    }
    status = p->output == RUN_OUT_SWEEP ? print_sweep(&e) : p->output == RUN_OUT_CV ? print_cv(&e)
           : p->output == RUN_OUT_SCAN ? print_scan(&e) : print_full(&e);
error:
    free(labels);
    eval_out_free(&e);
    return status;
}

/* ----------------------------------------------------------------- data provider (linreg.c:192-198, input.c:23-50) */
/* sel[i*intsize+j] = (input[i]>>j)&1 (input.c:41), over the words of this provider's share */
static void fill_choice_bits(const run_ctx *x, uint8_t *sel) {
    const int w2 = x->plan->sys.width;
    for (size_t i = 0; i < x->plan->share_words; i++) {
        uint64_t v = run_share_word(x->plan, x->share_A, x->share_b, x->share_yy, i);
        for (int j = 0; j < w2; j++) sel[i * (size_t)w2 + (size_t)j] = (uint8_t)((v >> j) & 1);
    }
}
static int run_provider(run_ctx *x) {
    const int party = x->c->party, device = x->device;
    const size_t bits = x->plan->share_words * (size_t)x->plan->sys.width;
    node *self = x->self;
    lgc_ot_receiver *R = 0;
    printf("party %d connecting to CSP and Evaluator\n", party);
    uint8_t s0[128][16], s1[128][16];
    check(!baseot_ext_receiver(self, 1, s0, s1), "base OT with the CSP failed");
    TRACE("base OT done");
    printf("party %d connected successfully to CSP and Evaluator\n", party);
    LGC(lgc_ot_receiver_create(&R, device, s0, s1));
    TRACE("input OT: receiver session");
    if (x->plan->o->input_ring) {                                    /* see input_ot_ring_csp */
        const size_t ub = lgc_ot_u_bytes(bits);
        uint8_t *selh = malloc(bits), hue[64], hl[64], tok = 0;
        void *dsel = NULL, *due = NULL, *dl = NULL;
        fill_choice_bits(x, selh);
        LGC(lgc_ot_receiver_set_device_io(R, 1));
        LGC(lgc_dev_alloc(device, bits, &dsel, NULL));
        LGC(lgc_dev_alloc(device, ub + bits * 32, &due, hue));
        LGC(lgc_dev_alloc(device, bits * 16, &dl, hl));
        LGC(lgc_dev_upload(dsel, selh, bits));
        OPENSSL_cleanse(selh, bits); free(selh);
        LGC(lgc_ot_labels_recv_start(R, dsel, bits, due));
        check(!send_blob(self, 1, hue, sizeof hue), "OT: could not hand the buffer to the CSP");
        TRACE("input OT: u sent");
        check(!recv_blob(self, 1, &tok, 1), "OT: the CSP did not answer");
        TRACE("input OT: ciphertexts received");
        LGC(lgc_ot_labels_recv_finish(R, (uint8_t *)due + ub, dl));
        check(!send_blob(self, 2, hl, sizeof hl), "could not hand the labels to the Evaluator");   /* input.c:46 */
        check(!recv_blob(self, 2, &tok, 1), "the Evaluator did not take the labels");
        TRACE("labels forwarded to the Evaluator");
        lgc_ot_receiver_destroy(R);
        lgc_dev_free_secret(dsel, bits); lgc_dev_free(due); lgc_dev_free_secret(dl, bits * 16);
        return 0;
    }
    uint8_t *sel = malloc(bits), *u = malloc(lgc_ot_u_bytes(bits)), *e = malloc(bits * 32), *labels = malloc(bits * 16);
    fill_choice_bits(x, sel);
    LGC(lgc_ot_labels_recv_start(R, sel, bits, u));
    check(!send_blob(self, 1, u, lgc_ot_u_bytes(bits)), "OT: could not send u to the CSP");
    TRACE("input OT: u sent");
    check(!recv_blob(self, 1, e, bits * 32), "OT: could not receive from the CSP");
    TRACE("input OT: ciphertexts received");
    LGC(lgc_ot_labels_recv_finish(R, e, labels));
    check(!send_blob(self, 2, labels, bits * 16), "could not forward labels to the Evaluator");   /* input.c:46 */
    TRACE("labels forwarded to the Evaluator");
    lgc_ot_receiver_destroy(R);
    free(sel); free(u); free(e); free(labels);
    return 0;
error:
    return 1;
}

/* ------------------------------------------------------------------------------------------------------------------ main */
int main(int argc, char **argv) {
    config *c = NULL;
    node *self = NULL;
    lgc_party *blocks[kMaxDevices] = {0};       /* --devices: blocks[0] == x.party_obj */
    int n_blocks = 0, status;
    const char *msg;
    run_opts o;
    run_plan plan;
    run_ctx x;
    create_job cj;
    memset(&plan, 0, sizeof plan);
    memset(&x, 0, sizeof x);
    memset(&cj, 0, sizeof cj);

    /* the command line: scan, the reference's line about phase 2's precision, the rule book */
    msg = run_opts_scan(&o, argc, argv);
    if (o.party_read) {
        char tag_[16];
        snprintf(tag_, sizeof tag_, "p%d", o.party);
        lgc_trace_set_tag(tag_);
        lgc_trace_mark("main entered");
    }
    check(!msg, "%s", msg);
    protocol_set_table_lanes(o.table_lanes);
    if (o.prec_phase2 != -1) printf("Using different precision for phase 2 (%i)\n", o.prec_phase2);
    msg = run_opts_check(&o);
    check(!msg, "%s", msg);
    const int party = o.party;
    int device = getenv("LINREG_DEVICE") ? atoi(getenv("LINREG_DEVICE")) : 0;
    n_blocks = run_opts_blocks(&o);
    if (n_blocks && party <= 2) {
        /* before anything is allocated: every index exists, and distinct devices can reach each other (the shared prefix
         * travels by peer copy, lgc_party_share_prefix; the Evaluator maps the CSP's table rings over hipIpc) */
        check(lgc_devices_preflight(o.devices, (size_t)n_blocks) == LGC_OK, "--devices: %s", lgc_last_error());
        device = o.devices[0];
    }

    /* HIP runtime + device context (60-150 ms with four or five processes starting at once): on a thread, beside the
     * configuration file, the socket mesh and a data provider's parsing of its columns */
    static int warm_device;
    pthread_t warm_th;
    warm_device = device;
    /* the code objects this party will launch from, and streams for its OT sessions: data providers run phase 1 and the label
     * OT, the CSP is the initializer (phase-1 kernels) and the label-OT sender; the Evaluator's kernels come with its program */
    g_warm_what = party == 2 ? 0 : 3;   /* (no pooled streams: every extra hardware queue costs ~60 ms when four processes tear down at once) */
    int warm_started = pthread_create(&warm_th, NULL, warm_main, &warm_device) == 0;
    if (warm_started) pthread_detach(warm_th);

    /* the configuration, and with it the plan of the run: known before any protocol message */
    status = config_new(&c, o.input);
    check(!status, "Could not read config");
    c->party = party;
    check(party >= 1 && party <= c->num_parties, "Party must be in 1..%d", c->num_parties);
    msg = run_plan_build(&plan, &o, c->n, c->d, c->num_parties, device);
    check(!msg, "%s", msg);
    lgc_trace_mark("configuration read");
    x.c = c; x.plan = &plan; x.device = device; x.blocks = blocks;
    x.time = wall_clock();
    if (party == 2) printf("{\"n\":\"%zd\", \"d\":\"%zd\" \"p\":\"%d\"}\n", c->n, c->d, c->num_parties - 1);

    status = node_new(&self, party, c->num_parties, c->endpoint);
    check(!status, "Could not create node");
    x.self = self;
    TRACE("connected");
    static watchdog_arg wd;
    if (party <= 2) {                                                /* parties 1 and 2 watch each other's connection */
        pthread_t wt;
        wd.fd = self->fd[(3 - party) - 1]; wd.party = party; wd.peer = 3 - party;
        if (wd.fd >= 0 && !pthread_create(&wt, NULL, peer_watchdog, &wd)) pthread_detach(wt);
    }

    /* phase 1, and beside it the creation of the phase-2 object */
    cj.plan = &plan; cj.blocks = blocks;
    cj.role = party == 1 ? LGC_ROLE_GARBLER : LGC_ROLE_EVALUATOR;
    if (party == 1) {
        /* the garbler of phase 2 is built while this process is the trusted initializer (TI mode) or idle (OT mode) */
        check(!pthread_create(&cj.th, NULL, create_main, &cj), "could not start the garbler's creation thread");
        cj.started = 1;
        if (!p1_mode_is_ot(&plan.job.mode)) {
            status = run_trusted_initializer(self, c, &plan.job);
            check(!status, "Error while running trusted initializer");
        }
    } else if (party > 2) {
        status = run_party(self, c, &plan.job, &x.share_A, &x.share_b, &x.share_yy);
        check(!status, "Error while running party %d", party);
    } else {
        /* The Evaluator has no part in phase 1: it brings up its GPU context, program and buffers while the data
         * providers work, instead of after the barrier with the CSP waiting for it (0.3 s of a 0.9 s config-3 run). */
        create_main(&cj);
        check(!cj.rc, "%s", cj.err);
        x.party_obj = cj.party_obj;
    }
    TRACE("phase 1 done");
    check(!net_barrier(self), "Error while waiting for other peers to finish");
    TRACE("barrier");
    printf("Party %d finished phase 1\n", party);

    /* phase 2 */
    if (party == 1) {
        pthread_join(cj.th, NULL);
        cj.started = 0;
        check(!cj.rc, "%s", cj.err);
        x.party_obj = cj.party_obj;
        check(!create_rings(&cj), "%s", cj.err);
    }
    if (party == 1 ? run_csp(&x) : party == 2 ? run_evaluator(&x) : run_provider(&x)) goto error;

    g_protocol_over = 1;
    TRACE("protocol done");
    for (int k = 1; k < n_blocks; k++) if (blocks[k]) lgc_party_destroy(blocks[k]);
    if (x.party_obj) lgc_party_destroy(x.party_obj);       /* (wipes label material before its memory is released) */
    node_destroy(&self);
    config_destroy(&c);
    free(x.share_A);
    free(x.share_b);
    free(x.share_yy);
    run_plan_free(&plan);
    run_opts_free(&o);
    g_protocol_over = 2;
    TRACE("exit");
    /* (leaving through _exit() to skip the HIP runtime's exit handlers -- 70-80 ms per process -- was measured and is WORSE:
     * the kernel driver then tears the process's queues and mappings down by itself, 250 ms for config 2) */
    return 0;
error:
    if (cj.started) { pthread_join(cj.th, NULL); if (!x.party_obj) x.party_obj = cj.party_obj; }
    for (int k = 1; k < n_blocks; k++) if (blocks[k]) lgc_party_destroy(blocks[k]);
    if (x.party_obj) lgc_party_destroy(x.party_obj);
    config_destroy(&c);
    node_destroy(&self);
    free(x.share_A);
    free(x.share_b);
    free(x.share_yy);
    g_protocol_over = 2;
    return 1;
}
