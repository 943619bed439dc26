/* phase1_plan.c -- see phase1_plan.h */
#include <stdlib.h>
#include "phase1_plan.h"

const char *p1_mode_check(const p1_flags *f) {
    const int use_ot = f->use_ot || f->ot_ring;
    /* --ti_matrix: the initializer's protocol with one matrix triple per provider pair */
    if (f->ti_matrix && f->ot_ring) return "--ti_matrix and --ot_ring exclude each other";
    if (f->ti_matrix && use_ot) return "--ti_matrix and --use_ot exclude each other (it is a mode of the trusted initializer)";
    if (f->ti_matrix && f->ti_ring) return "--ti_matrix and --ti_ring exclude each other";
    if (f->ti_matrix && f->scan) return "--ti_matrix and --scan exclude each other";
    /* --ot_matrix: the OT mode with one vector OT per bit of the receiver's operand; --ot_half inherits its exclusions */
    if (f->ot_half && !(use_ot && f->ot_matrix)) return "--ot_half needs --use_ot --ot_matrix";
    if (f->ot_matrix && f->ot_ring) return "--ot_matrix and --ot_ring exclude each other";
    if (f->ot_matrix && !use_ot) return "--ot_matrix needs --use_ot (it is a mode of the OT-based phase 1)";
    if (f->ot_matrix && f->scan) return "--ot_matrix and --scan exclude each other";
    return NULL;
}

p1_transport p1_transport_of(const p1_flags *f) {
    if (f->ot_half) return P1_OT_HALF;
    if (f->ot_matrix) return P1_OT_MATRIX;
    if (f->ot_ring) return P1_OT_RING;
    if (f->use_ot) return P1_OT_PAIRS;
    if (f->ti_matrix) return P1_TI_MATRIX;
    return f->ti_ring ? P1_TI_RING : P1_TI_SOCKETS;
}

const char *p1_mode_refuses(const p1_mode *m) {
    const int ring = m->transport == P1_TI_RING || m->transport == P1_OT_RING;
    const int matrix = m->transport == P1_TI_MATRIX || m->transport == P1_OT_MATRIX || m->transport == P1_OT_HALF;
    if (ring && m->folds) return "--folds excludes --ti_ring and --ot_ring";
    if (m->scan && (ring || matrix || m->folds)) return "--scan excludes --folds, --ti_ring, --ot_ring, --ti_matrix and --ot_matrix";
    return NULL;
}

/* Each order is written once (ti_order, ot_order): with no list to fill it only counts, so a count and its list cannot disagree,
 * and every list is allocated at exactly its size */
static size_t ti_order(const int *owner, size_t d, size_t M, p1_pair *v) {
    size_t np = 0;
    for (size_t i = 0; i <= d; i++)
        for (size_t j = 0; j <= i && j < d; j++) {
            if (owner[i] == owner[j] || scan_skips(d, M, i, j)) continue;
            const p1_pair p = {owner[i], owner[j], (uint32_t)i, (uint32_t)j};
            if (v) v[np] = p;
            np++;
        }
    return np;
}
size_t p1_plan_ti(const int *owner, size_t d, size_t M, p1_pair **out) {
    const size_t np = ti_order(owner, d, M, NULL);
    *out = NULL;
    if (!np) return 0;
    if (!(*out = malloc(np * sizeof **out))) return (size_t)-1;
    return ti_order(owner, d, M, *out);
}

int p1_pair_view(const p1_pair *p, int me, p1_view *v) {
    if (p->pa != me && p->pb != me) return 0;
    v->is_a = p->pa == me;
    v->peer = v->is_a ? p->pb : p->pa;
    v->col = v->is_a ? p->ci : p->cj;
    return 1;
}

static size_t ot_order(size_t d, size_t M, size_t i0, size_t i1, int y_on_sender, size_t j0, size_t j1, int y_on_receiver,
                       size_t *ri, size_t *rj) {
    size_t q = 0;
#define PAIR(i, j) do { if (ri) { ri[q] = (i); rj[q] = (j); } q++; } while (0)
    for (size_t i = i0; i < i1; i++) {
        for (size_t j = j0; j < j1; j++) if (!scan_skips(d, M, i, j)) PAIR(i, j);
        if (y_on_receiver) PAIR(i, d);
    }
    if (y_on_sender) for (size_t j = j0; j < j1; j++) PAIR(d, j);
#undef PAIR
    return q;
}
size_t p1_plan_ot(size_t d, size_t M, size_t i0, size_t i1, int y_on_sender, size_t j0, size_t j1, int y_on_receiver,
                  size_t **ri, size_t **rj) {
    const size_t np = ot_order(d, M, i0, i1, y_on_sender, j0, j1, y_on_receiver, NULL, NULL);
    *ri = *rj = NULL;
    if (!np) return 0;
    *ri = malloc(np * sizeof **ri); *rj = malloc(np * sizeof **rj);
    if (!*ri || !*rj) { free(*ri); free(*rj); *ri = *rj = NULL; return (size_t)-1; }
    return ot_order(d, M, i0, i1, y_on_sender, j0, j1, y_on_receiver, *ri, *rj);
}

static size_t clamp(size_t v, size_t lo, size_t hi) { return v < lo ? lo : v > hi ? hi : v; }
size_t p1_ti_batch_pairs(size_t n) { return clamp(((size_t)64 << 20) / (n * 8), 1, 1024); }
/* a batch costs every party a fixed ~0.5 ms of tokens and device synchronisations whatever its size, and config 4 has 1e5 pairs of
 * 5e4 words -- with 64 MiB slots (167 pairs, 602 batches; rounds 2-3) its phase 1 was 0.55 s of which two thirds were those
 * fixed costs */
size_t p1_ring_batch_pairs(size_t n) { return clamp(((size_t)256 << 20) / (n * 8), 1, 1024); }
/* at most 2^24 OTs (256 MiB of u) per batch, two in flight on the receiver side.  Measured on config 3 (1.6e9 OTs between two
 * provider processes on one GPU, scripts/exp/ot_batch_ab.sh): phase 1 through at 0.46 s with 2^24, 0.58 s with 2^25 (rounds 2-3),
 * 0.8 / 1.2 / 2.2 s with 2^26..28 -- the session's buffers grow with the batch and a fresh device or page-locked allocation
 * costs more than the per-batch tokens do */
size_t p1_ot_batch_pairs(size_t n, int w, size_t npairs) {
    const size_t per = ((size_t)1 << 24) / (n * (size_t)w);
    return per < 1 ? 1 : per > npairs ? npairs : per;
}
