/* phase1_plan.h -- the pure-host part of phase 1's host side: the mode a run is in, the one rule book that says which options
 * go together, the cross-party pairs in the two orders the protocols walk them, and the batch rules of the per-pair transports.
 * No GPU, no sockets, no globals: the initializer and every provider derive the same plan from the column ownership and the mode
 * alone, which is what keeps the streams of all sockets aligned.  tests/tools/asan_phase1_plan.c runs it under the sanitizers. */
#ifndef LINREG_PHASE1_PLAN_H
#define LINREG_PHASE1_PLAN_H
#include <stddef.h>
#include <stdint.h>

/* ---------------------------------------------------------------- the mode */
typedef enum {
    P1_TI_SOCKETS,      /* the trusted initializer's protocol over sockets (the default) */
    P1_TI_RING,         /* --ti_ring: that protocol with all parties on one node, vectors through device rings */
    P1_TI_MATRIX,       /* --ti_matrix: one matrix triple per provider pair (include/linreg_gc_p1_matrix.h) */
    P1_OT_PAIRS,        /* --use_ot: one Gilboa product per pair of columns */
    P1_OT_RING,         /* --ot_ring: that mode with u / y of the extension in device rings */
    P1_OT_MATRIX,       /* --use_ot --ot_matrix: one vector OT per operand bit (include/linreg_gc_ot_matrix.h) */
    P1_OT_HALF          /* ... --ot_half: its half-payload form (include/linreg_gc_ot_half.h) */
} p1_transport;
typedef struct {
    p1_transport transport;
    size_t scan;        /* --scan=M: the last M feature columns are candidates (include/linreg_gc_scan.h); 0: none */
    size_t folds;       /* --folds=K: phase 1 once per row fold (include/linreg_gc_folds.h); 0: the whole file */
} p1_mode;
static inline int p1_mode_is_ot(const p1_mode *m) { return m->transport >= P1_OT_PAIRS; }

/* what a command line set, before it is known to make a mode: --use_ot --ti_matrix has to be sayable to be refused.  --ot_ring
 * implies --use_ot.  scan / folds: whether the option was given */
typedef struct { int use_ot, ot_ring, ti_ring, ti_matrix, ot_matrix, ot_half, scan, folds; } p1_flags;
/* the message of the first rule the flags break, or NULL.  The rules are those between the phase-1 transports and of --scan with
 * the matrix modes; what --folds, --scan and --inference exclude beyond phase 1 (--devices, --lambdas, --input_ring, and the ring
 * transports with them) is bin/linreg's to say, and the mode does not depend on folds */
const char *p1_mode_check(const p1_flags *f);
/* the transport of flags that passed p1_mode_check (--use_ot wins over --ti_ring, as it always has) */
p1_transport p1_transport_of(const p1_flags *f);
/* what no caller may ask of run_party / run_trusted_initializer, as a message, or NULL: the ring transports move whole files in
 * the full loop order (no --folds, no --scan); the matrix transports know no --scan.  bin/linreg says all of this earlier */
const char *p1_mode_refuses(const p1_mode *m);

/* what run_party / run_trusted_initializer are told beyond the configuration file (protocol.h says what each field asks of them) */
typedef struct {
    int precision, precision_p2;    /* fractional bits in phase 1 / phase 2 */
    int w1, w2;                     /* word widths of the two phases: 32 or 64 */
    int device;
    p1_mode mode;
    int want_yy;
} p1_job;

/* --scan: no model holds two candidate columns, so every side leaves the pairs (i, j) of two different candidates out of its
 * loops, in the same loop order */
static inline int scan_skips(size_t d, size_t M, size_t i, size_t j) { return M && i < d && j < d && i != j && i >= d - M && j >= d - M; }

/* ---------------------------------------------------------------- the cross-party pairs
 * owner[i], i <= d: the 0-based party index that holds column i (column d is y); non-decreasing in i (config_owner). */
typedef struct { int pa, pb; uint32_t ci, cj; } p1_pair;   /* pa = owner[ci] > pb = owner[cj]; ci <= d, cj < d, cj <= ci */
/* the initializer's loop order (src/phase1.c:256-258): for i <= d, for j <= i and j < d, owners differ, not skipped by the scan.
 * Every TI socket carries its party's pairs in this order.  Returns the count and the list in *out (malloc'd, free();
 * NULL when there is no pair), or (size_t)-1 when out of memory */
size_t p1_plan_ti(const int *owner, size_t d, size_t M, p1_pair **out);
/* a provider's view of one pair: 0 when the pair is not `me`'s.  is_a: `me` holds the higher column (party a of
 * inner_product_ti); col: its own column of the pair.  Since owner[] is monotone, is_a is the same for every pair with one peer */
typedef struct { int peer, is_a; uint32_t col; } p1_view;
int p1_pair_view(const p1_pair *p, int me, p1_view *v);

/* the OT modes' block order for one provider pair: the sender's columns [i0, i1) against the receiver's [j0, j1), then the
 * sender's column against y where the receiver holds it, row by row; last y against the receiver's columns where the sender
 * holds it.  ri / rj: the sender's / receiver's column of each pair (d: y), malloc'd (free()).  Returns the count (0: nothing
 * allocated), or (size_t)-1 when out of memory */
size_t p1_plan_ot(size_t d, size_t M, size_t i0, size_t i1, int y_on_sender, size_t j0, size_t j1, int y_on_receiver,
                  size_t **ri, size_t **rj);
/* of providers me and peer (0-based party indices), which is the OT sender (src/phase1.c:392) */
static inline int p1_ot_i_am_sender(int me, int peer) { return (me % 2 == peer % 2) == (me < peer); }

/* ---------------------------------------------------------------- pairs per batch, n rows each */
size_t p1_ti_batch_pairs(size_t n);                            /* TI over sockets: about 64 MiB of x (and of y), 1..1024 pairs */
size_t p1_ring_batch_pairs(size_t n);                          /* --ti_ring: 256 MiB per ring slot, 1..1024 pairs */
size_t p1_ot_batch_pairs(size_t n, int w, size_t npairs);      /* --use_ot per pair: 2^24 OTs (n w per pair), 1..npairs pairs */
#endif
