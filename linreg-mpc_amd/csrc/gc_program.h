// gc_program.h -- host-side lowering of the phase-2 solvers to launches of
// word-machine records (no device code here).
//
// Follows, statement by statement:
//   input assembly  src/linear.oc:10-94 (data providers) / :96-135 (two-party)
//   cgd             src/cgd.oc:96-212
//   cholesky        src/cholesky.oc:51-93
//   ldlt            src/ldlt.oc:50-90
// Wrap-around additions are re-associated freely (tree / carry-save sums):
// addition mod 2^w is associative, so results are identical.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <tuple>
#include <utility>
#include <vector>

#include "gc_exec.h"

namespace gc {

static const size_t kMinRecsPerLaunch = 8192;   // >= 2x the chip's resident waves (256 CUs x 12-16)
// Largest launch of the co-located solver, in gate steps (2 KiB of garbled table each): 2^25 = 64 GiB of tables.  A MAC
// launch runs in whole rounds of the chip (one workgroup per CU: 4096 garbler / 3072 evaluator records per round), so the
// fewer launches a matrix-vector product is cut into, the less is lost to partly filled last rounds: with 2^23 the d = 500
// product (27.5 M steps with Karatsuba records) fell into four launches of 3.81 / 5.09 rounds -- the evaluator ran six
// rounds for five rounds of work -- with 2^25 it is ONE launch.  (Round 4: with records of one Karatsuba pair a launch is tens
// of rounds and the partly filled last round no longer matters, but every launch still pays ~1 ms of ramp-up and tail, and
// smaller launches measured slower: d = 500 CGD-15 1.81 s at 2^25, 1.87 at 2^24, 1.93 at 2^23; scripts/exp/mac_ab.sh cap*.)
// The table ring is the largest launch plus kRingSlackBytes: 64 of the 288 GB of an MI355X at d = 500.
#ifndef GC_DEFAULT_CAP_LOG2
#define GC_DEFAULT_CAP_LOG2 25
#endif
static const uint64_t kDefaultCapSteps = 1ull << GC_DEFAULT_CAP_LOG2;
// ... a merged sweep program is cut into equal pieces by the same cap (replicate_program).  Rounds 3 - 4 used 2^24 there, so
// that the ring of a sweep block (32 + 8 GiB) fitted the one a d = 500 solver leaves parked; but every launch pays ~1 ms of
// ramp-up and tail (all workgroups start in lock step, the last ones leave CUs idle), and a 64-circuit block has 90 such
// launches: 2^25 halves them -- 6.27 -> 6.00 s for the 64-lambda block (scripts/exp/sweep_cap_ab.sh); blocks of <= 16 circuits
// fit one launch per product either way.
#ifndef GC_SWEEP_CAP_LOG2
#define GC_SWEEP_CAP_LOG2 25
#endif
static const uint64_t kSweepCapSteps = 1ull << GC_SWEEP_CAP_LOG2;
static const uint64_t kGenericCapSteps = 1ull << 24;     // launches other than MAC launches (Program::emit)
static const size_t kRingSlackBytes = (size_t)8 << 30;
// ... adjustable (lgc_set_table_ring_slack): eight ranks rehearsing an 8-GPU sweep on ONE GPU must fit its HBM together
inline size_t &ring_slack_bytes() { static size_t v = kRingSlackBytes; return v; }

struct Launch {
    uint32_t first_rec, nrec;   // slice of Program::recs
    uint64_t step0, steps;      // gate steps covered
    uint64_t gates;             // active AND gates
    bool mac_only;
    bool mack;                  // mac_only launch whose records are OP_MACK (Karatsuba products: a kernel of their own)
    uint8_t force[2] = {0, 0};  // garbler, evaluator: the LaunchMode a test program forces (gc_launch.h); 0 = by record count
};

enum { SELECT_REVEAL_INDEX = 1, SELECT_REVEAL_SCORES = 2 };   // LGC_SELECT_REVEAL_* (linreg_gc_lasso_select.h)
enum { SELECT_REVEAL_CURVE = 4 };                             // LGC_SELECT_REVEAL_CURVE (linreg_gc_lasso_cv_se.h)
enum { CV_RULE_MIN = 0, CV_RULE_ONE_SE = 1 };                 // LGC_CV_RULE_* (linreg_gc_lasso_cv_se.h)
enum { INFER_SE = 1, INFER_FIT = 2 };                          // LGC_INFER_* (linreg_gc_inference.h)
enum { SCAN_SE = 1 };                                         // LGC_SCAN_SE (linreg_gc_scan.h)
enum Alg { ALG_CHOLESKY = 0, ALG_LDLT = 1, ALG_CGD = 2, ALG_DIMCHECK = 3, ALG_LASSO = 4 };

struct Program {
    int w, p;
    size_t d, T, nshares;
    std::vector<Rec> recs;
    std::vector<Launch> launches;
    uint32_t n_words;            // word file size
    uint32_t n_reveal;           // decode slots
    uint32_t in_base;            // first input word: nshares x (T + targets * d), share-major
    uint32_t rv_beta;            // decode slot of beta[0]
    uint32_t rv_trace;           // decode slot of trace[0] (cgd: iters x (d+4), lasso: iters x d), or ~0u
    uint32_t rv_ab;              // decode slot of the debug reveal of a, b (T + d), or ~0u
    uint64_t total_steps, total_gates;
    uint64_t total_xors = 0;     // flat-list XOR gates (rec_cost): reporting only
    uint64_t max_launch_steps;
    // cgd: per iteration, the last launch of the iteration and the AND gates emitted up to there
    // (the points where cgd.oc:190-194 prints yaoGateCount() and the running time)
    std::vector<uint32_t> iter_launch;
    std::vector<uint64_t> iter_gates;
    // lambda sweep (replicate_program): `replicas` copies of one circuit in one program; copy t
    // uses words x + t * word_stride (x != 0) and decode slots r + t * reveal_stride
    uint32_t replicas, word_stride, reveal_stride;
    uint32_t lam_rec;            // index of the OP_CONST record holding lambda, or ~0u
    // shared prefix of a sweep (data-provider path): words [0, shared_end) -- the constant zero, the input
    // words and the share sums -- and the launches [0, prefix_launches) that produce the sums are the same
    // for every lambda (lambda enters after them, linear.oc:52-57): garbled once, shared by all circuits
    uint32_t shared_end, prefix_launches;
    uint64_t prefix_steps;
    // right-hand sides of one solve (build_program's `targets`): b_0 .. b_{k-1} follow A in every share, beta is k x d,
    // target-major.  A is factored (or multiplied) once; target t runs the operations of a solve with b = b_t
    size_t targets;
    // input words per share: A, then b_0 .. b_{k-1}; with a validation system (below) then A_v and b_v
    size_t in_words() const {
        if (scan) return (d - 1) * d / 2 + d + scan * (d + 1);      // [A (T_c)] [b (c)] [yy] [h (M c)] [gg (M)] [gy (M)], c = d - 1
        return folds ? folds * (T + d) + (yy ? folds : 0) : (T + targets * d) * (validate ? 2 : 1) + (infer ? 1 : 0);
    }
    // lasso path (lower_lasso): L values of lambda1 on the one M and b; beta is L x d, lambda-major
    size_t path = 1;
    // model selection on a hold-out (Spec::validate): every share carries a second system, the path's models are scored on
    // it inside the circuit and only the best is revealed -- beta* (d words), then its index (SELECT_REVEAL_INDEX: one
    // word), then the L scores (SELECT_REVEAL_SCORES), in consecutive decode slots from rv_beta
    bool validate = false;
    int select_reveal = 0;
    // K-fold cross-validation of a lasso path (Spec::folds): every share carries K fold systems, K + 1 paths are fitted side
    // by side (on all folds but k, and on all of them), the K scores of every value are summed and only the full-data model
    // at the best value is revealed, laid out as the selection's
    size_t folds = 0;
    // the one-standard-error rule (Spec::yy, Spec::cv_rule; linreg_gc_lasso_cv_se.h): every share ends with K words yy_k, the
    // curve (mean_l, se_l) of the per-fold errors is formed in the circuit and beta+ is the refit at l+, the first value in
    // `order` (the values by decreasing penalty, public) whose mean is within one standard error of the minimum's.  Revealed:
    // beta+, then l+ and l* (SELECT_REVEAL_INDEX; CV_RULE_MIN: l* alone), the scores, then the curve (SELECT_REVEAL_CURVE)
    bool yy = false;
    int cv_rule = CV_RULE_MIN;
    std::vector<uint32_t> order;
    bool selects() const { return validate || folds != 0; }
    // K-fold cross-validation of the ridge lambda sweep (build_ridge_cv, linreg_gc_ridge_cv.h): `folds` and `path` (the L values
    // of lambda) as for the lasso, `cv_circuits` merged single-solve circuits (replicate_program) and a scoring and selection
    // tail behind them.  keep_beta: the single-solve circuit leaves beta in its words (beta_at) instead of revealing it
    bool ridge_cv = false, keep_beta = false;
    int ridge_alg = 0;
    uint32_t cv_circuits = 0, beta_at = 0;
    // inference on the Cholesky solve (Spec::infer, linreg_gc_inference.h): every share is [A (T)] [b (d)] [yy (1)]; behind beta
    // the program reveals u_0 .. u_{d-1} (INFER_SE), then s2 and r2 (INFER_FIT).  resid_fixed: q(resid_scale), a public constant
    int infer = 0;
    uint64_t resid_fixed = 0;
    // an association scan (Spec::scan, linreg_gc_scan.h): `scan` candidate columns, each fitted with the d - 1 shared covariates
    // in a system of size d; revealed: the scan coefficients, then (scan_bits & SCAN_SE) the scan words w_m.  resid_fixed as above
    size_t scan = 0;
    int scan_bits = 0;
    size_t infer_words() const { return ((infer & INFER_SE) ? d : 0) + ((infer & INFER_FIT) ? 2 : 0); }
    size_t index_words() const { return (select_reveal & SELECT_REVEAL_INDEX) ? (cv_rule == CV_RULE_ONE_SE ? 2 : 1) : 0; }
    size_t beta_words() const {
        if (selects()) return d + index_words() + ((select_reveal & SELECT_REVEAL_SCORES) ? path : 0) + ((select_reveal & SELECT_REVEAL_CURVE) ? 2 * path : 0);
        if (scan) return scan * ((scan_bits & SCAN_SE) ? 2 : 1);
        return targets * path * d + infer_words();
    }

    // ---- builder state
    size_t merge_hint = 1;       // this program will be replicated this many times (replicate_program): the dot products of
                                 // ONE circuit then need only 1 / merge_hint of the records that fill the chip
    uint64_t cap_steps;          // split launches above this many steps
    uint64_t step_cursor;
    std::map<std::pair<uint32_t, uint32_t>, std::pair<uint64_t, uint64_t>> cost_cache;
    std::map<std::pair<uint32_t, uint32_t>, uint64_t> xor_cache;
    bool open;

    Program() : w(64), p(56), d(0), T(0), nshares(0), n_words(1), n_reveal(0), in_base(0), rv_beta(0),
                rv_trace(~0u), rv_ab(~0u), total_steps(0), total_gates(0), max_launch_steps(0),
                replicas(1), word_stride(0), reveal_stride(0), lam_rec(~0u), shared_end(1), prefix_launches(0),
                prefix_steps(0), targets(1), cap_steps(kDefaultCapSteps), step_cursor(0), open(false) {}

    // (words64: the word count without the wrap of 32-bit ids; a cross-validation past kMaxWords is marked `overflow` --
    // OP_PROX's pair offset is a signed field -- and so is an inference program, whose inverse columns and their shadow double
    // the word file; every other program is what it has always been)
    static constexpr uint64_t kMaxWords = 1ull << 31;
    uint64_t words64 = 1;
    uint32_t alloc(size_t n) {
        uint32_t r = n_words;
        n_words += (uint32_t)n;
        words64 += n;
        if ((folds || infer || scan) && words64 >= kMaxWords) overflow = true;
        return r;
    }
    uint32_t alloc_reveal(size_t n) { uint32_t r = n_reveal; n_reveal += (uint32_t)n; return r; }

    // (op, cnt) of the record costed last and its figures: consecutive records are mostly of one kind, and a merged sweep
    // emits millions of them (two map lookups per record were most of the 0.2-0.3 s a 64-circuit program took to build)
    uint32_t memo_op = ~0u, memo_cnt = 0;
    uint64_t memo_steps = 0, memo_gates = 0, memo_xors = 0;
    static constexpr uint32_t kVariantKey = 0x100u;
    void cost(const Rec &r, uint64_t &steps, uint64_t &gates) {
        if (r.op == OP_PROX) { prox_cost(r, steps, gates); return; }
        if (r.op == OP_STEPEXP && r.cnt == 2) { ratio_cost(r, steps, gates); return; }
        // cost depends on (op, cnt) only -- for OP_IDIVC (cnt is 1) on the divisor: its multiplier's set bits are the steps
        const uint32_t cnt = r.op == OP_IDIVC ? r.c : r.cnt;
        // ... and on the variant: the signed minimum (OP_MAX, b = 2) and the gated select (OP_SUM, b != 0) have keys of their
        // own; the first-match one-hot (OP_EQ, cnt >= 2) differs from the comparison (cnt = 1) by its cnt
        const uint32_t kop = r.op | (((r.op == OP_MAX && r.b == 2) || (r.op == OP_SUM && r.b)) ? kVariantKey : 0u);
        if (kop == memo_op && cnt == memo_cnt) { steps = memo_steps; gates = memo_gates; return; }
        std::pair<uint32_t, uint32_t> key(kop, cnt);
        auto it = cost_cache.find(key);
        if (it == cost_cache.end()) {
            uint64_t s, g, x = 0;
            rec_cost(r, w, p, s, g, &x);
            it = cost_cache.insert(std::make_pair(key, std::make_pair(s, g))).first;
            xor_cache[key] = x;
        }
        steps = it->second.first;
        gates = it->second.second;
        memo_op = kop; memo_cnt = cnt; memo_steps = steps; memo_gates = gates; memo_xors = xor_cache[key];
    }

    // OP_PROX: the cost depends on the 64-bit momentum constant (b | cnt << 32; cnt's bit 31 marks a bounded record, which
    // then has an entry of its own) and on whether the record forms hdiff (sb)
    std::map<std::pair<uint64_t, bool>, std::pair<std::pair<uint64_t, uint64_t>, uint64_t>> prox_cache;
    void prox_cost(const Rec &r, uint64_t &steps, uint64_t &gates) {
        const std::pair<uint64_t, bool> key((uint64_t)r.b | ((uint64_t)r.cnt << 32), r.sb != 0);
        auto it = prox_cache.find(key);
        if (it == prox_cache.end()) {
            uint64_t s, g, x = 0;
            rec_cost(r, w, p, s, g, &x);
            it = prox_cache.insert(std::make_pair(key, std::make_pair(std::make_pair(s, g), x))).first;
        }
        steps = it->second.first.first;
        gates = it->second.first.second;
        memo_op = ~0u;                                   // (the (op, cnt) memo stays valid for its own key only)
        memo_xors = it->second.second;
    }

    // OP_STEPEXP with cnt = 2: the cost depends on the ratio r (sa | sb << 32), a Circ::mulc of popcount(r) shifted copies
    std::map<uint64_t, std::pair<std::pair<uint64_t, uint64_t>, uint64_t>> ratio_cache;
    void ratio_cost(const Rec &r, uint64_t &steps, uint64_t &gates) {
        const uint64_t key = (uint64_t)(uint32_t)r.sa | ((uint64_t)(uint32_t)r.sb << 32);
        auto it = ratio_cache.find(key);
        if (it == ratio_cache.end()) {
            uint64_t s, g, x = 0;
            rec_cost(r, w, p, s, g, &x);
            it = ratio_cache.insert(std::make_pair(key, std::make_pair(std::make_pair(s, g), x))).first;
        }
        steps = it->second.first.first;
        gates = it->second.first.second;
        memo_op = ~0u;
        memo_xors = it->second.second;
    }

    void new_launch() { open = false; }

    void emit(Rec r) {
        uint64_t s, g;
        cost(r, s, g);
        bool mac = (r.op == OP_MAC || r.op == OP_MAC2 || r.op == OP_MACK);
        const bool mack = r.op == OP_MACK;
        // the table cap is for the MAC launches (fewer, larger launches: kDefaultCapSteps); every other launch is cut at
        // kGenericCapSteps as in rounds 1-4 -- the input division of an 8-circuit sweep block is 18.7 M steps, and as ONE
        // launch it would set the size of the block's table ring (36 GiB instead of 18)
        const uint64_t cap_here = mac || cap_steps < kGenericCapSteps ? cap_steps : kGenericCapSteps;
        if (!open || launches.back().steps + s > cap_here || launches.back().mac_only != mac || launches.back().mack != mack) {
            Launch L;
            L.first_rec = (uint32_t)recs.size();
            L.nrec = 0;
            L.step0 = step_cursor;
            L.steps = 0;
            L.gates = 0;
            L.mac_only = mac;
            L.mack = mack;
            launches.push_back(L);
            open = true;
        }
        Launch &L = launches.back();
        r.step0 = step_cursor;
        recs.push_back(r);
        L.nrec++;
        L.steps += s;
        L.gates += g;
        step_cursor += s;
        total_steps += s;
        total_gates += g;
        total_xors += memo_xors;                       // (cost(r) above left r's figures in the memo)
        if (L.steps > max_launch_steps) max_launch_steps = L.steps;
    }

    static Rec mk(uint32_t op, uint32_t dst, uint32_t a = 0, uint32_t b = 0, uint32_t c = 0, uint32_t cnt = 1,
                  int32_t sa = 1, int32_t sb = 1) {
        Rec r;
        r.op = op; r.cnt = cnt; r.dst = dst; r.a = a; r.b = b; r.c = c; r.sa = sa; r.sb = sb; r.step0 = 0;
        return r;
    }

    // k trees of OP_MAX level by level in the same launches: tree t writes the maximum of the n words at src + t * sstep
    // (stride 1) and the constant-zero word to dst + t * dstep, and uses scratch + t * max_tree_scratch(n).  mode 1: an
    // unsigned maximum at both widths (OP_MAX with b = 1), where the constant zero is the least value and needs no record
    // of its own; mode 2: the signed MINIMUM of the n words at both widths (b = 2), the constant zero not among them
    void max_trees(size_t k, uint32_t dst, uint32_t dstep, uint32_t src, uint32_t sstep, size_t n, uint32_t scratch, int mode = 0) {
        const uint32_t ub = (uint32_t)mode;
        const bool uns = mode != 0;
        const size_t fan = 8;
        const uint32_t bstep = (uint32_t)max_tree_scratch(n);
        uint32_t cur = src, cstep = sstep;
        size_t cnt = n;
        uint32_t buf = scratch;
        new_launch();
        while (cnt > fan) {
            size_t groups = (cnt + fan - 1) / fan;
            for (size_t t = 0; t < k; t++)
                for (size_t g = 0; g < groups; g++) {
                    size_t len = (g + 1) * fan <= cnt ? fan : cnt - g * fan;
                    emit(mk(OP_MAX, buf + (uint32_t)(t * bstep + g), cur + (uint32_t)(t * cstep + g * fan), ub, 0, (uint32_t)len));
                }
            new_launch();
            cur = buf;
            cstep = bstep;
            buf += (uint32_t)groups;
            cnt = groups;
        }
        // the initial ng = 0 (cgd.oc:98-101,140): at w = 64 the compare is unsigned (obig_cmp) and max(x, 0) is x -- nothing
        // to fold in; at w = 32 it is signed and a magnitude of INT_MIN loses against the zero: one more record
        if (w == 64 || uns) {
            for (size_t t = 0; t < k; t++) emit(mk(OP_MAX, dst + (uint32_t)(t * dstep), cur + (uint32_t)(t * cstep), ub, 0, (uint32_t)cnt));
            new_launch();
            return;
        }
        for (size_t t = 0; t < k; t++) emit(mk(OP_MAX, buf + (uint32_t)(t * bstep), cur + (uint32_t)(t * cstep), 0, 0, (uint32_t)cnt));
        new_launch();
        for (size_t t = 0; t < k; t++) {
            const uint32_t tmp = buf + (uint32_t)(t * bstep);
            emit(mk(OP_MAX, dst + (uint32_t)(t * dstep), tmp, 0, 0, 2, -(int32_t)tmp));  // words[tmp], words[0] (= const zero)
        }
        new_launch();
    }
    static size_t max_tree_scratch(size_t n) { return n / 4 + 16; }

    // dot products in carry-save form, chunked so that a launch has enough waves.
    // result words: dst[i] = base[i] - sum_k A[i][k]*B[k]  (subtract) or  = sum (no base)
    // kdelta != 0 (64-bit only): the products go through the Karatsuba circuit (OP_MACK); hdiff of every operand
    // word of the job lies kdelta words above it (the caller has emitted the OP_HDIFF records)
    struct DotJob { uint32_t dst, base, a, b; uint32_t len; bool has_base; uint32_t kdelta = 0; };
    // MAC records of a batch of dot products for `chunk` products per record (two chunks per record
    // when w == 32); fills the partial-word bookkeeping of every job
    void dots_records(const std::vector<DotJob> &jobs, uint32_t scratch, size_t chunk, std::vector<Rec> &out,
                      std::vector<std::pair<uint32_t, uint32_t>> &parts, bool kara_ok = true) const {
        out.clear();
        parts.assign(jobs.size(), std::make_pair(0u, 0u));   // (first partial word, count of words)
        uint32_t cur = scratch;
        for (size_t i = 0; i < jobs.size(); i++) {
            const DotJob &J = jobs[i];
            parts[i].first = cur;
            uint32_t nparts = 0;
            for (uint32_t k0 = 0; k0 < J.len;) {
                uint32_t left = J.len - k0;
                if (w == 32 && left >= 2) {
                    // two chunks of `len` products side by side in one wave (lanes 0..31 / 32..63)
                    uint32_t len = left / 2 < chunk ? left / 2 : (uint32_t)chunk;
                    out.push_back(mk(OP_MAC2, cur, J.a + k0, J.b + k0, 0, len));
                    cur += 4;
                    nparts += 4;
                    k0 += 2 * len;
                } else {
                    // ceil(len / chunk) records of (nearly) equal length rather than full chunks and a remainder: the
                    // records of a launch run in lock step, round by round.  Karatsuba records take their products two
                    // at a time: even lengths (a single leftover product would be paired with the zero word)
                    const uint32_t nrec_job = (uint32_t)((left + chunk - 1) / chunk);      // (w == 32: `left` is the odd last product)
                    const bool kara = J.kdelta && w == 64 && kara_ok;
                    const uint32_t unit = kara ? 2u : 1u, units = (left + unit - 1) / unit;
                    for (uint32_t q = 0; q < nrec_job && k0 < J.len; q++) {
                        uint32_t un = units / nrec_job + (q < units % nrec_job ? 1u : 0u);
                        uint32_t len = un * unit;
                        if (len > J.len - k0) len = J.len - k0;
                        if (!len) continue;
                        out.push_back(mk(kara ? OP_MACK : OP_MAC, cur, J.a + k0, J.b + k0, kara ? J.kdelta : 0, len));
                        cur += 2;
                        nparts += 2;
                        k0 += len;
                    }
                }
            }
            parts[i].second = nparts;
        }
    }
    // Launch shaping.  The MAC kernels run one workgroup per CU with 16 (garbler) or 12 (evaluator)
    // records each, and every record of a batch takes the same time, so a launch proceeds in rounds
    // of 4096 / 3072 records: a launch of 10 400 records costs three garbler rounds but fills 2.55.
    // Among the chunk sizes down to half the default and the launch counts that respect the table
    // cap, pick the pair with the least rounds x steps, and split the records evenly.
    // (Round 4: the callers' record targets -- kMvRecords64/32, kFactRecords below -- now ask for records so short that a big
    // launch is tens of rounds and the round model only decides between neighbouring chunk sizes; it still matters for
    // mid-size batches and for the launch count of a merged sweep.)
    static double round_cost(size_t per, size_t quantum) {   // a workgroup is the unit: a partial round costs a round
        return (double)((per + quantum - 1) / quantum);
    }
    // relative time of a batch of MAC records run as `launches` equal launches, longest records first: a round takes as
    // long as its first (longest) record; garbler rounds of 4096 records weigh 64 (16 waves per CU, 4 AES per gate),
    // evaluator rounds of 3072 weigh 24 (12 waves, 2 AES).  rep: every record stands for `rep` equal ones (the circuits
    // of a merged sweep, replicate_program).
    static double shaped_cost(const std::vector<uint64_t> &steps_desc, size_t rep, size_t launches) {
        const size_t N = steps_desc.size() * rep, per = (N + launches - 1) / launches;
        double t = 3e2 * (double)launches;
        for (size_t lo = 0; lo < N; lo += per) {
            const size_t hi = lo + per < N ? lo + per : N;
            for (size_t i = lo; i < hi; i += 4096) t += 64.0 * (double)steps_desc[i / rep];
            for (size_t i = lo; i < hi; i += 3072) t += 24.0 * (double)steps_desc[i / rep];
        }
        return t;
    }
    // kara_min: Karatsuba records (jobs with kdelta) where the batch has more than kara_min products; 0 = where the
    // default chunk holds two products
    void dots(const std::vector<DotJob> &jobs, uint32_t scratch, size_t target_waves, size_t kara_min = 0) {
        size_t total = 0;
        bool any_kara = false;
        for (size_t i = 0; i < jobs.size(); i++) { total += jobs[i].len; any_kara = any_kara || (jobs[i].kdelta && w == 64); }
        if (total == 0) return;
        size_t c0 = dots_chunk(total, target_waves), clo = dots_chunk_low(total, target_waves);
        // Karatsuba records take their products in pairs: only where the batch is large enough for two products per record
        // (the early and late columns of a factorisation are not: a lone product paired with the zero word costs 220 steps)
        const bool kara_ok = kara_min ? total > kara_min : c0 >= 2;
        if (any_kara && kara_ok) { if (c0 < 2) c0 = 2; if (clo < 2) clo = 2; }
        // chunk sizes from half to one and a half times the default (larger chunks: fewer, longer records -- and fewer
        // partial sums to merge); the scratch for the partial sums is sized for the smallest chunk
        size_t chi = c0 + c0 / 2;
        {
            uint64_t s1, g1;
            cost(mk(OP_MAC, 0, 0, 0, 0, 1), s1, g1);
            const size_t by_slot = (size_t)(cap_steps / ((uint64_t)kMinRecsPerLaunch * s1));
            if (chi > by_slot) chi = by_slot > c0 ? by_slot : c0;
        }
        const size_t rep = merge_hint ? merge_hint : 1;
        std::vector<Rec> recs_best, recs_try;
        std::vector<std::pair<uint32_t, uint32_t>> parts, parts_try;
        std::vector<uint64_t> sdesc;
        double best = -1.0;
        size_t best_launches = 1;
        for (size_t c = chi; c >= clo; c--) {
            dots_records(jobs, scratch, c, recs_try, parts_try, kara_ok);
            uint64_t steps = 0, smax = 0;
            sdesc.resize(recs_try.size());
            for (size_t i = 0; i < recs_try.size(); i++) {
                uint64_t s1, g1;
                cost(recs_try[i], s1, g1);
                steps += s1;
                if (s1 > smax) smax = s1;
                sdesc[i] = s1;
            }
            std::sort(sdesc.begin(), sdesc.end(), [](uint64_t x, uint64_t y) { return x > y; });
            const size_t R = recs_try.size();
            const size_t lmin = (size_t)((steps + cap_steps - 1) / cap_steps);
            for (size_t L = lmin ? lmin : 1; L <= lmin + 3; L++) {
                size_t per = (R + L - 1) / L;
                if ((uint64_t)per * smax > cap_steps) continue;
                // a merged sweep is ONE batch of rep x R records (replicate_program cuts it by the table cap afterwards)
                const double c_est = shaped_cost(sdesc, rep, rep > 1 ? 1 : L);
                if (best < 0 || c_est < best) { best = c_est; best_launches = L; recs_best = recs_try; parts = parts_try; }
                if (rep > 1) break;
            }
            if (c == 1) break;
        }
        if (best < 0) {   // cannot happen (L = lmin + 3 always fits); keep the default shape
            dots_records(jobs, scratch, c0, recs_best, parts, kara_ok);
            best_launches = 0;
        }
        {   // the partial sums of this call must fit the scratch its caller allocated
            uint32_t end = scratch;
            for (size_t i = 0; i < parts.size(); i++) if (parts[i].first + parts[i].second > end) end = parts[i].first + parts[i].second;
            auto cap = dots_caps.find(scratch);
            if (cap == dots_caps.end() || (size_t)(end - scratch) > cap->second) overflow = true;
        }
        new_launch();
        // longest records first: a round of the chip then holds records of one length (the records of a launch are
        // independent, so their order is free)
        std::stable_sort(recs_best.begin(), recs_best.end(), [](const Rec &x, const Rec &y) { return x.cnt > y.cnt; });
        const size_t R = recs_best.size();
        const size_t per = best_launches ? (R + best_launches - 1) / best_launches : R;
        for (size_t i = 0; i < R; i++) {
            if (i && per && i % per == 0) new_launch();
            emit(recs_best[i]);
        }
        new_launch();
        // Merging the partial sums of a job is a chain of carry-save steps as long as the job has parts (two words per
        // piece).  Where few jobs run at once the chain IS the run time of the merge launch (Cholesky at d = 100: 198
        // merge launches of up to 198 + 14 dependent steps, 8 % of the solve), so long merges go in two levels: groups of
        // about sqrt(parts) words are resolved side by side, then the group sums are merged (sums mod 2^w: any grouping
        // gives the same word).  Many jobs at once (a merged lambda sweep) are throughput-bound and keep the single
        // level: the extra additions would cost more than the shorter chain saves.
        size_t maxparts = 0;
        for (size_t i = 0; i < jobs.size(); i++) if (jobs[i].len && parts[i].second > maxparts) maxparts = parts[i].second;
        if (jobs.size() <= kSumTreeMaxJobs && maxparts >= kSumTreeMinParts) {
            std::vector<uint32_t> gsz(jobs.size(), 0), gcnt(jobs.size(), 0);
            size_t need = 0;
            for (size_t i = 0; i < jobs.size(); i++) {
                if (jobs[i].len == 0) continue;
                uint32_t cnt = parts[i].second, m = 1;
                while ((uint64_t)m * m < cnt) m++;
                gsz[i] = m; gcnt[i] = (cnt + m - 1) / m;
                need += gcnt[i];
            }
            if (need > sum_tree_cap) { sum_tree_cap = need + need / 2 + 16; sum_tree_base = alloc(sum_tree_cap); }
            uint32_t off = 0;
            std::vector<uint32_t> first(jobs.size(), 0);
            for (size_t i = 0; i < jobs.size(); i++) {
                if (jobs[i].len == 0) continue;
                first[i] = sum_tree_base + off;
                for (uint32_t g = 0; g < gcnt[i]; g++) {
                    uint32_t lo = g * gsz[i], n = parts[i].second - lo < gsz[i] ? parts[i].second - lo : gsz[i];
                    emit(mk(OP_SUM, first[i] + g, parts[i].first + lo, 0, 0, n));
                }
                off += gcnt[i];
            }
            new_launch();
            for (size_t i = 0; i < jobs.size(); i++) {
                const DotJob &J = jobs[i];
                if (J.len == 0) continue;
                if (J.has_base) emit(mk(OP_SUBSUM, J.dst, first[i], 0, J.base, gcnt[i]));
                else emit(mk(OP_SUM, J.dst, first[i], 0, 0, gcnt[i]));
            }
            new_launch();
            return;
        }
        for (size_t i = 0; i < jobs.size(); i++) {
            const DotJob &J = jobs[i];
            if (J.len == 0) continue;
            if (J.has_base) emit(mk(OP_SUBSUM, J.dst, parts[i].first, 0, J.base, parts[i].second));
            else emit(mk(OP_SUM, J.dst, parts[i].first, 0, 0, parts[i].second));
        }
        new_launch();
    }
    static constexpr size_t kSumTreeMaxJobs = 1024, kSumTreeMinParts = 32;
    uint32_t sum_tree_base = 0;          // scratch words of the first merge level (grow-only, shared by all dots() calls)
    size_t sum_tree_cap = 0;
    // products per OP_MAC record: enough records to fill the chip (target_waves), and
    // short enough that one table slot (cap_steps gate steps) still holds >= kMinRecsPerLaunch
    // records -- a launch with fewer waves than the GPU has wave slots idles most CUs
    size_t dots_chunk(size_t total, size_t target_waves) {
        size_t chunk = (total + target_waves - 1) / target_waves;
        uint64_t s1, g1;
        cost(mk(OP_MAC, 0, 0, 0, 0, 1), s1, g1);      // (an upper bound for OP_MACK records as well)
        size_t by_slot = (size_t)(cap_steps / ((uint64_t)kMinRecsPerLaunch * s1));
        if (chunk > by_slot) chunk = by_slot;
        if (chunk < 1) chunk = 1;
        return chunk;
    }
    // smallest chunk the launch shaping in dots() may pick (sizes the scratch for the partial sums)
    size_t dots_chunk_low(size_t total, size_t target_waves) {
        size_t c = dots_chunk(total, target_waves) / 2;
        return c < 1 ? 1 : c;
    }
    // Scratch words for the partial sums of ONE dots() call (two words per record, four per dual 32-bit record), whatever
    // its batch: with c0 = ceil(total / target_waves) the smallest chunk tried is max(1, c0 / 2) >= c0 / 3, so a call makes
    // at most 3 * target_waves + njobs records (total_products: an upper bound on the products of any one call).  (Round 2 sized this from the total of the LARGEST call at ITS smallest
    // chunk; a smaller call has its own, relatively smaller, smallest chunk -- c0 = 4 gives 2 -- and with the larger table
    // cap of round 3 the 32-bit Cholesky at d = 250 ran 4 000 words past the end.  build_program now also verifies that
    // every record stays inside the word file: Program::ranges_ok.)
    size_t dots_scratch(size_t total_products, size_t njobs, size_t target_waves) {
        // ... unless the table cap, not the target, bounds the chunk (dots_chunk: by_slot): then a call makes up to
        // total / max(1, by_slot / 2) records
        uint64_t s1, g1;
        cost(mk(OP_MAC, 0, 0, 0, 0, 1), s1, g1);
        const size_t by_slot = (size_t)(cap_steps / ((uint64_t)kMinRecsPerLaunch * s1));
        const size_t lo = by_slot / 2 ? by_slot / 2 : 1;
        size_t recs = 3 * target_waves;
        if (total_products / lo + 1 > recs) recs = total_products / lo + 1;
        if (recs > total_products) recs = total_products;                 // (never more records than products)
        return 2 * (recs + njobs + 2) + 4 * njobs + 16;   // + tails of dual 32-bit records
    }
    // allocate the scratch of a series of dots() calls and remember its size: dots() checks every call against it
    // (a call that does not fit marks the program `overflow`, which the engine refuses to run)
    std::map<uint32_t, size_t> dots_caps;
    bool overflow = false;
    uint32_t alloc_dots(size_t total_products, size_t njobs, size_t target_waves, size_t extra = 0) {
        const size_t n = dots_scratch(total_products, njobs, target_waves) + extra;
        const uint32_t base = alloc(n);
        dots_caps[base] = n;
        return base;
    }
    // every word a record touches lies inside the word file (checked once per built program)
    bool ranges_ok() const {
        if (overflow) return false;
        for (size_t i = 0; i < recs.size(); i++) {
            const Rec &r = recs[i];
            uint64_t hi = 0;
            auto upd = [&hi](uint64_t x) { if (x > hi) hi = x; };
            const uint64_t n = r.cnt ? r.cnt : 1;
            switch (r.op) {
            case OP_MAC: upd(r.dst + 1); upd((uint64_t)((int64_t)r.a + (int64_t)(n - 1) * r.sa)); upd((uint64_t)((int64_t)r.b + (int64_t)(n - 1) * r.sb)); break;
            case OP_MAC2: upd(r.dst + 3); upd((uint64_t)((int64_t)r.a + (int64_t)(2 * n - 1) * r.sa)); upd((uint64_t)((int64_t)r.b + (int64_t)(2 * n - 1) * r.sb)); break;
            case OP_MACK: upd(r.dst + 1); upd((uint64_t)((int64_t)r.a + (int64_t)(n - 1) * r.sa) + r.c); upd((uint64_t)((int64_t)r.b + (int64_t)(n - 1) * r.sb) + r.c); break;
            case OP_STEPEXP: upd(r.dst + 2); upd(r.a); upd(r.b); break;
            case OP_PROX: upd(r.dst); upd(r.a); upd((uint32_t)(r.a + (uint32_t)r.sa)); upd((uint32_t)(r.dst + (uint32_t)r.sa));
                upd((uint64_t)r.c + ((r.cnt & kProxBounded) ? 4 : 2));
                if (r.sb) upd((uint32_t)(r.dst + (uint32_t)r.sa + (uint32_t)r.sb));
                break;
            case OP_SUM: case OP_SUBSUM: case OP_MAX: case OP_ABSSUM: upd(r.dst); upd(r.a); upd((uint64_t)((int64_t)r.a + (int64_t)(n - 1) * r.sa)); if (r.op == OP_SUBSUM) upd(r.c);
                if (r.op == OP_SUM && r.b) { upd(r.b); upd((uint64_t)((int64_t)r.b + (int64_t)(n - 1) * r.sb)); }   // the gate words of a gated select
                break;
            case OP_EQ: upd(r.dst); upd(r.a); upd(r.b);
                if (r.cnt >= 2) { upd(r.dst + n - 1); upd((uint64_t)((int64_t)r.a + (int64_t)(n - 1) * r.sa)); upd(r.c); }   // the one-hot variant
                break;
            case OP_IPMAC: upd(r.dst + 3); upd(r.a + n - 1); upd(r.b + n - 1); break;
            case OP_IPFIN: case OP_IPMERGE: upd(r.dst + (r.op == OP_IPMERGE ? 3 : 0)); upd(r.a + 4 * n - 1); break;
            case OP_CONST: upd(r.dst); break;
            case OP_REVEAL: upd(r.a); break;
            case OP_IDIVC: case OP_COPY: case OP_ABS: case OP_SQRT: case OP_HDIFF: upd(r.dst); upd(r.a); break;
            case OP_MULSUB: upd(r.dst); upd(r.a); upd(r.b); upd(r.c); if (r.cnt >= 2) upd((uint32_t)(r.dst + (uint32_t)r.sa)); break;   // the second store's offset wraps in 32 bits, as in exec_record
            case OP_DIVB: upd(r.dst); upd(r.a); upd(r.b); break;
            case OP_DIV: case OP_MUL: upd(r.dst); upd(r.a); upd(r.b); if (r.op == OP_DIV) upd(r.c); if (r.cnt == 2) upd((uint32_t)(r.dst + (uint32_t)r.sa)); break;
            default: upd(r.dst); upd(r.a); upd(r.b); break;
            }
            if (hi >= n_words) return false;
        }
        return true;
    }

    // wide inner products (fixed.oc:124-147), several independent ones level-synchronously:
    // one product per record, then a fan-in-4 merge tree of carry-save accumulators
    struct IpJob { uint32_t dst, a, b; };
    void inners(const std::vector<IpJob> &jobs, size_t n, uint32_t scratch) {
        const size_t fan = 4;
        const size_t per = inner_scratch(n) / 1;   // words reserved per job
        new_launch();
        for (size_t j = 0; j < jobs.size(); j++) {
            uint32_t base = scratch + (uint32_t)(j * per);
            for (size_t k = 0; k < n; k++)
                emit(mk(OP_IPMAC, base + (uint32_t)(4 * k), jobs[j].a + (uint32_t)k, jobs[j].b + (uint32_t)k, 0, 1));
        }
        new_launch();
        size_t cnt = n;
        uint32_t off_cur = 0, off_next = (uint32_t)(4 * n);
        while (cnt > fan) {
            size_t groups = (cnt + fan - 1) / fan;
            for (size_t j = 0; j < jobs.size(); j++) {
                uint32_t base = scratch + (uint32_t)(j * per);
                for (size_t g = 0; g < groups; g++) {
                    size_t len = (g + 1) * fan <= cnt ? fan : cnt - g * fan;
                    emit(mk(OP_IPMERGE, base + off_next + (uint32_t)(4 * g), base + off_cur + (uint32_t)(4 * g * fan), 0, 0,
                            (uint32_t)len));
                }
            }
            new_launch();
            off_cur = off_next;
            off_next += (uint32_t)(4 * groups);
            cnt = groups;
        }
        for (size_t j = 0; j < jobs.size(); j++) {
            uint32_t base = scratch + (uint32_t)(j * per);
            emit(mk(OP_IPFIN, jobs[j].dst, base + off_cur, 0, 0, (uint32_t)cnt));
        }
        new_launch();
    }
    static size_t inner_scratch(size_t n) { return 4 * n + 4 * (n / 3 + 8) + 16; }   // per job

    // OP_REVEAL of the n words at src into the decode slots [slot, slot + n), then the launch closes
    void reveal(uint32_t slot, uint32_t src, size_t n) {
        for (size_t i = 0; i < n; i++) emit(mk(OP_REVEAL, slot + (uint32_t)i, src + (uint32_t)i));
        new_launch();
    }
    // beta: the n words at src, revealed into decode slots of their own
    void reveal_beta(uint32_t src, size_t n) {
        beta_at = src;
        if (keep_beta) return;                   // (a circuit of a ridge cross-validation: scored and selected from, not revealed)
        rv_beta = alloc_reveal(n); reveal(rv_beta, src, n);
    }
    // the end of an iteration: its last launch and the AND gates emitted up to there
    void mark_iteration() { iter_launch.push_back((uint32_t)(launches.size() - 1)); iter_gates.push_back(total_gates); }
};

// Records per big multiply-accumulate launch.  Rounds 1-3 shaped these launches to whole rounds of the chip (12 288 records of
// ~21 products: three garbler rounds of 4 096 waves, four evaluator rounds of 3 072) -- but records of one length retire in lock
// step, and the OTHER chain's dependent small launches (sums, inner products, the scalar dividers between two matrix-vector
// products) then get CUs only at a round boundary: one launch of that chain per ~11 ms round, so the chain ran past the MAC
// kernel it was meant to hide behind and the next matrix-vector product started 4-7 ms late, every iteration
// (kernel timelines: profiles/r4_timeline_d500_cgd3_*.txt).  Short records (two products = one Karatsuba pair, 220 gate
// steps, ~1.5 ms) turn workgroups over continuously: the chain finishes in half the MAC kernel's time, the MAC kernels
// themselves lose nothing (d = 500 CGD-15: 1.99 -> 1.81 s, d = 300: 0.78 -> 0.71 s; scripts/exp/shape_ab*.sh).  The price is
// more partial sums to merge (+1 % gate steps at d = 500).  kTargetWaves still decides WHERE Karatsuba records are used
// (batches of more than that many products), so programs of small systems are what they were.
// (End of round 5: 8 192 instead of 12 288 -- d = 91 ... 110 get Karatsuba records too -- now that a Karatsuba launch of up to
// three rounds picks its waves per workgroup, gc_mack_waves: d = 100 CGD-15 0.128 -> 0.122 s, scripts/exp/kara_small_ab.sh;
// with sixteen-wave workgroups the 5 000 pairs of d = 100 were rounds of 16 + 3.5 waves and 3 % SLOWER than 10 000 plain records.)
static const size_t kTargetWaves = 8192;
static const size_t kMvRecords64 = 131072;       // matrix-vector products of CGD, 64-bit (chunk floor: one Karatsuba pair)
static const size_t kMvRecords32 = 65536;        // ... 32-bit (two-chunk OP_MAC2 records; 131 072 costs 5 % more steps)
static const size_t kFactRecords = 65536;        // a column step of Cholesky / LDL^T (d = 500: 12.6 -> 12.0 s)
static const size_t kAbsChunk = 64;              // magnitudes per OP_ABSSUM record (lasso: the row sums of |M_ij| >> s)

// FISTA's momentum coefficients c_k = (t_k - 1) / t_{k+1}, t_0 = 1, t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2, in IEEE double,
// quantised as lambda is: (int64)(c_k 2^p), truncated.  Public and data-independent.  (The statements are split so that no
// compiler contracts them into a fused multiply-add: the host-side model computes them the same way.)
inline std::vector<uint64_t> fista_coefficients(int iters, int w, int p) {
    std::vector<uint64_t> c((size_t)(iters > 0 ? iters : 0));
    double t = 1.0;
    for (int k = 0; k < iters; k++) {
        const double t4 = 4.0 * t * t;
        const double r = std::sqrt(1.0 + t4);
        const double tn = (1.0 + r) / 2.0;
        const double ck = (t - 1.0) / tn;
        uint64_t q = (uint64_t)(int64_t)std::ldexp(ck, p);
        if (w == 32) q = (uint64_t)(uint32_t)q;
        c[(size_t)k] = q;
        t = tn;
    }
    return c;
}

// Karatsuba products in the matrix-vector launches of CGD (64-bit; Circ::mack2).  Process-wide switch for A/B runs
// (lgc_set_karatsuba); garbler and evaluator must agree, as on everything else that shapes the program.
inline int &program_karatsuba() { static int on = 1; return on; }

// What build_program lowers: one phase-2 solve.
//   normalize = 1: data-provider path (linear.oc:52-65): diag += lambda, off-diag and b divided by d
//   normalize = 0: two-party benchmark path (linear.oc:96-135): a = in1 + in2, nothing else
//   reveal_ab: debug reveal of a and b (linear.oc:68-84)
// (merge_hint and cap_steps, which shape the dot products, are set on the Program)
struct Spec {
    int alg, w, p, iters;             // iters: CGD / lasso iterations
    size_t d, nshares, targets;
    int normalize, reveal_ab, trace;
    uint64_t lambda_fixed, l1_fixed;  // lambda (on the diagonal) and lasso's lambda1, in fixed point
    // a lasso path: l1_count values at l1_path (fixed point) replace l1_fixed -- lambda1 values (L1_ABSOLUTE) or ratios r_l of
    // lambda_max = max_i |b_i| (L1_RATIO); l1_path = 0 is the single solve
    int l1_mode = 0;
    size_t l1_count = 1;
    const uint64_t *l1_path = 0;
    // lasso options (linreg_gc_lasso_opts.h): l1_coord != 0 gives every (value l, coordinate i) its own quantised
    // q(lambda1_l w_i) (L1_ABSOLUTE) or q(r_l w_i) (L1_RATIO) at l1_coord[l d + i]; boxed[i] marks a coordinate with a finite
    // bound, clamped to [lo[i], hi[i]] (a missing side holds the extreme word).  l1_coord = 0: no options, today's layout
    const uint64_t *l1_coord = 0;
    const uint64_t *lo = 0, *hi = 0;
    const uint8_t *boxed = 0;
    // model selection (linreg_gc_lasso_select.h): every share carries a validation system after the training system; the
    // path's models are scored on it in the circuit and beta* alone is revealed (select_reveal: SELECT_REVEAL_* bits)
    bool validate = false;
    int select_reveal = 0;
    // K-fold cross-validation (linreg_gc_lasso_cv.h): every share carries `folds` fold systems; 0: none.  Excludes validate
    size_t folds = 0;
    // linreg_gc_lasso_cv_se.h: every share ends with the K words yy_k; the rule the refit is chosen by (CV_RULE_*)
    bool yy = false;
    int cv_rule = CV_RULE_MIN;
    // are the curve (mean_l, se_l) and hence the sums Y_k formed?  Where something is scored and the rule or the reveal asks
    bool curve() const { return yy && folds && l1_path && l1_count > 1 && (cv_rule == CV_RULE_ONE_SE || (select_reveal & SELECT_REVEAL_CURVE)); }
    // inference (linreg_gc_inference.h; ALG_CHOLESKY, one target): INFER_* bits, and q(resid_scale)
    int infer = 0;
    uint64_t resid_fixed = 0;
    // an association scan (linreg_gc_scan.h; ALG_CHOLESKY): the number of candidate columns and the SCAN_* bits; d is c + 1
    size_t scan = 0;
    int scan_bits = 0;
};
enum { L1_ABSOLUTE = 0, L1_RATIO = 1 };

// Where the input assembly leaves the system for the solvers.  k right-hand sides: every share is [A (T)] [b_0 (d)] ...
// [b_{k-1} (d)]; A is shared by all targets, and every per-target vector or scalar below is an array of k, target t at
// offset t * d (t): k = 1 is the single-target program, word for word
struct Layout {
    size_t d, K;
    uint32_t M;                       // full symmetric storage, M[i*d+j] == M[j*d+i]
    uint32_t bv;                      // b_t at bv + t * d
    uint32_t Mi(size_t i, size_t j) const { return M + (uint32_t)(i * d + j); }
    uint32_t tv_(uint32_t base, size_t t) const { return base + (uint32_t)(t * d); }    // vector of target t
    // the systems lower_lasso fits and scores on, each full symmetric with its b: without cross-validation the one training
    // system (M, bv) and, with Spec::validate, the one validation system (no lambda2); with K folds the K + 1 training
    // systems (all folds but k, then all folds: with lambda2) and the K validation systems (fold k, no lambda2)
    std::vector<uint32_t> Ms, bs, Mvs, bvs;
    uint32_t yy = 0;                  // the K words Y_k (Spec::curve), or 0
    uint32_t Y = 0, b0 = 0;           // inference: the share sum of yy (divided as b is) and b as assembled, untouched by the solve
};

// "check if inputs have equal dimensions" (src/linear.oc:109-114): the first word of either party's input is its d; one
// comparison, revealed.  d = 1, two shares: a program that does not depend on what it checks
inline void lower_dimcheck(Program &P) {
    const uint32_t eq = P.alloc(1);
    P.new_launch();
    P.emit(Program::mk(OP_EQ, eq, P.in_base, P.in_base + (uint32_t)P.in_words()));
    P.new_launch();
    P.reveal_beta(eq, 1);
}

// ---- input assembly.  A packed system is [A (T)] [b (.)]: the lower triangle of a symmetric matrix row by row, entry (i, j)
// at tri(i, j), then its vector(s) -- the form of a share and of the share sums.  Each helper below acts on ONE system
inline uint32_t tri(size_t i, size_t j) { return (uint32_t)(i * (i + 1) / 2 + j); }
// where a system lies: A packed or in full d x d storage, and its vector(s)
struct SysAt {
    size_t d; uint32_t A, b; bool full;
    uint32_t a(size_t i, size_t j) const { return A + (full ? (uint32_t)(i * d + j) : tri(i, j)); }
};
inline SysAt packed_at(size_t d, uint32_t base) { return {d, base, base + tri(d, 0), false}; }
// a[ij] = sum of shares (linear.oc:31-49 / :116-127): the system `off` words into every share, with nb vector words, into `to`
inline void sum_shares(Program &P, uint32_t off, size_t nb, const SysAt &to) {
    const uint32_t in = P.in_base + off, n = (uint32_t)P.nshares, stride = (uint32_t)P.in_words();
    for (size_t i = 0; i < to.d; i++)
        for (size_t j = 0; j <= i; j++) P.emit(Program::mk(OP_SUM, to.a(i, j), in + tri(i, j), 0, 0, n, (int32_t)stride));
    for (size_t i = 0; i < nb; i++) P.emit(Program::mk(OP_SUM, to.b + (uint32_t)i, in + tri(to.d, 0) + (uint32_t)i, 0, 0, n, (int32_t)stride));
}
// the division by the public normalizer (linear.oc:57-65): the off-diagonals and the vector words of a packed system, in place
inline void divide_by_d(Program &P, const SysAt &s, size_t nb) {
    for (size_t i = 0; i < s.d; i++)
        for (size_t j = 0; j < i; j++) P.emit(idivc_rec(s.a(i, j), s.a(i, j), (uint32_t)s.d, P.w));
    for (size_t i = 0; i < nb; i++) P.emit(idivc_rec(s.b + (uint32_t)i, s.b + (uint32_t)i, (uint32_t)s.d, P.w));
}
// A packed triangle at `src` into the full symmetric storage at M, both triangles (the factorisations work in place), row by
// row as the pairs (i, j), (j, i).  The diagonal is what differs between the callers, and with it the record order: += the
// word lam (linear.oc:54-56), all d in a launch of their own ahead of the pairs (DIAG_LAMBDA_LAUNCH) or each at the head of
// its row (DIAG_LAMBDA_ROW); or copied at the end of its row (DIAG_COPY: a validation system takes no lambda)
enum Diag { DIAG_LAMBDA_LAUNCH, DIAG_LAMBDA_ROW, DIAG_COPY };
inline void mirror(Program &P, size_t d, uint32_t M, uint32_t src, Diag diag, uint32_t lam) {
    auto at = [&](size_t i, size_t j) { return M + (uint32_t)(i * d + j); };
    if (diag == DIAG_LAMBDA_LAUNCH) {
        for (size_t i = 0; i < d; i++) P.emit(Program::mk(OP_ADD, at(i, i), src + tri(i, i), lam));
        P.new_launch();
    }
    for (size_t i = 0; i < d; i++) {
        if (diag == DIAG_LAMBDA_ROW) P.emit(Program::mk(OP_ADD, at(i, i), src + tri(i, i), lam));
        for (size_t j = 0; j < i; j++) {
            P.emit(Program::mk(OP_COPY, at(i, j), src + tri(i, j)));
            P.emit(Program::mk(OP_COPY, at(j, i), src + tri(i, j)));
        }
        if (diag == DIAG_COPY) P.emit(Program::mk(OP_COPY, at(i, i), src + tri(i, i)));
    }
}
// debug reveal (linear.oc:68-84) of a system into the slots from `slot`, laid out as a share is
inline void reveal_system(Program &P, uint32_t slot, const SysAt &s, size_t nb) {
    for (size_t i = 0; i < s.d; i++)
        for (size_t j = 0; j <= i; j++) P.emit(Program::mk(OP_REVEAL, slot + tri(i, j), s.a(i, j)));
    for (size_t i = 0; i < nb; i++) P.emit(Program::mk(OP_REVEAL, slot + tri(s.d, 0) + (uint32_t)i, s.b + (uint32_t)i));
}
// the end of the prefix a sweep garbles once (replicate_program): words and launches up to here do not depend on lambda
inline void close_prefix(Program &P, uint32_t shared_end) {
    P.new_launch();
    P.shared_end = shared_end;
    P.prefix_launches = (uint32_t)P.launches.size();
    P.prefix_steps = P.total_steps;
}

// K-fold cross-validation: every share is [A_0 (T)] [b_0 (d)] ... [A_{K-1} (T)] [b_{K-1} (d)].  Fold k is
// assembled as a validation system is -- share sums, on the data-provider path the off-diagonals and b divided by d, no
// lambda2 -- in the two launches the input assembly has always had, into the packed words S + k H (H = T + d).  Then, entry
// by entry on the packed form: tot = sum_k F_k (one OP_SUM of K words, H apart), tot - F_k, the constant divisions by K - 1
// (none for K = 2) and by K, and one launch that mirrors everything into full symmetric storage and adds lambda2 to the
// K + 1 training diagonals -- on BOTH input paths: the folds double as validation systems and must stay free of it.
// The 2 K + 1 matrices lie side by side from L.M on, inside the word range whose Karatsuba shadow the lasso allocates
inline Layout lower_fold_inputs(Program &P, const Spec &spec) {
    const size_t d = spec.d, T = P.T, K = P.folds, H = T + d, IN = P.in_words();
    const uint32_t S = P.alloc(IN);                      // the folds F_k, packed; b of fold k stays here (S + k H + T)
    Layout L = {d, 1, P.alloc((2 * K + 1) * d * d), 0};
    const uint32_t tot = P.alloc(H), dif = P.alloc(K * H);   // later the packed full system and the K packed training systems
    auto fold = [&](size_t k) { return packed_at(d, S + (uint32_t)(k * H)); };
    auto train = [&](size_t s) { return packed_at(d, s < K ? dif + (uint32_t)(s * H) : tot); };
    for (size_t s = 0; s <= K; s++) { L.Ms.push_back(L.M + (uint32_t)(s * d * d)); L.bs.push_back(train(s).b); }
    for (size_t k = 0; k < K; k++) { L.Mvs.push_back(L.M + (uint32_t)((K + 1 + k) * d * d)); L.bvs.push_back(fold(k).b); }
    L.bv = L.bs[K];
    P.new_launch();
    for (size_t k = 0; k < K; k++) sum_shares(P, (uint32_t)(k * H), d, fold(k));
    // Y_k = the share sum of yy_k (the K words behind the folds of every share), divided as b_k is: words of the prefix
    if (spec.curve()) {
        L.yy = S + (uint32_t)(K * H);
        for (size_t k = 0; k < K; k++)
            P.emit(Program::mk(OP_SUM, L.yy + (uint32_t)k, P.in_base + (uint32_t)(K * H + k), 0, 0, (uint32_t)P.nshares, (int32_t)IN));
    }
    P.new_launch();
    if (spec.normalize) {
        for (size_t k = 0; k < K; k++) divide_by_d(P, fold(k), d);
        for (size_t k = 0; k < (L.yy ? K : 0); k++) P.emit(idivc_rec(L.yy + (uint32_t)k, L.yy + (uint32_t)k, (uint32_t)d, P.w));
        close_prefix(P, S + (uint32_t)IN);
    }
    const uint32_t lam = P.alloc(1);
    P.emit(Program::mk(OP_CONST, lam, (uint32_t)spec.lambda_fixed, (uint32_t)(spec.lambda_fixed >> 32)));
    for (size_t e = 0; e < H; e++) P.emit(Program::mk(OP_SUM, tot + (uint32_t)e, S + (uint32_t)e, 0, 0, (uint32_t)K, (int32_t)H));
    P.new_launch();
    for (size_t e = 0; e < K * H; e++) P.emit(Program::mk(OP_SUB, dif + (uint32_t)e, tot + (uint32_t)(e % H), S + (uint32_t)e));
    P.new_launch();
    if (K > 2)                                           // (in place: the differences were formed from tot one launch earlier)
        for (size_t e = 0; e < K * H; e++) P.emit(idivc_rec(dif + (uint32_t)e, dif + (uint32_t)e, (uint32_t)(K - 1), spec.w));
    for (size_t e = 0; e < H; e++) P.emit(idivc_rec(tot + (uint32_t)e, tot + (uint32_t)e, (uint32_t)K, spec.w));
    P.new_launch();
    for (size_t s = 0; s <= K; s++) mirror(P, d, L.Ms[s], train(s).A, DIAG_LAMBDA_ROW, lam);
    for (size_t k = 0; k < K; k++) mirror(P, d, L.Mvs[k], fold(k).A, DIAG_COPY, 0);
    P.new_launch();
    if (spec.reveal_ab) {                                // the K folds as assembled
        P.rv_ab = P.alloc_reveal(IN);
        for (size_t k = 0; k < K; k++) reveal_system(P, P.rv_ab + (uint32_t)(k * H), fold(k), d);
        // (shares with yy words: Y_k, or the constant zero where no curve is formed)
        for (size_t k = 0; k < (P.yy ? K : 0); k++) P.emit(Program::mk(OP_REVEAL, P.rv_ab + (uint32_t)(K * H + k), L.yy ? L.yy + (uint32_t)k : 0));
        P.new_launch();
    }
    return L;
}

// The shares (at P.in_base) summed into M and b, the normalizer prefix, lambda and the mirror of the lower triangle.
// With Spec::validate (lasso model selection) [A_v (T)] [b_v (d)] follow the training system in every share: the validation
// system goes through every step right after the training system, in the same launches, and takes no lambda.  M_v lies
// right behind b, inside the word range whose Karatsuba shadow the lasso allocates; on the data-provider path b_v stays
// where it was summed
inline Layout lower_inputs(Program &P, const Spec &spec) {
    if (P.folds) return lower_fold_inputs(P, spec);
    const size_t d = spec.d, K = spec.targets, IN = P.in_words();
    const bool normalize = spec.normalize != 0;
    // On the data-provider path the sums go to words of their own, S, right after the inputs: everything up to the
    // division does not depend on lambda, so a sweep garbles it once and every circuit of the sweep reads S
    const uint32_t S = normalize ? P.alloc(IN) : 0;
    Layout L = {d, K, P.alloc(d * d), P.alloc(K * d)};   // (a braced list: allocated in this order)
    // the systems of a share: its offset in the share, its vectors and where the solvers read it
    struct In { uint32_t off; size_t nb; SysAt at; };
    std::vector<In> in = {{0, K * d, {d, L.M, L.bv, true}}};
    auto sums = [&](uint32_t off) { return packed_at(d, S + off); };   // (data-provider path) the packed sums of the system at `off`
    L.Ms.push_back(L.M); L.bs.push_back(L.bv);
    if (P.validate) {
        const uint32_t H = (uint32_t)(P.T + K * d), Mv = P.alloc(d * d);
        in.push_back({H, d, {d, Mv, normalize ? sums(H).b : P.alloc(d), true}});
        L.Mvs.push_back(Mv); L.bvs.push_back(in[1].at.b);
    }
    // inference: Y, the share sum of the word yy behind b, goes through what the words of b go through, in b's launches.  On
    // the data-provider path the packed sums keep b as assembled (the solvers work on the copy at L.bv): that is b0; on the
    // two-party path b is summed straight into L.bv, so b0 is a copy taken in the mirror launch
    if (P.infer) {
        L.Y = normalize ? S + (uint32_t)(IN - 1) : P.alloc(1);
        L.b0 = normalize ? sums(0).b : P.alloc(d);
    }
    P.new_launch();
    for (const In &s : in) sum_shares(P, s.off, s.nb, normalize ? sums(s.off) : s.at);
    if (P.infer) P.emit(Program::mk(OP_SUM, L.Y, P.in_base + (uint32_t)(IN - 1), 0, 0, (uint32_t)P.nshares, (int32_t)IN));
    P.new_launch();
    if (normalize) {
        // in place on the share sums, still in the prefix: a sweep divides once, not once per circuit
        for (const In &s : in) divide_by_d(P, sums(s.off), s.nb);
        if (P.infer) P.emit(idivc_rec(L.Y, L.Y, (uint32_t)d, P.w));
        close_prefix(P, S + (uint32_t)IN);
        const uint32_t lam = P.alloc(1);
        P.lam_rec = (uint32_t)P.recs.size();
        P.emit(Program::mk(OP_CONST, lam, (uint32_t)spec.lambda_fixed, (uint32_t)(spec.lambda_fixed >> 32)));
        P.new_launch();
        mirror(P, d, L.M, sums(0).A, DIAG_LAMBDA_LAUNCH, lam);
        for (size_t i = 0; i < K * d; i++) P.emit(Program::mk(OP_COPY, L.bv + (uint32_t)i, sums(0).b + (uint32_t)i));
        if (P.validate) mirror(P, d, in[1].at.A, sums(in[1].off).A, DIAG_COPY, 0);
    } else {
        // the sums went straight into the lower triangles: mirror those
        for (const In &s : in)
            for (size_t i = 0; i < d; i++)
                for (size_t j = 0; j < i; j++) P.emit(Program::mk(OP_COPY, s.at.a(j, i), s.at.a(i, j)));
        for (size_t i = 0; i < (P.infer ? d : 0); i++) P.emit(Program::mk(OP_COPY, L.b0 + (uint32_t)i, L.bv + (uint32_t)i));
    }
    P.new_launch();
    if (spec.reveal_ab) {
        P.rv_ab = P.alloc_reveal(IN);
        for (const In &s : in) reveal_system(P, P.rv_ab + s.off, s.at, s.nb);
        if (P.infer) P.emit(Program::mk(OP_REVEAL, P.rv_ab + (uint32_t)(IN - 1), L.Y));
        P.new_launch();
    }
    return L;
}

// Records per d x d matrix-vector product (CGD, lasso): enough to fill the chip -- together with the other circuits of a
// merged sweep -- and at least two per row; kara_min: Karatsuba products where d * d exceeds it
inline void mv_shape(const Program &P, size_t &waves, size_t &kara_min) {
    const size_t rep = P.merge_hint ? P.merge_hint : 1, d = P.d;
    const size_t mv_target = P.w == 64 ? kMvRecords64 : kMvRecords32;
    waves = mv_target / rep;
    if (waves < 2 * d) waves = 2 * d < mv_target ? 2 * d : mv_target;     // at least two records per row
    kara_min = kTargetWaves / rep;
    if (kara_min < 2 * d) kara_min = 2 * d < kTargetWaves ? 2 * d : kTargetWaves;
}


// ---- lasso.  FISTA (Beck & Teboulle, SIAM J. Imaging Sciences 2(1), 2009) on 1/2 beta^T M beta - b^T beta + lambda1 |beta|_1,
// one target.  Step 2^(p - l) with 2^l ulps >= the largest Gershgorin row sum of M, never revealed; theta = step(lambda1).
// Per iteration: g = M y - b, z = y - step(g), x' = soft(z, theta), y' = x' + c_k (x' - x).  DESIGN.md 2.6.
// A path of NL values of lambda1 runs NL such recurrences on the one M and b, side by side in the launches a single solve
// has (as lower_cgd carries k targets); K-fold cross-validation (P.folds) runs NF = K + 1 such paths, one per training
// system of L.Ms, in the same launches.  NL = 1 in absolute mode and NF = 1 is the single solve, record for record.
// The stages share one plan: sizes and word addresses, fixed once by lasso_plan
struct LassoGroup { size_t l; uint64_t q, lo, hi; bool boxed; };
struct LassoPlan {
    size_t d, NL, NF, NG, GW;            // coordinates, values, fits, threshold groups per fit and the words of a group
    std::vector<size_t> fit;             // the training systems fitted, as indices into Layout::Ms; the last is the full system
    bool ratio, opts, scored;
    int s;                               // the row sums are of |M_ij| >> s, 2^s >= d
    uint32_t TOT;                        // NF NL d: fit f, value l has its vectors at + (f NL + l) d
    uint32_t x, y, u, b2;                // x, y in one block and (M y), the copies of b in another: OP_PROX's pairs, TOT apart
    uint32_t kdelta = 0;                 // Karatsuba products: the offset of the shadow of [L.M, y + TOT), or 0
    uint32_t sc, l1w;                    // the groups, GW words each, fit-major; absolute mode: the NG constants lambda1
    size_t ntree, nch, chl;              // maximum trees; OP_ABSSUM chunks per row and their length
    uint32_t rowsum, mmax;               // the d row sums of every fit (ratio mode: then |b_i| of the full system); their maxima (then lambda_max)
    uint32_t parts, sc_max, sc_dot;      // scratch: the row sums' chunks, the maximum trees, the dot products (shaped by mv_shape:)
    size_t mv_waves, kara_min;
    std::vector<LassoGroup> groups;      // options: the groups in order of first use, and each (l, i)'s group
    std::vector<uint32_t> gof;
    uint32_t group(size_t f, size_t g) const { return sc + (uint32_t)(GW * (f * NG + g)); }
    uint32_t vec(uint32_t base, size_t f, size_t l) const { return base + (uint32_t)((f * NL + l) * d); }
};
// With options (spec.l1_coord) every distinct (l, q(lambda1_l w_i) or q(r_l w_i), lo_i, hi_i) is a group of five words
// (shift word, theta, -theta, lo, hi) with its own OP_STEPEXP record; coordinate i of value l reads its group.  Without
// options the groups are the NL values, three words each
inline void lasso_groups(LassoPlan &Q, const Spec &spec) {
    std::map<std::tuple<size_t, uint64_t, uint64_t, uint64_t, bool>, uint32_t> seen;
    Q.gof.resize(Q.NL * Q.d);
    for (size_t l = 0; l < Q.NL; l++)
        for (size_t i = 0; i < Q.d; i++) {
            const bool bx = spec.boxed[i] != 0;
            const LassoGroup g = {l, spec.l1_coord[l * Q.d + i], bx ? spec.lo[i] : 0, bx ? spec.hi[i] : 0, bx};
            auto it = seen.insert(std::make_pair(std::make_tuple(g.l, g.q, g.lo, g.hi, g.boxed), (uint32_t)Q.groups.size())).first;
            if (it->second == Q.groups.size()) Q.groups.push_back(g);
            Q.gof[l * Q.d + i] = it->second;
        }
}

// What is fitted and where it lives.  Cross-validation fits the K training systems and the full one; one value needs no
// cross-validation: the full system alone is fitted.  Scores are formed where a selection needs them (NL > 1) or a hold-out
// selection reveals them
inline LassoPlan lasso_plan(Program &P, const Spec &spec, const Layout &L) {
    LassoPlan Q;
    const size_t d = Q.d = L.d, NL = Q.NL = spec.l1_path ? spec.l1_count : 1;
    Q.ratio = spec.l1_mode == L1_RATIO; Q.opts = spec.l1_coord != 0;
    if (P.folds && NL > 1) for (size_t k = 0; k < P.folds; k++) Q.fit.push_back(k);
    Q.fit.push_back(P.folds);                            // (without folds the one system, L.Ms[0])
    const size_t NF = Q.NF = Q.fit.size();
    Q.TOT = (uint32_t)(NF * NL * d);
    for (Q.s = 0; ((size_t)1 << Q.s) < d;) Q.s++;
    Q.x = P.alloc(2 * (size_t)Q.TOT); Q.y = Q.x + Q.TOT;
    mv_shape(P, Q.mv_waves, Q.kara_min);
    // hdiff(M) once, hdiff(y_l) by the OP_PROX record that forms y_l, in the ONE shadow that holds every matrix, x and y
    if (spec.w == 64 && spec.iters > 1 && program_karatsuba() && d * d > Q.kara_min) Q.kdelta = P.alloc((size_t)(Q.y + Q.TOT - L.M)) - L.M;
    Q.u = P.alloc(2 * (size_t)Q.TOT); Q.b2 = Q.u + Q.TOT;
    if (Q.opts) lasso_groups(Q, spec);
    Q.NG = Q.opts ? Q.groups.size() : NL; Q.GW = Q.opts ? 5 : 3;
    Q.sc = P.alloc(Q.GW * Q.NG * NF);
    Q.ntree = NF + (Q.ratio ? 1 : 0);
    Q.l1w = Q.ratio ? 0 : P.alloc(Q.NG);
    Q.rowsum = P.alloc(Q.ntree * d); Q.mmax = P.alloc(Q.ntree);
    Q.nch = (d + kAbsChunk - 1) / kAbsChunk; Q.chl = (d + Q.nch - 1) / Q.nch;
    Q.parts = Q.nch > 1 ? P.alloc(NF * d * Q.nch) : 0;
    Q.sc_max = P.alloc(Q.ntree * Program::max_tree_scratch(d));
    Q.scored = P.selects() && (NL > 1 || (!P.folds && (spec.select_reveal & SELECT_REVEAL_SCORES)));
    Q.sc_dot = spec.iters > 1 || Q.scored ? P.alloc_dots(NF * NL * d * d, NF * NL * d, Q.mv_waves) : 0;
    if (spec.trace) P.rv_trace = P.alloc_reveal((size_t)spec.iters * d);
    return Q;
}

// The dot products of length d for (system f, value l, coordinate i), f < nf, l < NL, i < ni, in that order: job
// (f NL + l) ni + i writes the word dst + its index, multiplies the d words at a(f, l) + i d with the vector of (f, l) in
// the block `vec` and, with `sub`, subtracts the sum from the word base(f, i) (zero_word: the constant zero)
inline uint32_t zero_word(size_t, size_t) { return 0; }
template <class A, class B>
inline std::vector<Program::DotJob> lasso_dot_jobs(const LassoPlan &Q, size_t nf, size_t ni, uint32_t dst, A a, uint32_t vec, bool sub, B base, uint32_t kdelta) {
    std::vector<Program::DotJob> jobs;
    jobs.reserve(nf * Q.NL * ni);
    for (size_t f = 0; f < nf; f++)
        for (size_t l = 0; l < Q.NL; l++)
            for (size_t i = 0; i < ni; i++) {
                Program::DotJob J = {dst + (uint32_t)((f * Q.NL + l) * ni + i), base(f, i), a(f, l) + (uint32_t)(i * Q.d), Q.vec(vec, f, l), (uint32_t)Q.d, sub, kdelta};
                jobs.push_back(J);
            }
    return jobs;
}

// Setup.  One launch: lambda1 (absolute mode) and the bounds, the copies of b beside (M y), hdiff(M), the row sums of
// |M_ij| >> s in chunks of kAbsChunk and, in ratio mode, |b_i| of the full system.  Then the Gershgorin maximum of every
// fit -- in ratio mode lambda_max = max_i |b_i| in the same launches, the last tree, shared by all fits -- and one
// OP_STEPEXP per fit and group: theta = step(lambda1), in ratio mode step(mulc(lambda_max, r))
inline void lasso_setup(Program &P, const Spec &spec, const Layout &L, const LassoPlan &Q) {
    const size_t d = Q.d, NF = Q.NF, NG = Q.NG;
    auto value = [&](size_t g) { return Q.opts ? Q.groups[g].q : spec.l1_path ? spec.l1_path[g] : spec.l1_fixed; };
    auto konst = [&](uint32_t dst, uint64_t v) { P.emit(Program::mk(OP_CONST, dst, (uint32_t)v, (uint32_t)(v >> 32))); };
    auto Mf = [&](size_t f, size_t i, size_t j) { return L.Ms[Q.fit[f]] + (uint32_t)(i * d + j); };
    P.new_launch();
    for (size_t g = 0; g < (Q.ratio ? 0 : NG); g++) konst(Q.l1w + (uint32_t)g, value(g));
    for (size_t f = 0; f < NF; f++)
        for (size_t g = 0; g < (Q.opts ? NG : 0); g++)
            if (Q.groups[g].boxed) { konst(Q.group(f, g) + 3, Q.groups[g].lo); konst(Q.group(f, g) + 4, Q.groups[g].hi); }
    for (size_t f = 0; f < NF; f++)
        for (size_t l = 0; l < Q.NL; l++)
            for (size_t i = 0; i < d; i++) P.emit(Program::mk(OP_COPY, Q.vec(Q.b2, f, l) + (uint32_t)i, L.bs[Q.fit[f]] + (uint32_t)i));
    if (Q.kdelta)
        for (size_t f = 0; f < NF; f++)
            for (size_t i = 0; i < d; i++)
                for (size_t j = 0; j <= i; j++) P.emit(Program::mk(OP_HDIFF, Mf(f, i, j) + Q.kdelta, Mf(f, i, j)));
    for (size_t f = 0; f < NF; f++)
        for (size_t i = 0; i < d; i++)
            for (size_t q = 0; q < Q.nch; q++) {
                const size_t lo = q * Q.chl, len = lo + Q.chl <= d ? Q.chl : d - lo;
                const uint32_t dst = Q.nch > 1 ? Q.parts + (uint32_t)((f * d + i) * Q.nch + q) : Q.rowsum + (uint32_t)(f * d + i);
                P.emit(Program::mk(OP_ABSSUM, dst, Mf(f, i, lo), 0, (uint32_t)Q.s, (uint32_t)len));
            }
    if (Q.ratio)
        for (size_t i = 0; i < d; i++) P.emit(Program::mk(OP_ABSSUM, Q.rowsum + (uint32_t)(NF * d + i), L.bv + (uint32_t)i, 0, 0, 1));
    P.new_launch();
    for (size_t i = 0; i < (Q.nch > 1 ? NF * d : 0); i++) P.emit(Program::mk(OP_SUM, Q.rowsum + (uint32_t)i, Q.parts + (uint32_t)(i * Q.nch), 0, 0, (uint32_t)Q.nch));
    P.max_trees(Q.ntree, Q.mmax, 1, Q.rowsum, (uint32_t)d, d, Q.sc_max, true);     // unsigned (opens and closes its own launches)
    for (size_t f = 0; f < NF; f++)
        for (size_t g = 0; g < NG; g++) {
            const uint64_t r = value(g);
            if (Q.ratio) P.emit(Program::mk(OP_STEPEXP, Q.group(f, g), Q.mmax + (uint32_t)f, Q.mmax + (uint32_t)NF, (uint32_t)Q.s, 2, (int32_t)(uint32_t)r, (int32_t)(uint32_t)(r >> 32)));
            else P.emit(Program::mk(OP_STEPEXP, Q.group(f, g), Q.mmax + (uint32_t)f, Q.l1w + (uint32_t)g, (uint32_t)Q.s));
        }
    if (Q.kdelta)                                             // the mirror of hdiff(M), beside it
        for (size_t f = 0; f < NF; f++)
            for (size_t i = 0; i < d; i++)
                for (size_t j = 0; j < i; j++) P.emit(Program::mk(OP_COPY, Mf(f, j, i) + Q.kdelta, Mf(f, i, j) + Q.kdelta));
    P.new_launch();
}

// One iteration with momentum constant c: (M y) for every fit and value in one dots() batch -- none in iteration 0, where
// y = 0 and the vectors (M y) are still the zero word file's -- then ONE launch of NF NL d OP_PROX records, a boxed
// coordinate's with kProxBounded
inline void lasso_iteration(Program &P, const Spec &spec, const Layout &L, const LassoPlan &Q, int it, uint64_t c) {
    if (it > 0)
        P.dots(lasso_dot_jobs(Q, Q.NF, Q.d, Q.u, [&](size_t f, size_t) { return L.Ms[Q.fit[f]]; }, Q.y, false, zero_word, Q.kdelta), Q.sc_dot, Q.mv_waves, Q.kara_min);
    for (size_t f = 0; f < Q.NF; f++)
        for (size_t l = 0; l < Q.NL; l++)
            for (size_t i = 0; i < Q.d; i++) {
                const size_t g = Q.opts ? Q.gof[l * Q.d + i] : l;
                const uint32_t flag = Q.opts && Q.groups[g].boxed ? kProxBounded : 0, v = Q.vec(0, f, l) + (uint32_t)i;
                P.emit(Program::mk(OP_PROX, Q.x + v, Q.u + v, (uint32_t)c, Q.group(f, g), (uint32_t)(c >> 32) | flag, (int32_t)Q.TOT, (int32_t)Q.kdelta));
            }
    P.new_launch();
    if (spec.trace) P.reveal(P.rv_trace + (uint32_t)((size_t)it * Q.d), Q.x, Q.d);
    P.mark_iteration();
}

// Scoring on the validation systems (M_v, b_v), DESIGN.md 2.6: the hold-out error of beta_l = x_l is, up to a constant,
// score_l = beta^T M_v beta - 2 b_v^T beta, formed as r_l = 2 b_v - M_v beta_l and score_l = 0 - <beta_l, r_l>.
// Cross-validation scores fit k on validation system k and sums the K scores of every value.  Returns the NL words
// selected on (the constant zero where nothing is scored)
inline uint32_t lasso_scores(Program &P, const Layout &L, const LassoPlan &Q, uint32_t *per_fold = 0) {
    if (!Q.scored) return 0;
    const size_t d = Q.d, NL = Q.NL, NV = L.Mvs.size();
    const uint32_t score = P.alloc(NV * NL), b2v = P.alloc(NV * d), rr = P.alloc(NV * NL * d);
    const uint32_t sc_sco = P.alloc_dots(NV * NL * d, NV * NL, kTargetWaves), cv = P.folds ? P.alloc(NL) : score;
    if (per_fold) *per_fold = score;                           // score_{k,l} at + k NL + l
    // setup: 2 b_v, and for the Karatsuba products the half-difference words of M_v and of every beta_l in the shadow
    // (OP_PROX formed hdiff(y_l), not hdiff(x_l))
    for (size_t k = 0; k < NV; k++)
        for (size_t i = 0; i < d; i++) P.emit(Program::mk(OP_ADD, b2v + (uint32_t)(k * d + i), L.bvs[k] + (uint32_t)i, L.bvs[k] + (uint32_t)i));
    if (Q.kdelta) {
        for (size_t k = 0; k < NV; k++)
            for (size_t i = 0; i < d * d; i++) P.emit(Program::mk(OP_HDIFF, L.Mvs[k] + (uint32_t)i + Q.kdelta, L.Mvs[k] + (uint32_t)i));
        for (size_t i = 0; i < NV * NL * d; i++) P.emit(Program::mk(OP_HDIFF, Q.x + (uint32_t)i + Q.kdelta, Q.x + (uint32_t)i));
    }
    P.new_launch();
    // r: NV NL d dot products, shaped as an iteration's are; the scores: NV NL plain products (r has no shadow, and they are
    // 1 / d of the batch before)
    P.dots(lasso_dot_jobs(Q, NV, d, rr, [&](size_t k, size_t) { return L.Mvs[k]; }, Q.x, true,
                          [&](size_t k, size_t i) { return b2v + (uint32_t)(k * d + i); }, Q.kdelta), Q.sc_dot, Q.mv_waves, Q.kara_min);
    P.dots(lasso_dot_jobs(Q, NV, 1, score, [&](size_t k, size_t l) { return Q.vec(Q.x, k, l); }, rr, true, zero_word, 0),
           sc_sco, kTargetWaves);
    for (size_t l = 0; l < (P.folds ? NL : 0); l++)            // cv_l = sum_k score_{k,l}, in a launch of its own
        P.emit(Program::mk(OP_SUM, cv + (uint32_t)l, score + (uint32_t)l, 0, 0, (uint32_t)NV, (int32_t)NL));
    P.new_launch();
    return cv;
}

// l* = the first l whose score is the signed minimum: its one-hot words (NL, all lanes) and its index word
struct LassoPick { uint32_t hot, index; };
inline LassoPick select_argmin(Program &P, size_t NL, uint32_t cv) {
    const uint32_t smin = P.alloc(1), hot = P.alloc(NL), sc_min = P.alloc(Program::max_tree_scratch(NL)), index = P.alloc(1);
    P.max_trees(1, smin, 1, cv, (uint32_t)NL, NL, sc_min, 2);
    P.emit(Program::mk(OP_EQ, hot, cv, smin, index, (uint32_t)NL, 1));
    P.new_launch();
    return {hot, index};
}
inline LassoPick lasso_argmin(Program &P, const LassoPlan &Q, uint32_t cv) { return select_argmin(P, Q.NL, cv); }

// The one-standard-error rule (linreg_gc_lasso_cv_se.h), between the scores and the selection.  The curve:
// e_{k,l} = score_{k,l} + Y_k, S_l = sum_k e_{k,l}, mean_l = tdiv(S_l, K), q_l = sum_k mul(e - mean, e - mean),
// se_l = sqrt(tdiv(q_l, K (K - 1))) -- eight launches of K NL or NL records.  Then l* as ever, and with the rule
// thr = mean_{l*} + se_{l*} by the gated select, and l+ = the first l in the public order pi with mean_l <= thr (signed),
// composed of record shapes the selection already has: m_l = min(mean_l, thr) (OP_MAX, b = 2, over the two words),
// z_l = mean_l - m_l (zero exactly where mean_l <= thr) written at l's POSITION in pi, the first-match one-hot of z against
// the constant zero (OP_EQ, cnt = NL), the one-hot words copied back to value order, and l+ = the gated select of the
// constants pi_0 .. pi_{NL-1}.  l* always qualifies (se >= 0), so there is a match.
struct LassoCurve { uint32_t mean = 0, se = 0; LassoPick min = {0, 0}, pick = {0, 0}; };
inline LassoCurve lasso_one_se(Program &P, const Spec &spec, const Layout &L, const LassoPlan &Q, uint32_t cv, uint32_t score) {
    LassoCurve R;
    const size_t NL = Q.NL, K = P.folds;
    if (NL <= 1) return R;                                     // nothing is scored: l+ = l* = 0, a curve of zero words
    if (!spec.curve()) { R.pick = R.min = lasso_argmin(P, Q, cv); return R; }
    const bool rule = spec.cv_rule == CV_RULE_ONE_SE;
    const uint32_t KL = (uint32_t)(K * NL), e = P.alloc(KL), S = P.alloc(NL), dev = P.alloc(KL), sq = P.alloc(KL), q = P.alloc(NL);
    R.mean = P.alloc(NL); R.se = P.alloc(NL);
    const uint32_t piw = rule ? P.alloc(NL) : 0;
    for (size_t k = 0; k < K; k++)
        for (size_t l = 0; l < NL; l++) P.emit(Program::mk(OP_ADD, e + (uint32_t)(k * NL + l), score + (uint32_t)(k * NL + l), L.yy + (uint32_t)k));
    for (size_t j = 0; j < (rule ? NL : 0); j++) P.emit(Program::mk(OP_CONST, piw + (uint32_t)j, P.order[j], 0));
    P.new_launch();
    for (size_t l = 0; l < NL; l++) P.emit(Program::mk(OP_SUM, S + (uint32_t)l, e + (uint32_t)l, 0, 0, (uint32_t)K, (int32_t)NL));
    P.new_launch();
    for (size_t l = 0; l < NL; l++) P.emit(idivc_rec(R.mean + (uint32_t)l, S + (uint32_t)l, (uint32_t)K, P.w));
    P.new_launch();
    for (uint32_t i = 0; i < KL; i++) P.emit(Program::mk(OP_SUB, dev + i, e + i, R.mean + (uint32_t)(i % NL)));
    P.new_launch();
    for (uint32_t i = 0; i < KL; i++) P.emit(Program::mk(OP_MUL, sq + i, dev + i, dev + i));
    P.new_launch();
    for (size_t l = 0; l < NL; l++) P.emit(Program::mk(OP_SUM, q + (uint32_t)l, sq + (uint32_t)l, 0, 0, (uint32_t)K, (int32_t)NL));
    P.new_launch();
    for (size_t l = 0; l < NL; l++) P.emit(idivc_rec(R.se + (uint32_t)l, q + (uint32_t)l, (uint32_t)(K * (K - 1)), P.w));
    P.new_launch();
    for (size_t l = 0; l < NL; l++) P.emit(Program::mk(OP_SQRT, R.se + (uint32_t)l, R.se + (uint32_t)l));
    P.new_launch();
    R.pick = R.min = lasso_argmin(P, Q, cv);
    if (!rule) return R;
    const uint32_t tm = P.alloc(2), ts = tm + 1, thr = P.alloc(1), m = P.alloc(NL), z = P.alloc(NL), hotp = P.alloc(NL), idxp = P.alloc(1);
    R.pick.hot = P.alloc(NL); R.pick.index = P.alloc(1);
    std::vector<uint32_t> pos(NL);                             // pos[l]: where l stands in pi
    for (size_t j = 0; j < NL; j++) pos[P.order[j]] = (uint32_t)j;
    P.emit(Program::mk(OP_SUM, tm, R.mean, R.min.hot, 0, (uint32_t)NL, 1, 1));
    P.emit(Program::mk(OP_SUM, ts, R.se, R.min.hot, 0, (uint32_t)NL, 1, 1));
    P.new_launch();
    P.emit(Program::mk(OP_ADD, thr, tm, ts));
    P.new_launch();
    for (size_t l = 0; l < NL; l++)                            // the two words mean_l and thr, by the stride between them
        P.emit(Program::mk(OP_MAX, m + (uint32_t)l, R.mean + (uint32_t)l, 2, 0, 2, (int32_t)(thr - (R.mean + (uint32_t)l))));
    P.new_launch();
    for (size_t l = 0; l < NL; l++) P.emit(Program::mk(OP_SUB, z + pos[l], R.mean + (uint32_t)l, m + (uint32_t)l));
    P.new_launch();
    // b = 0: against the constant zero.  idxp is a discard slot: the record shape writes the matching POSITION in pi there,
    // and nothing reads it -- l+ itself is the gated select of the constants pi_j below
    P.emit(Program::mk(OP_EQ, hotp, z, 0, idxp, (uint32_t)NL, 1));
    P.new_launch();
    for (size_t l = 0; l < NL; l++) P.emit(Program::mk(OP_COPY, R.pick.hot + (uint32_t)l, hotp + pos[l]));
    P.emit(Program::mk(OP_SUM, R.pick.index, piw, hotp, 0, (uint32_t)NL, 1, 1));
    P.new_launch();
    return R;
}

// Selection among the last fit's models (the full system's) by the one-hot words of `pick` (hot = 0: one value, nothing to
// select): beta*_i = XOR_l (hot_l & beta_{l,i}).  Then the reveal: beta* and, if asked for, the index (with the
// one-standard-error rule l+ and then l*), the scores and the curve -- nothing else.
// One value needs no selection: beta* = beta_0, every index 0 (the constant zero)
inline void lasso_select(Program &P, const Spec &spec, const LassoPlan &Q, uint32_t cv, const LassoCurve &R) {
    const size_t d = Q.d, NL = Q.NL;
    const uint32_t xs = Q.vec(Q.x, Q.NF - 1, 0);
    uint32_t best = xs;
    if (NL > 1) {
        best = P.alloc(d);
        // one record per coordinate, one AND step per value
        for (size_t i = 0; i < d; i++) P.emit(Program::mk(OP_SUM, best + (uint32_t)i, xs + (uint32_t)i, R.pick.hot, 0, (uint32_t)NL, (int32_t)d, 1));
        P.new_launch();
    }
    P.rv_beta = P.alloc_reveal(P.beta_words());
    uint32_t slot = P.rv_beta;
    for (size_t i = 0; i < d; i++) P.emit(Program::mk(OP_REVEAL, slot++, best + (uint32_t)i));
    if (spec.select_reveal & SELECT_REVEAL_INDEX) {
        P.emit(Program::mk(OP_REVEAL, slot++, R.pick.index));
        if (P.cv_rule == CV_RULE_ONE_SE) P.emit(Program::mk(OP_REVEAL, slot++, R.min.index));
    }
    if (spec.select_reveal & SELECT_REVEAL_SCORES)             // (cross-validation of one value scores nothing: the constant zero)
        for (size_t l = 0; l < NL; l++) P.emit(Program::mk(OP_REVEAL, slot++, cv + (uint32_t)(Q.scored ? l : 0)));
    if (spec.select_reveal & SELECT_REVEAL_CURVE)              // (the zero word where no curve is formed)
        for (size_t h = 0; h < 2; h++)
            for (size_t l = 0; l < NL; l++) P.emit(Program::mk(OP_REVEAL, slot++, (h ? R.se : R.mean) + (uint32_t)((h ? R.se : R.mean) ? l : 0)));
    P.new_launch();
}

inline void lower_lasso(Program &P, const Spec &spec, const Layout &L) {
    const LassoPlan Q = lasso_plan(P, spec, L);
    lasso_setup(P, spec, L, Q);
    const std::vector<uint64_t> ck = fista_coefficients(spec.iters, spec.w, spec.p);
    for (int it = 0; it < spec.iters; it++) lasso_iteration(P, spec, L, Q, it, ck[(size_t)it]);
    if (P.selects()) {
        uint32_t score = 0;
        const uint32_t cv = lasso_scores(P, L, Q, &score);
        lasso_select(P, spec, Q, cv, lasso_one_se(P, spec, L, Q, cv, score));
    }
    else P.reveal_beta(Q.x, Q.NL * Q.d);                     // the whole path, value-major
}

inline void lower_cgd(Program &P, const Spec &spec, const Layout &L) {
    // k independent recurrences on the one M: every statement below runs for all targets in the launch it has in the
    // single-target program (target t: vectors at + t * d, scalars at + t)
    const size_t d = L.d, K = L.K;
    const uint32_t D = (uint32_t)d, M = L.M, bv = L.bv;
    const int w = spec.w, iters = spec.iters;
    const uint32_t x = P.alloc(K * d), g = P.alloc(K * d), pv = P.alloc(K * d), gscl = P.alloc(K * d), pA = P.alloc(K * d),
                   tabs = P.alloc(K * d);
    const uint32_t ng = P.alloc(K), q = P.alloc(K), gp = P.alloc(K), eta = P.alloc(K), gamma = P.alloc(K),
                   gAp = P.alloc(K);
    const uint32_t sc_max = P.alloc(K * Program::max_tree_scratch(d));
    const uint32_t sc_ip = P.alloc(2 * K * Program::inner_scratch(d));
    size_t mv_waves, kara_min;
    mv_shape(P, mv_waves, kara_min);
    const uint32_t sc_dot = P.alloc_dots(K * d * d, K * d, mv_waves);
    if (spec.trace) P.rv_trace = P.alloc_reveal((size_t)iters * (d + 4));
    // Karatsuba products for A p (w = 64): the words hdiff(M[i][j]) -- once per solve -- and hdiff(p[k]) -- once per
    // iteration -- live in a shadow of the word range [M, pv + k d), kdelta words above their operands
    uint32_t kdelta = 0;
    if (w == 64 && iters > 0 && program_karatsuba() && d * d > kara_min) {   // (needs two products per record)
        kdelta = P.alloc((size_t)(pv + (uint32_t)(K * d) - M)) - M;
        for (size_t i = 0; i < d; i++)
            for (size_t j = 0; j <= i; j++) P.emit(Program::mk(OP_HDIFF, L.Mi(i, j) + kdelta, L.Mi(i, j)));
        P.new_launch();
        for (size_t i = 0; i < d; i++)
            for (size_t j = 0; j < i; j++) P.emit(Program::mk(OP_COPY, L.Mi(j, i) + kdelta, L.Mi(i, j) + kdelta));
        P.new_launch();
    }
    // cgd.oc:96-106
    for (size_t i = 0; i < K * d; i++) P.emit(Program::mk(OP_SUB, g + (uint32_t)i, 0, bv + (uint32_t)i));
    P.new_launch();
    for (size_t i = 0; i < K * d; i++) P.emit(Program::mk(OP_ABS, tabs + (uint32_t)i, g + (uint32_t)i));
    P.max_trees(K, ng, 1, tabs, D, d, sc_max);
    // g_i / max_j |g_j|: a quotient of at most 2^p.  At w = 64 the maximum is an UNSIGNED maximum of the very magnitudes
    // the divider forms (Circ::vabs, Circ::gt), so |g_i| <= |ng| holds for every input and the divider may skip the
    // quotient bits above p (OP_DIVB); at w = 32 the compare is signed (fixed.oc:78-88) and |INT_MIN| escapes it
    const uint32_t op_divb = w == 64 ? OP_DIVB : OP_DIV;
    for (size_t t = 0; t < K; t++)
        for (size_t i = 0; i < d; i++) P.emit(Program::mk(op_divb, L.tv_(pv, t) + (uint32_t)i, L.tv_(g, t) + (uint32_t)i, ng + (uint32_t)t));
    P.new_launch();
    for (int it = 0; it < iters; it++) {
        // pA = A p  (cgd.oc:119-125): d k dot products on the one M
        if (kdelta && it == 0) {                 // (later iterations: the record that makes p_i forms hdiff(p_i), below)
            for (size_t i = 0; i < K * d; i++) P.emit(Program::mk(OP_HDIFF, pv + (uint32_t)i + kdelta, pv + (uint32_t)i));
            P.new_launch();
        }
        std::vector<Program::DotJob> jobs(K * d);
        for (size_t t = 0; t < K; t++)
            for (size_t i = 0; i < d; i++) {
                Program::DotJob J = {L.tv_(pA, t) + (uint32_t)i, 0, L.Mi(i, 0), L.tv_(pv, t), D, false, kdelta};
                jobs[t * d + i] = J;
            }
        P.dots(jobs, sc_dot, mv_waves, kara_min);
        {                                        // q = <pA,p> (:128), gp = <g,p> (:130)
            std::vector<Program::IpJob> ij(2 * K);
            for (size_t t = 0; t < K; t++) {
                Program::IpJob j0 = {q + (uint32_t)t, L.tv_(pA, t), L.tv_(pv, t)}, j1 = {gp + (uint32_t)t, L.tv_(g, t), L.tv_(pv, t)};
                ij[2 * t] = j0; ij[2 * t + 1] = j1;
            }
            P.inners(ij, d, sc_ip);
        }
        for (size_t t = 0; t < K; t++) P.emit(Program::mk(OP_DIV, eta + (uint32_t)t, gp + (uint32_t)t, q + (uint32_t)t)); // :133
        P.new_launch();
        for (size_t t = 0; t < K; t++)
            for (size_t i = 0; i < d; i++) {     // :141-145
                const uint32_t xi = L.tv_(x, t) + (uint32_t)i, gi = L.tv_(g, t) + (uint32_t)i;
                P.emit(Program::mk(OP_MULSUB, xi, L.tv_(pv, t) + (uint32_t)i, eta + (uint32_t)t, xi));
                // ... and |g_i| with it (cnt = 2): the maximum below starts from these
                P.emit(Program::mk(OP_MULSUB, gi, eta + (uint32_t)t, L.tv_(pA, t) + (uint32_t)i, gi, 2, (int32_t)(tabs - g)));
            }
        P.max_trees(K, ng, 1, tabs, D, d, sc_max);   // :140,146-149  (opens a launch of its own)
        for (size_t t = 0; t < K; t++)
            for (size_t i = 0; i < d; i++)       // :153-155
                P.emit(Program::mk(op_divb, L.tv_(gscl, t) + (uint32_t)i, L.tv_(g, t) + (uint32_t)i, ng + (uint32_t)t));
        P.new_launch();
        {                                        // :157
            std::vector<Program::IpJob> ij(K);
            for (size_t t = 0; t < K; t++) { Program::IpJob j = {gAp + (uint32_t)t, L.tv_(pA, t), L.tv_(gscl, t)}; ij[t] = j; }
            P.inners(ij, d, sc_ip);
        }
        for (size_t t = 0; t < K; t++) P.emit(Program::mk(OP_DIV, gamma + (uint32_t)t, gAp + (uint32_t)t, q + (uint32_t)t));  // :159
        P.new_launch();
        for (size_t t = 0; t < K; t++)
            for (size_t i = 0; i < d; i++)       // :162-165
                P.emit(Program::mk(OP_MULSUB, L.tv_(pv, t) + (uint32_t)i, L.tv_(pv, t) + (uint32_t)i, gamma + (uint32_t)t,
                                   L.tv_(gscl, t) + (uint32_t)i, kdelta ? 3u : 1u, kdelta ? (int32_t)kdelta : 1));
        P.new_launch();
        if (spec.trace) {                        // reveals at :167-189 (single-target programs only)
            uint32_t base = P.rv_trace + (uint32_t)((size_t)it * (d + 4));
            for (size_t i = 0; i < d; i++) P.emit(Program::mk(OP_REVEAL, base + (uint32_t)i, x + (uint32_t)i));
            P.emit(Program::mk(OP_REVEAL, base + D, gamma));
            P.emit(Program::mk(OP_REVEAL, base + D + 1, eta));
            P.emit(Program::mk(OP_REVEAL, base + D + 2, q));
            P.emit(Program::mk(OP_REVEAL, base + D + 3, ng));
            P.new_launch();
        }
        P.mark_iteration();
    }
    P.reveal_beta(x, K * d);
}

// Karatsuba products in the factorisations (w = 64, large d): see lower_cholesky
inline bool fact_karatsuba(int w, size_t d) { return w == 64 && program_karatsuba() && (d / 2) * (d / 2 + 1) >= 2 * 4096; }

// Column j of a factorisation, L_ij -= <row i of L, v> for i >= j, and step j of every target's forward substitution,
// rhs_t[j] -= <row j of L, sol_t>: one batch of dot products (v: row j of L for Cholesky, L_jk D_k for LDL^T)
struct Inference;
inline void inference_column_jobs(const Layout &L, const Inference &I, size_t i, uint32_t kdelta, std::vector<Program::DotJob> &jobs);
inline void column_dots(Program &P, const Layout &L, size_t j, uint32_t v, uint32_t rhs, uint32_t sol, uint32_t sc_dot, uint32_t kdelta,
                        const Inference *inf = 0) {
    std::vector<Program::DotJob> jobs;
    for (size_t i = j; i < L.d; i++) {
        Program::DotJob J = {L.Mi(i, j), L.Mi(i, j), L.Mi(i, 0), v, (uint32_t)j, true, kdelta};
        jobs.push_back(J);
    }
    for (size_t t = 0; t < L.K; t++) {
        Program::DotJob F = {L.tv_(rhs, t) + (uint32_t)j, L.tv_(rhs, t) + (uint32_t)j, L.Mi(j, 0), L.tv_(sol, t), (uint32_t)j, true, kdelta};
        jobs.push_back(F);
    }
    if (inf) inference_column_jobs(L, *inf, j, kdelta, jobs);
    P.dots(jobs, sc_dot, kFactRecords, 4096);
}

// The dot products of step ii of the k back substitutions, rhs_t[ii] -= sum_{k > ii} L^T_{ii,k} sol_t[k] (row ii of M right
// of the diagonal, read stride-1), each shaped as a single one's (64 records per target): a step costs what it costs with
// one target as long as the chip has room
inline void back_dots(Program &P, const Layout &L, size_t ii, uint32_t rhs, uint32_t sol, uint32_t sc_dot) {
    std::vector<Program::DotJob> jobs(L.K);
    for (size_t t = 0; t < L.K; t++) {
        Program::DotJob J = {L.tv_(rhs, t) + (uint32_t)ii, L.tv_(rhs, t) + (uint32_t)ii, L.Mi(ii, ii + 1), L.tv_(sol, t) + (uint32_t)(ii + 1),
                             (uint32_t)(L.d - 1 - ii), true};
        jobs[t] = J;
    }
    P.dots(jobs, sc_dot, 64 * L.K);
}

// Inference on the Cholesky solve (linreg_gc_inference.h).  Column j of L^-1 is z_j = L^-1 e_j: z_j[j] =
// div(2^p, L_jj), z_j[i] = div(0 - sum_{k=j}^{i-1} mul(L_ik, z_j[k]), L_ii) -- the forward substitution of a unit vector with
// its structural zeros left out.  z_j lies at Z + j d, stride 1 in i, so step i of column j is a dot product of row i of L
// from column j with z_j from its diagonal on: inference_column_jobs, which ride in column i's batch
struct Inference { int bits = 0; uint32_t Z = 0, one = 0, lam = 0, rs = 0; uint64_t lambda_fixed = 0; };
inline void inference_column_jobs(const Layout &L, const Inference &I, size_t i, uint32_t kdelta, std::vector<Program::DotJob> &jobs) {
    for (size_t j = 0; j < ((I.bits & INFER_SE) ? i : 0); j++) {
        const uint32_t zji = I.Z + (uint32_t)(j * L.d + i);
        Program::DotJob J = {zji, 0, L.Mi(i, j), I.Z + (uint32_t)(j * L.d + j), (uint32_t)(i - j), true, kdelta};   // base: the constant zero
        jobs.push_back(J);
    }
}
// The tail behind the back substitution: v_j = |z_j|^2, b0^T beta and beta^T beta in one batch of plain products (beta has no
// half-difference words); e = Y - b0^T beta - mul(beta^T beta, q(lambda)) (the last term absent when q(lambda) = 0: mul by a
// constant word is Circ::mulc bit for bit); s2 = mul(e, q(resid_scale)) beside div(e, Y); the d products mul(s2, v_j) beside
// r2 = 2^p - div(e, Y); the d square roots; ONE reveal launch: beta, then u, then s2 and r2
inline void inference_tail(Program &P, const Layout &L, const Inference &I, uint32_t beta) {
    const size_t d = L.d, nv = (I.bits & INFER_SE) ? d : 0;
    const bool fit = (I.bits & INFER_FIT) != 0;
    const uint32_t v = P.alloc(nv), bb = P.alloc(2), qq = bb + 1, e = P.alloc(2), t = e + 1, s2 = P.alloc(1), r2 = P.alloc(1), u = P.alloc(nv);
    const uint32_t sc = P.alloc_dots(nv * (nv + 1) / 2 + 2 * d, nv + 2, kTargetWaves, 8 * d + 16);
    std::vector<Program::DotJob> jobs;
    for (size_t j = 0; j < nv; j++) {
        const uint32_t zjj = I.Z + (uint32_t)(j * d + j);
        Program::DotJob J = {v + (uint32_t)j, 0, zjj, zjj, (uint32_t)(d - j), false};
        jobs.push_back(J);
    }
    Program::DotJob B = {bb, 0, L.b0, beta, (uint32_t)d, false}, Q = {qq, 0, beta, beta, (uint32_t)d, false};
    jobs.push_back(B);
    if (I.lambda_fixed) jobs.push_back(Q);
    P.dots(jobs, sc, kTargetWaves);
    P.emit(Program::mk(OP_SUB, e, L.Y, bb));
    if (I.lambda_fixed) {
        P.emit(Program::mk(OP_MUL, t, qq, I.lam));
        P.new_launch();
        P.emit(Program::mk(OP_SUB, e, e, t));
    }
    P.new_launch();
    P.emit(Program::mk(OP_MUL, s2, e, I.rs));
    if (fit) P.emit(Program::mk(OP_DIV, r2, e, L.Y));
    P.new_launch();
    for (size_t j = 0; j < nv; j++) P.emit(Program::mk(OP_MUL, u + (uint32_t)j, s2, v + (uint32_t)j));
    if (fit) P.emit(Program::mk(OP_SUB, r2, I.one, r2));
    P.new_launch();
    for (size_t j = 0; j < nv; j++) P.emit(Program::mk(OP_SQRT, u + (uint32_t)j, u + (uint32_t)j));
    P.new_launch();
    P.beta_at = beta;
    P.rv_beta = P.alloc_reveal(d + P.infer_words());
    for (size_t i = 0; i < d; i++) P.emit(Program::mk(OP_REVEAL, P.rv_beta + (uint32_t)i, beta + (uint32_t)i));
    for (size_t j = 0; j < nv; j++) P.emit(Program::mk(OP_REVEAL, P.rv_beta + (uint32_t)(d + j), u + (uint32_t)j));
    if (fit) {
        P.emit(Program::mk(OP_REVEAL, P.rv_beta + (uint32_t)(d + nv), s2));
        P.emit(Program::mk(OP_REVEAL, P.rv_beta + (uint32_t)(d + nv + 1), r2));
    }
    P.new_launch();
}

// inf: the inference request (Spec::infer != 0; one target), or 0 -- the plain solve, record for record what it has always been
inline void lower_cholesky(Program &P, const Layout &L, const Spec *inf = 0) {
    const size_t d = L.d, K = L.K;
    const uint32_t M = L.M, bv = L.bv;
    Inference I;
    if (inf) { I.bits = inf->infer; I.lambda_fixed = inf->lambda_fixed; }
    const bool se = (I.bits & INFER_SE) != 0;
    // (the inverse columns lie behind y, inside the one Karatsuba shadow: [M, y + k d) becomes [M, Z + d d))
    const uint32_t y = P.alloc(K * d);
    if (se) I.Z = P.alloc(d * d);
    const uint32_t beta = P.alloc(K * d);
    if (inf) { I.one = P.alloc(3); I.lam = I.one + 1; I.rs = I.one + 2; }
    // (with the inverse columns a column's batch holds up to d (d + 1) / 2 more products in d more jobs)
    const uint32_t sc_dot = se ? P.alloc_dots(d * d + d * (d + 1) / 2 + K * d, 2 * d + K, kFactRecords, 8 * K * d + 16)
                               : P.alloc_dots(d * d + K * d, d + K, kFactRecords, 4 * K * d + 8);
    // Karatsuba products in the factorisation (w = 64, large d): an entry L_kj -- and y_j -- is final once column j has
    // been scaled, so its hdiff word (shadow of [M, y + k d), kdelta words up) is formed in the launch that mirrors the
    // column (independent of the copies: no launch is added to the chain); columns with fewer than two products per
    // record keep the plain array (dots()).  The back substitution (one short dot product per step) is left as it is.
    uint32_t kdelta = 0;
    if (fact_karatsuba(P.w, d)) kdelta = P.alloc((size_t)(y + (uint32_t)(K * d + (se ? d * d : 0)) - M)) - M;
    // cholesky.oc:51-65 (factorisation) and :68-76 (forward substitution) as ONE chain of launches: step j of
    // the forward substitution, y_j = (b_j - sum_{k<j} L_jk y_k) / L_jj, needs row j of L (complete once
    // column j - 1 has been scaled) and y_0..y_{j-1}, so its dot product joins the dot products of column
    // j and its division joins the launch that scales column j.  Same operations on the same operands as
    // the reference's three loops (results identical); d division launches and 2d narrow launches fewer
    // on the dependent chain, which is what a small system's run time consists of.  With k targets, step j of
    // every target's forward substitution rides in the same two launches.
    for (size_t j = 0; j < d; j++) {
        if (j > 0) column_dots(P, L, j, L.Mi(j, 0), bv, y, sc_dot, kdelta, inf ? &I : 0);      // ... and b_j -= <L_j., y> (:70-73)
        P.emit(Program::mk(OP_SQRT, L.Mi(j, j), L.Mi(j, j)));
        if (inf && j == 0) {                     // the public constants of the inference, beside the first square root
            const uint64_t one = 1ull << P.p;
            P.emit(Program::mk(OP_CONST, I.one, (uint32_t)one, (uint32_t)(one >> 32)));
            P.emit(Program::mk(OP_CONST, I.lam, (uint32_t)I.lambda_fixed, (uint32_t)(I.lambda_fixed >> 32)));
            P.emit(Program::mk(OP_CONST, I.rs, (uint32_t)inf->resid_fixed, (uint32_t)(inf->resid_fixed >> 32)));
        }
        P.new_launch();
        // the division record stores its quotient twice (L_kj and its mirror L^T_jk, read stride-1 by the back
        // substitution) and, with Karatsuba products, its half-difference word: rounds 3-4 did both in a launch of
        // their own behind the divisions -- one more dependent launch per column, each of which waits for CUs beside
        // the other role's MAC kernel of that column
        const uint32_t hc = kdelta ? 2u : 1u;
        for (size_t k = j + 1; k < d; k++) P.emit(Program::mk(OP_DIV, L.Mi(k, j), L.Mi(k, j), L.Mi(j, j), L.Mi(j, k), hc, (int32_t)kdelta));
        for (size_t t = 0; t < K; t++)                                                                               // :75
            P.emit(Program::mk(OP_DIV, L.tv_(y, t) + (uint32_t)j, L.tv_(bv, t) + (uint32_t)j, L.Mi(j, j), 0, hc, (int32_t)kdelta));
        // step j of the inverse columns 0 .. j - 1, in place on the sums of this column's batch, and z_j[j]: d + 1 records in all
        for (size_t c = 0; c < (se ? j : 0); c++)
            P.emit(Program::mk(OP_DIV, I.Z + (uint32_t)(c * d + j), I.Z + (uint32_t)(c * d + j), L.Mi(j, j), 0, hc, (int32_t)kdelta));
        if (se) P.emit(Program::mk(OP_DIV, I.Z + (uint32_t)(j * d + j), I.one, L.Mi(j, j), 0, hc, (int32_t)kdelta));
        P.new_launch();
    }
    // :79-87.  The k back substitutions share each step's launches
    for (size_t ii = d; ii-- > 0;) {
        if (ii + 1 < d) back_dots(P, L, ii, y, beta, sc_dot);
        for (size_t t = 0; t < K; t++) P.emit(Program::mk(OP_DIV, L.tv_(beta, t) + (uint32_t)ii, L.tv_(y, t) + (uint32_t)ii, L.Mi(ii, ii)));
        P.new_launch();
    }
    if (inf) inference_tail(P, L, I, beta);
    else P.reveal_beta(beta, K * d);
}

inline void lower_ldlt(Program &P, const Layout &L) {
    const size_t d = L.d, K = L.K;
    const uint32_t D = (uint32_t)d, M = L.M, bv = L.bv;
    const uint32_t tv = P.alloc(d);
    const uint32_t sc_dot = P.alloc_dots(d * d + K * d, d + K, kFactRecords, 4 * K * d + 8);
    // Karatsuba products as in the Cholesky lowering: hdiff of L_kj in the launch that mirrors column j, of b_j (final
    // after step j of the forward substitution) and of the products t_k = L_jk D_k in a launch of their own per column
    uint32_t kdelta = 0;
    if (fact_karatsuba(P.w, d)) kdelta = P.alloc((size_t)(tv + D - M)) - M;
    for (size_t j = 0; j < d; j++) {             // ldlt.oc:50-64
        if (j > 0) {
            // t_k = L_jk D_k with its half-difference word from the same record; hdiff(b_{j-1}) (final since step j - 1 of
            // the forward substitution) rides in the same launch: one launch where rounds 3-4 had two
            for (size_t k = 0; k < j; k++) P.emit(Program::mk(OP_MUL, tv + (uint32_t)k, L.Mi(j, k), L.Mi(k, k), 0, kdelta ? 2u : 1u, (int32_t)kdelta));
            if (kdelta)
                for (size_t t = 0; t < K; t++)
                    P.emit(Program::mk(OP_HDIFF, L.tv_(bv, t) + (uint32_t)(j - 1) + kdelta, L.tv_(bv, t) + (uint32_t)(j - 1)));
            P.new_launch();
            // step j of the forward substitution (:67-73), b_j -= sum_{k<j} L_jk b_k, needs row j of L (complete once
            // column j - 1 has been scaled) and b_0 .. b_{j-1}: it joins the dot products of column j instead of
            // forming a chain of d - 1 launch pairs of its own after the factorisation (as in the Cholesky lowering)
            column_dots(P, L, j, tv, bv, bv, sc_dot, kdelta);
        }
        for (size_t k = j + 1; k < d; k++) P.emit(Program::mk(OP_DIV, L.Mi(k, j), L.Mi(k, j), L.Mi(j, j), L.Mi(j, k), kdelta ? 2u : 1u, (int32_t)kdelta));
        P.new_launch();
    }
    for (size_t t = 0; t < K; t++)               // :76-79
        for (size_t i = 0; i < d; i++)
            P.emit(Program::mk(OP_DIV, L.tv_(bv, t) + (uint32_t)i, L.tv_(bv, t) + (uint32_t)i, L.Mi(i, i)));
    P.new_launch();
    // :82-90 (as in the Cholesky lowering: all targets in each step's launches)
    for (size_t ii = d; ii-- > 0;)
        if (ii + 1 < d) back_dots(P, L, ii, bv, bv, sc_dot);
    P.reveal_beta(bv, K * d);
}

// ---- association scan (linreg_gc_scan.h).  c = d - 1 covariates shared by M candidate columns; candidate m is
// fitted in the system [C, g_m] of size d.  The c x c block is assembled, factored and forward-substituted once, as the plain
// Cholesky lowering does it (same records on the same operands); candidate m is one more ROW of the factor, u_m = row m of U
// (M x c, row-major: a row of U and a row of L are both stride 1), and rows never meet one another.  Step k of all M rows rides
// in covariate column k's batch of dot products and in its division launch (as the right-hand sides of several targets ride);
// a tail follows the last covariate column: one batch of 2 M dot products of length c (plus E0's with SCAN_SE), M square
// roots, the divisions, and with SCAN_SE the products and square roots of the scan words.  Every share is
// [A (T_c)] [b (c)] [yy] [h_0 (c)] .. [h_{M-1} (c)] [gg (M)] [gy (M)]; the normaliser is d
inline void lower_scan(Program &P, const Spec &spec) {
    const size_t d = spec.d, c = d - 1, M = P.scan, Tc = c * (c + 1) / 2, IN = P.in_words();
    const bool normalize = spec.normalize != 0, se = (P.scan_bits & SCAN_SE) != 0;
    const uint32_t oH = (uint32_t)(Tc + c + 1), oGG = oH + (uint32_t)(M * c), oGY = oGG + (uint32_t)M, oYY = (uint32_t)(Tc + c);
    // the share sums, laid out as a share is (on the data-provider path they are the prefix a division by d is applied to)
    const uint32_t S = P.alloc(IN);
    Layout L = {c, 1, P.alloc(c * c), P.alloc(c)};
    // [L.M, end of gy): the words the dot products read, the one range a Karatsuba shadow covers
    const uint32_t y = P.alloc(c), U = P.alloc(M * c), gg = P.alloc(M), gy = P.alloc(M), shadow_end = gy + (uint32_t)M;
    // P.dots decides per batch (more than 4096 products) whether the products are Karatsuba pairs; the shadow exists where the
    // largest batch, the tail's, can pass that rule
    uint32_t kdelta = 0;
    if (P.w == 64 && program_karatsuba() && 2 * M * c + c > 4096) kdelta = P.alloc((size_t)(shadow_end - L.M)) - L.M;
    const uint32_t hc = kdelta ? 2u : 1u;
    const uint32_t lam = P.alloc(1), one = P.alloc(1), rs = P.alloc(1), E0 = P.alloc(1);
    const uint32_t t = P.alloc(M), beta = P.alloc(M);
    const uint32_t z = P.alloc(se ? M : 0), v = P.alloc(se ? M : 0), e = P.alloc(se ? M : 0), wv = P.alloc(se ? M : 0);
    const uint32_t sc_dot = P.alloc_dots(c * c + c + 2 * M * c + c, 2 * M + c + 2, kFactRecords, 8 * (M + c) + 16);
    // share sums
    P.new_launch();
    for (size_t i = 0; i < IN; i++) P.emit(Program::mk(OP_SUM, S + (uint32_t)i, P.in_base + (uint32_t)i, 0, 0, (uint32_t)P.nshares, (int32_t)IN));
    P.new_launch();
    const SysAt sums = packed_at(c, S);
    if (normalize) {
        // everything but the diagonals A_kk and gg_m is divided by the public normaliser d = c + 1
        for (size_t i = 0; i < c; i++)
            for (size_t j = 0; j < i; j++) P.emit(idivc_rec(sums.a(i, j), sums.a(i, j), (uint32_t)d, P.w));
        for (size_t i = 0; i < c + 1 + M * c; i++) P.emit(idivc_rec(sums.b + (uint32_t)i, sums.b + (uint32_t)i, (uint32_t)d, P.w));   // b, yy, H
        for (size_t m = 0; m < M; m++) P.emit(idivc_rec(S + oGY + (uint32_t)m, S + oGY + (uint32_t)m, (uint32_t)d, P.w));
        close_prefix(P, S + (uint32_t)IN);
    }
    if (normalize) {
        P.lam_rec = (uint32_t)P.recs.size();
        P.emit(Program::mk(OP_CONST, lam, (uint32_t)spec.lambda_fixed, (uint32_t)(spec.lambda_fixed >> 32)));
    }
    if (se) {
        const uint64_t o = 1ull << P.p;
        P.emit(Program::mk(OP_CONST, one, (uint32_t)o, (uint32_t)(o >> 32)));
        P.emit(Program::mk(OP_CONST, rs, (uint32_t)spec.resid_fixed, (uint32_t)(spec.resid_fixed >> 32)));
    }
    P.new_launch();
    // the mirror launch: the c x c block into full symmetric storage with lambda on its diagonal, b, and the candidates' words
    // to where the solve overwrites them (the two-party path takes the words as given: its diagonals are copied)
    const uint32_t dop = normalize ? OP_ADD : OP_COPY, dlam = normalize ? lam : 0;
    for (size_t i = 0; i < c; i++) P.emit(Program::mk(dop, L.Mi(i, i), sums.a(i, i), dlam));
    for (size_t i = 0; i < c; i++)
        for (size_t j = 0; j < i; j++) {
            P.emit(Program::mk(OP_COPY, L.Mi(i, j), sums.a(i, j)));
            P.emit(Program::mk(OP_COPY, L.Mi(j, i), sums.a(i, j)));
        }
    for (size_t i = 0; i < c; i++) P.emit(Program::mk(OP_COPY, L.bv + (uint32_t)i, sums.b + (uint32_t)i));
    for (size_t i = 0; i < M * c; i++) P.emit(Program::mk(OP_COPY, U + (uint32_t)i, S + oH + (uint32_t)i));
    for (size_t m = 0; m < M; m++) P.emit(Program::mk(dop, gg + (uint32_t)m, S + oGG + (uint32_t)m, dlam));
    for (size_t m = 0; m < M; m++) P.emit(Program::mk(OP_COPY, gy + (uint32_t)m, S + oGY + (uint32_t)m));
    P.new_launch();
    // the shared factorisation and forward substitution (lower_cholesky's chain), with step k of every candidate row
    for (size_t k = 0; k < c; k++) {
        if (k > 0) {
            std::vector<Program::DotJob> jobs;
            for (size_t i = k; i < c; i++) {
                Program::DotJob J = {L.Mi(i, k), L.Mi(i, k), L.Mi(i, 0), L.Mi(k, 0), (uint32_t)k, true, kdelta};
                jobs.push_back(J);
            }
            Program::DotJob F = {L.bv + (uint32_t)k, L.bv + (uint32_t)k, L.Mi(k, 0), y, (uint32_t)k, true, kdelta};
            jobs.push_back(F);
            for (size_t m = 0; m < M; m++) {         // h_m[k] -= <row m of U, row k of L>: row c of the augmented factor
                const uint32_t um = U + (uint32_t)(m * c);
                Program::DotJob J = {um + (uint32_t)k, um + (uint32_t)k, um, L.Mi(k, 0), (uint32_t)k, true, kdelta};
                jobs.push_back(J);
            }
            P.dots(jobs, sc_dot, kFactRecords, 4096);
        }
        P.emit(Program::mk(OP_SQRT, L.Mi(k, k), L.Mi(k, k)));
        P.new_launch();
        for (size_t i = k + 1; i < c; i++) P.emit(Program::mk(OP_DIV, L.Mi(i, k), L.Mi(i, k), L.Mi(k, k), L.Mi(k, i), hc, (int32_t)kdelta));
        P.emit(Program::mk(OP_DIV, y + (uint32_t)k, L.bv + (uint32_t)k, L.Mi(k, k), 0, hc, (int32_t)kdelta));
        for (size_t m = 0; m < M; m++) {
            const uint32_t umk = U + (uint32_t)(m * c + k);
            P.emit(Program::mk(OP_DIV, umk, umk, L.Mi(k, k), 0, hc, (int32_t)kdelta));
        }
        P.new_launch();
    }
    // the tail: gg_m -= |u_m|^2, gy_m -= <u_m, y>, and E0 = Y - |y|^2 in one batch
    {
        std::vector<Program::DotJob> jobs;
        for (size_t m = 0; m < M; m++) {
            const uint32_t um = U + (uint32_t)(m * c);
            Program::DotJob G = {gg + (uint32_t)m, gg + (uint32_t)m, um, um, (uint32_t)c, true, kdelta};
            jobs.push_back(G);
        }
        for (size_t m = 0; m < M; m++) {
            Program::DotJob G = {gy + (uint32_t)m, gy + (uint32_t)m, U + (uint32_t)(m * c), y, (uint32_t)c, true, kdelta};
            jobs.push_back(G);
        }
        if (se) { Program::DotJob G = {E0, S + oYY, y, y, (uint32_t)c, true, kdelta}; jobs.push_back(G); }
        P.dots(jobs, sc_dot, kFactRecords, 4096);
    }
    for (size_t m = 0; m < M; m++) P.emit(Program::mk(OP_SQRT, gg + (uint32_t)m, gg + (uint32_t)m));                      // l_m
    P.new_launch();
    for (size_t m = 0; m < M; m++) P.emit(Program::mk(OP_DIV, t + (uint32_t)m, gy + (uint32_t)m, gg + (uint32_t)m));       // t_m
    for (size_t m = 0; m < (se ? M : 0); m++) P.emit(Program::mk(OP_DIV, z + (uint32_t)m, one, gg + (uint32_t)m));        // z_m
    P.new_launch();
    for (size_t m = 0; m < M; m++) P.emit(Program::mk(OP_DIV, beta + (uint32_t)m, t + (uint32_t)m, gg + (uint32_t)m));
    if (!se) P.new_launch();
    if (se) {                                // v_m and mul(t_m, t_m) beside the last division
        for (size_t m = 0; m < M; m++) P.emit(Program::mk(OP_MUL, v + (uint32_t)m, z + (uint32_t)m, z + (uint32_t)m));
        for (size_t m = 0; m < M; m++) P.emit(Program::mk(OP_MUL, e + (uint32_t)m, t + (uint32_t)m, t + (uint32_t)m));
        P.new_launch();
        for (size_t m = 0; m < M; m++) P.emit(Program::mk(OP_SUB, e + (uint32_t)m, E0, e + (uint32_t)m));                   // e_m
        P.new_launch();
        for (size_t m = 0; m < M; m++) P.emit(Program::mk(OP_MUL, e + (uint32_t)m, e + (uint32_t)m, rs));                   // s2_m
        P.new_launch();
        for (size_t m = 0; m < M; m++) P.emit(Program::mk(OP_MUL, wv + (uint32_t)m, e + (uint32_t)m, v + (uint32_t)m));
        P.new_launch();
        for (size_t m = 0; m < M; m++) P.emit(Program::mk(OP_SQRT, wv + (uint32_t)m, wv + (uint32_t)m));                   // w_m
        P.new_launch();
    }
    P.beta_at = beta;
    P.rv_beta = P.alloc_reveal(P.beta_words());
    for (size_t m = 0; m < M; m++) P.emit(Program::mk(OP_REVEAL, P.rv_beta + (uint32_t)m, beta + (uint32_t)m));
    for (size_t m = 0; m < (se ? M : 0); m++) P.emit(Program::mk(OP_REVEAL, P.rv_beta + (uint32_t)(M + m), wv + (uint32_t)m));
    P.new_launch();
}

// Build the whole phase-2 program
inline void build_program(Program &P, const Spec &spec) {
    P.w = spec.w; P.p = spec.p; P.d = spec.d; P.nshares = spec.nshares; P.targets = spec.targets;
    P.path = spec.alg == ALG_LASSO && spec.l1_path ? spec.l1_count : 1;
    P.validate = spec.alg == ALG_LASSO && spec.validate;
    P.folds = spec.alg == ALG_LASSO ? spec.folds : 0;
    P.infer = spec.alg == ALG_CHOLESKY ? spec.infer : 0;
    P.scan = spec.alg == ALG_CHOLESKY ? spec.scan : 0;
    P.scan_bits = P.scan ? spec.scan_bits : 0;
    P.resid_fixed = P.infer || (P.scan_bits & SCAN_SE) ? spec.resid_fixed : 0;
    P.yy = P.folds && spec.yy;
    P.cv_rule = P.yy ? spec.cv_rule : CV_RULE_MIN;
    if (P.cv_rule == CV_RULE_ONE_SE) {
        // pi: the values by decreasing penalty, compared as the unsigned words they were quantised to; ties to the smaller l
        for (size_t l = 0; l < P.path; l++) P.order.push_back((uint32_t)l);
        const uint64_t *v = spec.l1_path;
        if (v) std::stable_sort(P.order.begin(), P.order.end(), [v](uint32_t x, uint32_t y) { return v[x] > v[y]; });
    }
    P.select_reveal = P.selects() ? spec.select_reveal : 0;
    P.T = spec.d * (spec.d + 1) / 2;
    // word 0 is the constant zero (the word file starts zeroed on both sides)
    P.in_base = P.alloc(spec.nshares * P.in_words());
    if (spec.alg == ALG_DIMCHECK) { lower_dimcheck(P); return; }
    if (P.scan) { lower_scan(P, spec); return; }
    const Layout L = lower_inputs(P, spec);
    switch (spec.alg) {
    case ALG_LASSO: lower_lasso(P, spec, L); break;
    case ALG_CGD: lower_cgd(P, spec, L); break;
    case ALG_CHOLESKY: lower_cholesky(P, L, P.infer ? &spec : 0); break;
    default: lower_ldlt(P, L); break;        // ALG_LDLT
    }
}

// `count` circuits of the per-lambda sweep in one program.  lambda is a public constant
// added to the diagonal AFTER the shares are summed (linear.oc:52-57), so the input labels and the garbled
// share summation -- P0's shared prefix -- exist once and every circuit starts from the same sums: the
// data providers run ONE label OT whatever the number of lambdas.  Circuit t uses words x + t * word_stride
// for x >= shared_end and decode slots r + t * reveal_stride, and differs only in the OP_CONST record that
// holds lambda.  The records of all circuits of one launch of P0 share a launch, so the dependent chains
// (dividers, reveals) of different circuits fill the GPU together.
// first_copy: index of this program's first circuit in the whole sweep.  Ranks of a multi-GPU sweep share
// the prefix -- hence the garbler's offset R -- so their gate ids must not collide.  The number of gate steps a
// circuit lowers to depends on the size of the block it is merged into (merge_hint shapes the dot-product
// records), so the ranges are laid out on a CANONICAL stride that no lowering reaches: circuit k of the sweep
// owns gate steps inside [prefix + k * kSweepCircuitStride, prefix + (k + 1) * kSweepCircuitStride) on whichever
// rank and in whichever block it runs -- blocks of different sizes cannot overlap (round 3 used the block's own
// per-circuit count as the stride; two blocks whose sizes differed by one then shared gate ids under one R).
// Step numbers only enter the hash tweaks (64 * step + lane < 2^59 with at most 65536 circuits) and, as differences
// within a launch, the table rows.  Returns false when a circuit does not fit its stride.
static const uint64_t kSweepCircuitStride = 1ull << 36;
// sys_remap (ridge cross-validation): circuit t mirrors its system from the packed words sys_remap->off[t] above the ones P0
// mirrors from, [lo, lo + len) inside the shared prefix -- the OP_ADD / OP_COPY records that read those words are moved
struct SysRemap { uint32_t lo, len; const uint32_t *off; };
inline bool replicate_program(Program &P, const Program &P0, size_t count, const uint64_t *lambda_fixed, size_t first_copy = 0,
                              const SysRemap *sys_remap = 0) {
    P.w = P0.w; P.p = P0.p; P.d = P0.d; P.T = P0.T; P.nshares = P0.nshares;
    P.cap_steps = P0.cap_steps;
    P.shared_end = P0.shared_end;
    P.word_stride = P0.n_words - P0.shared_end;
    P.reveal_stride = P0.n_reveal;
    P.replicas = (uint32_t)count;
    P.n_words = P0.shared_end + (uint32_t)count * P.word_stride;
    P.n_reveal = (uint32_t)count * P.reveal_stride;
    P.in_base = P0.in_base; P.rv_beta = P0.rv_beta; P.rv_trace = P0.rv_trace; P.rv_ab = P0.rv_ab;
    P.lam_rec = ~0u;
    if (P0.prefix_steps >= kSweepCircuitStride || P0.total_steps - P0.prefix_steps > kSweepCircuitStride || first_copy + count > 65536)
        return false;
    size_t next_iter = 0;
    const uint32_t shared_end = P0.shared_end;
    {   // 6.4 M records (257 MB) for 64 circuits of d = 100 CGD-15: grown by doubling, the vector copied itself twice over
        size_t npre = 0;
        for (size_t li = 0; li < P0.prefix_launches && li < P0.launches.size(); li++) npre += P0.launches[li].nrec;
        P.recs.reserve(npre + (P0.recs.size() - npre) * count);
    }
    for (size_t li = 0; li < P0.launches.size(); li++) {
        const Launch &L = P0.launches[li];
        const bool prefix = li < P0.prefix_launches;
        if (li == P0.prefix_launches) {
            P.new_launch();
            P.prefix_launches = (uint32_t)P.launches.size();
            P.prefix_steps = P.total_steps;
            P.step_cursor = P0.prefix_steps + (uint64_t)first_copy * kSweepCircuitStride;
        }
        // a merged launch that exceeds the table cap is cut into EQUAL pieces (a ragged last piece of a MAC launch would
        // be a launch of a few hundred records: most of the chip idle, or the wrong kernel altogether)
        const uint64_t cap_keep = P.cap_steps;
        const uint64_t cap_l = L.mac_only || cap_keep < kGenericCapSteps ? cap_keep : kGenericCapSteps;   // (as in Program::emit)
        if (!prefix && L.nrec) {
            const uint64_t tot = L.steps * (uint64_t)count, pieces = (tot + cap_l - 1) / cap_l;
            uint64_t smax = 0;
            for (uint32_t k = 0; k < L.nrec; k++) { uint64_t s1, g1; P.cost(P0.recs[L.first_rec + k], s1, g1); if (s1 > smax) smax = s1; }
            uint64_t best_pieces = pieces;
            if (L.mac_only && pieces >= 1 && (uint64_t)L.nrec * count >= 2 * 4096) {
                // MAC launches run in whole rounds of the chip (dots()): among a few piece counts take the cheapest
                double best = -1.0;
                const uint64_t R = (uint64_t)L.nrec * count;
                for (uint64_t q = pieces; q <= pieces + 3; q++) {
                    const size_t per = (size_t)((R + q - 1) / q);
                    if ((uint64_t)per * smax > cap_l) continue;
                    const double c_est = (double)q * ((double)smax * (64.0 * Program::round_cost(per, 4096) + 24.0 * Program::round_cost(per, 3072)) + 3e2);
                    if (best < 0 || c_est < best) { best = c_est; best_pieces = q; }
                }
            }
            if (best_pieces > 1) {
                const uint64_t soft = (tot + best_pieces - 1) / best_pieces + smax;
                if (soft < cap_l) P.cap_steps = soft;
            }
        }
        // record-major: record k of every circuit, then record k + 1 ... -- the records of a launch are independent, and
        // equal records side by side make the rounds of a MAC launch uniform (dots() sorts them by length)
        for (uint32_t k = 0; k < L.nrec; k++) {
            for (size_t t = 0; t < (prefix ? 1 : count); t++) {
                const uint32_t wo = (uint32_t)t * P.word_stride, ro = (uint32_t)t * P.reveal_stride;
                Rec r = P0.recs[L.first_rec + k];
                auto mv = [wo, shared_end](uint32_t x) { return x >= shared_end ? x + wo : x; };
                switch (r.op) {
                case OP_CONST:
                    r.dst = mv(r.dst);
                    if (L.first_rec + k == P0.lam_rec) { r.a = (uint32_t)lambda_fixed[t]; r.b = (uint32_t)(lambda_fixed[t] >> 32); }
                    break;
                case OP_IDIVC: r.dst = mv(r.dst); r.a = mv(r.a); break;          // c is an immediate
                case OP_MACK: r.dst = mv(r.dst); r.a = mv(r.a); r.b = mv(r.b); break;   // c is an offset between words of one circuit
                case OP_REVEAL: r.dst += ro; r.a = mv(r.a); break;               // dst is a decode slot
                case OP_MAX: {
                    // max_tree folds in the constant zero as the SECOND operand through a stride of -a
                    const bool to_zero = r.cnt == 2 && r.sa == -(int32_t)r.a;
                    r.dst = mv(r.dst); r.a = mv(r.a);
                    if (to_zero) r.sa = -(int32_t)r.a;
                } break;
                default: r.dst = mv(r.dst); r.a = mv(r.a); r.b = mv(r.b); r.c = mv(r.c); break;
                }
                if (sys_remap && (r.op == OP_ADD || r.op == OP_COPY) && r.a >= sys_remap->lo && r.a - sys_remap->lo < sys_remap->len)
                    r.a += sys_remap->off[t];
                P.emit(r);
            }
        }
        P.cap_steps = cap_keep;
        P.new_launch();
        while (next_iter < P0.iter_launch.size() && P0.iter_launch[next_iter] == li) {
            P.iter_launch.push_back((uint32_t)(P.launches.size() - 1));
            P.iter_gates.push_back(P.total_gates);
            next_iter++;
        }
    }
    return true;
}

// ---- K-fold cross-validation of the ridge lambda sweep (linreg_gc_ridge_cv.h).  Every share is K packed fold
// systems, as for the lasso's cross-validation (lower_fold_inputs).  Three parts under the one R:
//   prefix   F_k (share sums, on the data-provider path the off-diagonals and b divided by d), tot = sum_k F_k, tot - F_k and
//            the constant divisions by K - 1 (none for K = 2) and K: packed, free of lambda, garbled once, below shared_end
//   fits     (K + 1) L single-solve circuits merged by replicate_program, circuit t = s L + l: the packed training system s
//            (s = K: the full system) mirrored with q(lambda_l) on its diagonal, then the solver of spec.alg exactly as
//            build_program lowers it behind the two-party input path; beta_{s,l} stays at beta_at + t word_stride
//   tail     on gate steps behind the last circuit's: r = 2 b_k - F_k beta_{k,l} and score_{k,l} = 0 - <beta_{k,l}, r> as two
//            batches of plain OP_MAC products (also at w = 64: no half-difference shadow of F_k and of the K L fold models is
//            formed; DESIGN.md 2.7 has the gate cost), cv_l = sum_k score_{k,l}, the first signed minimum and the gated select
//            among the L refits, which alone is revealed -- with l* and the cv_l where select_reveal asks
// One value (L = 1): nothing is scored, only the full system is assembled and fitted; l* and cv_0 are the constant zero.
// Returns 0, or what does not fit: 1 the word ids, 2 the circuit count or a circuit's gate steps
inline int build_ridge_cv(Program &P, const Spec &spec, size_t K, size_t NL, const uint64_t *lam, uint64_t cap_steps) {
    const size_t d = spec.d, T = d * (d + 1) / 2, H = T + d;
    const bool scored = NL > 1;
    const size_t NS = scored ? K + 1 : 1, NC = NS * NL;
    Program P0;
    P0.cap_steps = cap_steps ? cap_steps : kSweepCapSteps;
    P0.merge_hint = NC;
    P0.w = spec.w; P0.p = spec.p; P0.d = d; P0.nshares = spec.nshares; P0.targets = 1; P0.T = T;
    P0.folds = K; P0.keep_beta = true;
    const size_t IN = P0.in_words();
    P0.in_base = P0.alloc(spec.nshares * IN);
    // the prefix.  dif and tot are neighbours: training system s lies s H words above the first one
    const uint32_t S = P0.alloc(IN), dif = scored ? P0.alloc(K * H) : 0, tot = P0.alloc(H);
    auto fold = [&](size_t k) { return packed_at(d, S + (uint32_t)(k * H)); };
    P0.new_launch();
    for (size_t k = 0; k < K; k++) sum_shares(P0, (uint32_t)(k * H), d, fold(k));
    P0.new_launch();
    if (spec.normalize) for (size_t k = 0; k < K; k++) divide_by_d(P0, fold(k), d);
    P0.new_launch();
    for (size_t e = 0; e < H; e++) P0.emit(Program::mk(OP_SUM, tot + (uint32_t)e, S + (uint32_t)e, 0, 0, (uint32_t)K, (int32_t)H));
    P0.new_launch();
    for (size_t e = 0; e < (scored ? K * H : 0); e++) P0.emit(Program::mk(OP_SUB, dif + (uint32_t)e, tot + (uint32_t)(e % H), S + (uint32_t)e));
    P0.new_launch();
    if (K > 2)
        for (size_t e = 0; e < (scored ? K * H : 0); e++) P0.emit(idivc_rec(dif + (uint32_t)e, dif + (uint32_t)e, (uint32_t)(K - 1), spec.w));
    for (size_t e = 0; e < H; e++) P0.emit(idivc_rec(tot + (uint32_t)e, tot + (uint32_t)e, (uint32_t)K, spec.w));
    close_prefix(P0, tot + (uint32_t)H);
    // one circuit: lambda, the mirror of the first training system, the solver
    const uint32_t src = scored ? dif : tot;
    Layout L = {d, 1, P0.alloc(d * d), P0.alloc(d)};
    L.Ms.push_back(L.M); L.bs.push_back(L.bv);
    const uint32_t lamw = P0.alloc(1);
    P0.lam_rec = (uint32_t)P0.recs.size();
    P0.emit(Program::mk(OP_CONST, lamw, (uint32_t)lam[0], (uint32_t)(lam[0] >> 32)));
    P0.new_launch();
    mirror(P0, d, L.M, src, DIAG_LAMBDA_LAUNCH, lamw);
    for (size_t i = 0; i < d; i++) P0.emit(Program::mk(OP_COPY, L.bv + (uint32_t)i, src + (uint32_t)(T + i)));
    P0.new_launch();
    switch (spec.alg) {
    case ALG_CGD: lower_cgd(P0, spec, L); break;
    case ALG_CHOLESKY: lower_cholesky(P0, L); break;
    default: lower_ldlt(P0, L); break;
    }
    P0.new_launch();
    if (P0.overflow || (uint64_t)P0.shared_end + (uint64_t)(P0.n_words - P0.shared_end) * NC >= Program::kMaxWords) return 1;
    if (NC + 1 > 65536) return 2;
    std::vector<uint64_t> lf(NC);
    std::vector<uint32_t> off(NC);
    for (size_t t = 0; t < NC; t++) { lf[t] = lam[t % NL]; off[t] = (uint32_t)((t / NL) * H); }
    const SysRemap remap = {src, (uint32_t)H, off.data()};
    if (!replicate_program(P, P0, NC, lf.data(), 0, &remap)) return 2;
    P.folds = K; P.path = NL; P.select_reveal = spec.select_reveal; P.ridge_cv = true; P.ridge_alg = spec.alg;
    P.cv_circuits = (uint32_t)NC; P.replicas = 1; P.reveal_stride = 0;
    P.words64 = P.n_words;
    P.merge_hint = 1;
    P.new_launch();
    P.step_cursor = P0.prefix_steps + (uint64_t)NC * kSweepCircuitStride;
    const uint32_t stride = P.word_stride;
    auto beta = [&](size_t s, size_t l) { return P0.beta_at + (uint32_t)(s * NL + l) * stride; };
    uint32_t best = beta(0, 0), cv = 0;
    LassoPick pick = {0, 0};
    if (scored) {
        const uint32_t Fv = P.alloc(K * d * d), b2v = P.alloc(K * d), rr = P.alloc(K * NL * d), score = P.alloc(K * NL);
        cv = P.alloc(NL);
        size_t mv_waves, kara_min;
        mv_shape(P, mv_waves, kara_min);
        const uint32_t sc_r = P.alloc_dots(K * NL * d * d, K * NL * d, mv_waves), sc_s = P.alloc_dots(K * NL * d, K * NL, kTargetWaves);
        for (size_t k = 0; k < K; k++) {
            mirror(P, d, Fv + (uint32_t)(k * d * d), fold(k).A, DIAG_COPY, 0);
            for (size_t i = 0; i < d; i++) P.emit(Program::mk(OP_ADD, b2v + (uint32_t)(k * d + i), fold(k).b + (uint32_t)i, fold(k).b + (uint32_t)i));
        }
        P.new_launch();
        std::vector<Program::DotJob> jobs;
        jobs.reserve(K * NL * d);
        for (size_t k = 0; k < K; k++)
            for (size_t l = 0; l < NL; l++)
                for (size_t i = 0; i < d; i++) {
                    Program::DotJob J = {rr + (uint32_t)((k * NL + l) * d + i), b2v + (uint32_t)(k * d + i), Fv + (uint32_t)(k * d * d + i * d), beta(k, l), (uint32_t)d, true, 0};
                    jobs.push_back(J);
                }
        P.dots(jobs, sc_r, mv_waves, kara_min);
        jobs.clear();
        for (size_t k = 0; k < K; k++)
            for (size_t l = 0; l < NL; l++) {
                Program::DotJob J = {score + (uint32_t)(k * NL + l), 0, beta(k, l), rr + (uint32_t)((k * NL + l) * d), (uint32_t)d, true, 0};
                jobs.push_back(J);
            }
        P.dots(jobs, sc_s, kTargetWaves);
        for (size_t l = 0; l < NL; l++) P.emit(Program::mk(OP_SUM, cv + (uint32_t)l, score + (uint32_t)l, 0, 0, (uint32_t)K, (int32_t)NL));
        P.new_launch();
        pick = select_argmin(P, NL, cv);
        best = P.alloc(d);
        for (size_t i = 0; i < d; i++) P.emit(Program::mk(OP_SUM, best + (uint32_t)i, beta(K, 0) + (uint32_t)i, pick.hot, 0, (uint32_t)NL, (int32_t)stride, 1));
        P.new_launch();
    }
    P.rv_beta = P.alloc_reveal(P.beta_words());
    uint32_t slot = P.rv_beta;
    for (size_t i = 0; i < d; i++) P.emit(Program::mk(OP_REVEAL, slot++, best + (uint32_t)i));
    if (spec.select_reveal & SELECT_REVEAL_INDEX) P.emit(Program::mk(OP_REVEAL, slot++, pick.index));
    if (spec.select_reveal & SELECT_REVEAL_SCORES)
        for (size_t l = 0; l < NL; l++) P.emit(Program::mk(OP_REVEAL, slot++, scored ? cv + (uint32_t)l : 0));
    P.new_launch();
    return P.overflow ? 1 : 0;
}

// Garbled-table ring (co-located solver): launch i owns the byte range [off[i], off[i] + len[i]) of a
// ring of `ring_bytes`, allocated in launch order with wrap-around; before the garbler overwrites the
// range it waits for the evaluation of wait[i], the newest earlier launch whose range overlaps (the
// evaluator runs in launch order, so every older overlapping launch is done by then too; -1: none).
// ring_bytes == 0 picks the largest launch plus room for what runs ahead of its evaluation: as much again, at most
// kRingSlackBytes (the large launches are the MAC launches, which alternate garble / evaluate anyway; what does run ahead
// are the small launches between them -- merges, inner products, dividers, reveals: tens of MB per iteration).  Returns the
// ring size.
inline size_t plan_table_ring(const Program &P, size_t ring_bytes, std::vector<size_t> &off, std::vector<int64_t> &wait) {
    const size_t align = 4096, nl = P.launches.size();
    const size_t tbytes = (size_t)P.max_launch_steps * 2048;
    const size_t min_ring = (tbytes + align - 1) / align * align;
    if (ring_bytes == 0) ring_bytes = min_ring + (min_ring < ring_slack_bytes() ? min_ring : ring_slack_bytes()) + align;
    if (ring_bytes < min_ring) ring_bytes = min_ring;
    off.resize(nl);
    wait.assign(nl, -1);
    std::vector<size_t> len(nl);
    size_t head = 0;
    for (size_t i = 0; i < nl; i++) {
        len[i] = ((size_t)P.launches[i].steps * 2048 + align - 1) / align * align;
        if (head + len[i] > ring_bytes) head = 0;
        off[i] = head;
        head += len[i];
    }
    for (size_t i = 0; i < nl; i++) {
        // scanning back may stop once more than a full ring of newer ranges has been passed: anything
        // older was overwritten by launches that waited for evaluations newer than it
        size_t seen = 0;
        for (size_t j = i; j-- > 0 && seen <= ring_bytes;) {
            seen += len[j];
            if (len[i] && len[j] && off[j] < off[i] + len[i] && off[i] < off[j] + len[j]) {
                wait[i] = (int64_t)j;
                break;
            }
        }
        // the garbler chain is in order: what an earlier launch waited for holds for this one too
        if (i > 0 && wait[i - 1] > wait[i]) wait[i] = wait[i - 1];
    }
    return ring_bytes;
}
}  // namespace gc
