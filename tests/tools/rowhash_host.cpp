// rowhash_host.cpp -- gc_aes.h's row_hash and lane-uniform hash against hash_n on the host (tests/test_rowhash_cpu.py).
//
// A sequence is one label hashed at the tweaks of the 32 partial-product rows of a multiplier array that starts at gate
// step s0: row 0 at step s0, row i at step s0 + 2 i - 1 (tweak 128 step + 2 lane + h), i.e. one stride of 128 and then
// strides of 256.  row_hash runs the rows in order with one cache per lane; the lane-uniform form runs every row on 32
// emulated lanes (hash_lu_emul: a host copy of the device form's lane algebra -- the device code itself is tied to hash_n by
// the GPU tests).  Every hash must equal hash_n<1, HostTab>.  Prints one line per sequence; exit status 1 on a mismatch.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "gc_aes.h"

using namespace gc;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd32() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
static bool same(Lbl a, Lbl b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

int main(int argc, char **argv) {
    static const AesTables T = aes_make_tables(kFixedKey);
    HostTab tab;
    tab.te0 = T.te0;
    // the cases: "s0 description" per line (tests/golden/rowhash_starts.txt, shared with the GPU test)
    struct Seq { char what[64]; uint64_t s0; };
    std::vector<Seq> seqs;
    FILE *f = argc > 1 ? fopen(argv[1], "r") : 0;
    if (!f) { printf("usage: rowhash_host <file of array starts>\n"); return 2; }
    char line[256];
    while (fgets(line, sizeof line, f)) {
        Seq q;
        unsigned long long s0;
        if (line[0] == '#' || sscanf(line, "%llu %63[^\n]", &s0, q.what) != 2) continue;
        q.s0 = s0;
        seqs.push_back(q);
    }
    fclose(f);
    if (seqs.size() < 8) { printf("too few cases\n"); return 2; }
    int bad = 0;
    size_t total = 0;
    for (const Seq &q : seqs) {
        for (int h = 0; h < 2; h++) {
            const Lbl x = {rnd32(), rnd32(), rnd32(), rnd32()};
            const Lbl x2 = {rnd32(), rnd32(), rnd32(), rnd32()};
            RowCache<2> rc[32];
            int fills = 0, miss_row = 0, miss_lu = 0;
            uint64_t last_fill = 0;
            for (int r = 0; r < 32; r++) {
                const uint64_t step = q.s0 + (r ? 2 * r - 1 : 0), twu = 128 * step + (uint64_t)h;
                uint64_t tw[32];
                Lbl ref[32], ref2[32], lu[32];
                for (int l = 0; l < 32; l++) {
                    tw[l] = twu + 2 * (uint64_t)l;
                    hash_n<1, HostTab>(tab, T.rk, &x, &tw[l], &ref[l]);
                    hash_n<1, HostTab>(tab, T.rk, &x2, &tw[l], &ref2[l]);
                }
                // row_hash, two labels at once as the garbler runs it, one cache per lane
                for (int l = 0; l < 32; l++) {
                    const Lbl in[2] = {x, x2};
                    Lbl out[2];
                    row_hash<2, HostTab>(tab, T.rk, in, tw[l], twu, r == 0, rc[l], out);
                    if (!same(out[0], ref[l]) || !same(out[1], ref2[l])) miss_row++;
                }
                if (r == 0 || rc[0].tw != last_fill) { fills++; last_fill = rc[0].tw; }
                hash_lu_emul<HostTab>(tab, T.rk, x, tw, lu);
                for (int l = 0; l < 32; l++)
                    if (!same(lu[l], ref[l])) miss_lu++;
                total += 3 * 32;
            }
            printf("%-18s h=%d s0=%llu: fills %d, row_hash mismatches %d, lane-uniform mismatches %d\n", q.what, h,
                   (unsigned long long)q.s0, fills, miss_row, miss_lu);
            bad += miss_row + miss_lu;
            // a sequence that crosses nothing refills once (row 1: the step's parity); one crossing adds one fill
            if (fills < 2 || fills > 3) { printf("  unexpected number of fills\n"); bad++; }
        }
    }
    // a cache that is NOT refilled where it must be gives a wrong hash: the rule is needed, not just sufficient
    {
        const Lbl x = {rnd32(), rnd32(), rnd32(), rnd32()};
        RowCache<1> rc;
        Lbl out, ref;
        uint64_t t0 = 128ull * 511, t1 = 128ull * 513;
        row_hash<1, HostTab>(tab, T.rk, &x, t0, t0, true, rc, &out);
        rc.tw = t1;                                   // pretend the fill was made at t1
        row_hash<1, HostTab>(tab, T.rk, &x, t1, t1, false, rc, &out);
        hash_n<1, HostTab>(tab, T.rk, &x, &t1, &ref);
        if (same(out, ref)) { printf("stale cache went unnoticed\n"); bad++; }
    }
    printf("%s: %zu hashes compared\n", bad ? "FAIL" : "ok", total);
    return bad ? 1 : 0;
}
