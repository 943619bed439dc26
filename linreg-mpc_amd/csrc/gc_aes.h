// gc_aes.h -- fixed-key AES-128 and the garbling hash, host + device.
//
// CDNA4 has no AES instruction: the device path is a T-table AES with the tables staged in LDS
// (layouts in gc_device.h).  A ds_read_b32 is serviced in two groups of 32 lanes over 32 banks
// (MI355X_MICROARCH.md, LDS), so 32 replicas of an entry -- lane l reads replica l mod 32 -- are
// conflict-free whatever the data, and the LDS byte address (entry << 8 | table bits | replica << 2)
// is formed by ONE v_perm_b32 from the state word and a per-lane constant.  The MAC kernels and the
// one-workgroup-per-CU generic kernels keep all four rotated tables Te_t = rotl(Te0, 8t) resident
// (128 KiB): a round is 16 lookups + 8 three-input XORs (v_bitop3_b32), no rotates -- 240 VALU + 160
// ds_read_b32 per block.  Kernels that need two workgroups per CU use Te0 | Te2 in 64 KiB (one
// rotate per column); the single-table image (three v_alignbit per column) remains for the small
// input-label and PRG kernels.  Integer VALU issue is 16 lanes/clk/SIMD on CDNA4, so instruction
// count per block bounds the cipher until the LDS roof (160 lookups x 2 clk per wave) takes over.
//
// Conventions: a 128-bit block / label is 4 little-endian u32 words; word c
// is AES state column c, byte r of the word is state row r -- the byte order
// of FIPS-197 and of x86 AES-NI, so CPU (AES-NI) and GPU agree bit for bit.
//
// Hash (half-gates, Zahur-Rosulek-Evans 2015, fixed-key model):
//     H(x, t) = AES_k(sigma(x) ^ t) ^ sigma(x) ^ t,
//     sigma(xL || xR) = (xL ^ xR) || xL   (a linear orthomorphism)
// This replaces Obliv-C's libgcrypt-based gate hash (reference call site:
// execYaoProtocol, src/cmd/linreg.c:177).
#pragma once
#include <stdint.h>

#ifndef GC_HD
#if defined(__HIPCC__)
#define GC_HD __host__ __device__ __forceinline__
#else
#define GC_HD inline
#endif
#endif

namespace gc {

struct Lbl {
    uint32_t x, y, z, w;
};
GC_HD Lbl lxor(Lbl a, Lbl b) { Lbl r = {a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w}; return r; }
GC_HD Lbl lzero() { Lbl r = {0, 0, 0, 0}; return r; }
// m ? a : 0 without a branch
GC_HD Lbl lmask(Lbl a, uint32_t m) { uint32_t k = 0u - (m & 1u); Lbl r = {a.x & k, a.y & k, a.z & k, a.w & k}; return r; }

// ---------------------------------------------------------------- host tables
struct AesTables {
    uint8_t sbox[256];
    uint32_t te0[256];
    uint32_t rk[44];
};

constexpr uint8_t aes_xtime(uint8_t v) { return (uint8_t)((v << 1) ^ ((v >> 7) * 0x1b)); }

// S-box from first principles (multiplicative inverse in GF(2^8) + affine map).  constexpr: the device constants of the
// fixed-key hash are COMPILE-TIME data (gc_device.h c_aes) -- nothing is uploaded when a process starts, and a code
// object is loaded when its first kernel is launched, not because its constants had to be written.
constexpr AesTables aes_make_tables(const uint8_t *key) {
    AesTables t{};
    uint8_t pw[256] = {}, lg[256] = {};
    uint8_t g = 1;
    for (int i = 0; i < 255; i++) { pw[i] = g; lg[g] = (uint8_t)i; g = (uint8_t)(g ^ aes_xtime(g)); }  // generator 3
    for (int x = 0; x < 256; x++) {
        uint8_t inv = x ? pw[(255 - lg[x]) % 255] : 0;
        uint8_t s = inv, r = inv;
        for (int k = 0; k < 4; k++) { r = (uint8_t)((r << 1) | (r >> 7)); s ^= r; }
        t.sbox[x] = (uint8_t)(s ^ 0x63);
    }
    for (int x = 0; x < 256; x++) {
        uint8_t s = t.sbox[x], s2 = aes_xtime(s), s3 = (uint8_t)(s2 ^ s);
        t.te0[x] = (uint32_t)s2 | ((uint32_t)s << 8) | ((uint32_t)s << 16) | ((uint32_t)s3 << 24);
    }
    for (int i = 0; i < 4; i++)
        t.rk[i] = (uint32_t)key[4 * i] | ((uint32_t)key[4 * i + 1] << 8) | ((uint32_t)key[4 * i + 2] << 16) |
                  ((uint32_t)key[4 * i + 3] << 24);
    uint8_t rcon = 1;
    for (int i = 4; i < 44; i++) {
        uint32_t v = t.rk[i - 1];
        if (i % 4 == 0) {
            v = (v >> 8) | (v << 24);  // RotWord (bytes are little-endian in the word)
            v = (uint32_t)t.sbox[v & 0xff] | ((uint32_t)t.sbox[(v >> 8) & 0xff] << 8) |
                ((uint32_t)t.sbox[(v >> 16) & 0xff] << 16) | ((uint32_t)t.sbox[(v >> 24) & 0xff] << 24);
            v ^= rcon;
            rcon = aes_xtime(rcon);
        }
        t.rk[i] = t.rk[i - 4] ^ v;
    }
    return t;
}
inline void aes_build_tables(AesTables &t, const uint8_t key[16]) { t = aes_make_tables(key); }

// the fixed public key of this build (FIPS-197 Appendix B example key)
static constexpr uint8_t kFixedKey[16] = {0x2b, 0x7e, 0x15, 0x16, 0x28, 0xae, 0xd2, 0xa6,
                                          0xab, 0xf7, 0x15, 0x88, 0x09, 0xcf, 0x4f, 0x3c};

// what the device kernels read: round keys, Te0, and rotl24 of the round keys (two-table AES rounds)
struct DevAesConst {
    uint32_t rk[44];
    uint32_t te0[256];
    uint32_t rk24[44];
};
constexpr DevAesConst aes_make_dev_const() {
    AesTables t = aes_make_tables(kFixedKey);
    DevAesConst c{};
    for (int i = 0; i < 44; i++) { c.rk[i] = t.rk[i]; c.rk24[i] = (t.rk[i] << 24) | (t.rk[i] >> 8); }
    for (int i = 0; i < 256; i++) c.te0[i] = t.te0[i];
    return c;
}

GC_HD uint32_t rotl32(uint32_t v, int k) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(v, v, 32 - k);
#else
    return (v << k) | (v >> (32 - k));
#endif
}
// three-input XOR: one v_bitop3_b32 on gfx950 (there is no v_xor3 on gfx9)
GC_HD uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}
// last round: Te0[x] = (2s, s, s, 3s) holds S[x] in bytes 1 and 2; build the
// output column from four lookups with two byte permutes
GC_HD uint32_t last_lo(uint32_t v1, uint32_t v0) {   // byte0 <- S[i0], byte1 <- S[i1]
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(v1, v0, 0x0c0c0501);
#else
    return ((v0 >> 8) & 0xffu) | (v1 & 0xff00u);
#endif
}
GC_HD uint32_t last_hi(uint32_t v3, uint32_t v2) {   // byte2 <- S[i2], byte3 <- S[i3]
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(v3, v2, 0x05020c0c);
#else
    return (v2 & 0xff0000u) | ((v3 << 16) & 0xff000000u);
#endif
}

// N independent blocks, interleaved round by round (ILP hides LDS latency).
// T: table accessor, T::lk(word, k) returns Te0[byte k of word].
// Rounds FIRST .. 10 of the cipher on states that have been through rounds 0 .. FIRST - 1 (row_hash and hash_lu below
// enter at round 3).
template <int N, class T, int FIRST>
GC_HD void aes_rounds_n(const T &tab, const uint32_t *rk, uint32_t s[N][4], const uint32_t *rk24 = 0) {
#pragma unroll
    for (int rnd = FIRST; rnd < 10; rnd++) {
        uint32_t v[N][16];
#pragma unroll
        for (int b = 0; b < N; b++) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (T::kFourTables) {
                    v[b][4 * j + 0] = tab.lkt(0, s[b][j], 0);
                    v[b][4 * j + 1] = tab.lkt(1, s[b][(j + 1) & 3], 1);
                    v[b][4 * j + 2] = tab.lkt(2, s[b][(j + 2) & 3], 2);
                    v[b][4 * j + 3] = tab.lkt(3, s[b][(j + 3) & 3], 3);
                    continue;
                }
                v[b][4 * j + 0] = tab.lk(s[b][j], 0);
                v[b][4 * j + 1] = tab.lk(s[b][(j + 1) & 3], 1);
                v[b][4 * j + 2] = T::kTwoTables ? tab.lk2(s[b][(j + 2) & 3], 2) : tab.lk(s[b][(j + 2) & 3], 2);
                v[b][4 * j + 3] = T::kTwoTables ? tab.lk2(s[b][(j + 3) & 3], 3) : tab.lk(s[b][(j + 3) & 3], 3);
            }
        }
#pragma unroll
        for (int b = 0; b < N; b++) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (T::kFourTables) {
                    // Te_t = rotl(Te0, 8t) are all resident: no rotates
                    s[b][j] = xor3(xor3(v[b][4 * j], v[b][4 * j + 1], rk[4 * rnd + j]), v[b][4 * j + 2], v[b][4 * j + 3]);
                } else if (T::kTwoTables) {
                    // v2, v3 come from Te2 = rotl16(Te0): col = Te0[i0]^Te2[i2] ^ rotl8(Te0[i1]^Te2[i3]) ^ rk,
                    // with the round key folded in before the rotation (rk24 = rotl24(rk))
                    uint32_t x = xor3(v[b][4 * j + 1], v[b][4 * j + 3], rk24[4 * rnd + j]);
                    s[b][j] = xor3(v[b][4 * j], v[b][4 * j + 2], rotl32(x, 8));
                } else {
                    uint32_t t = xor3(v[b][4 * j], rotl32(v[b][4 * j + 2], 16), rk[4 * rnd + j]);
                    s[b][j] = xor3(t, rotl32(v[b][4 * j + 1], 8), rotl32(v[b][4 * j + 3], 24));
                }
            }
        }
    }
    {
        uint32_t v[N][16];
#pragma unroll
        for (int b = 0; b < N; b++) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                v[b][4 * j + 0] = tab.lk(s[b][j], 0);
                v[b][4 * j + 1] = tab.lk(s[b][(j + 1) & 3], 1);
                v[b][4 * j + 2] = tab.lk(s[b][(j + 2) & 3], 2);
                v[b][4 * j + 3] = tab.lk(s[b][(j + 3) & 3], 3);
            }
        }
#pragma unroll
        for (int b = 0; b < N; b++) {
#pragma unroll
            for (int j = 0; j < 4; j++)
                s[b][j] = xor3(last_lo(v[b][4 * j + 1], v[b][4 * j]), last_hi(v[b][4 * j + 3], v[b][4 * j + 2]), rk[40 + j]);
        }
    }
}
template <int N, class T>
GC_HD void aes_encrypt_n(const T &tab, const uint32_t *rk, uint32_t s[N][4], const uint32_t *rk24 = 0) {
#pragma unroll
    for (int b = 0; b < N; b++) {
        s[b][0] ^= rk[0]; s[b][1] ^= rk[1]; s[b][2] ^= rk[2]; s[b][3] ^= rk[3];
    }
    aes_rounds_n<N, T, 1>(tab, rk, s, rk24);
}

// K = sigma(x) ^ tweak, as 4 words
GC_HD void hash_prep(Lbl x, uint64_t tweak, uint32_t k[4]) {
    k[0] = x.z ^ (uint32_t)tweak;
    k[1] = x.w ^ (uint32_t)(tweak >> 32);
    k[2] = x.z ^ x.x;
    k[3] = x.w ^ x.y;
}

// N hashes at once: out[b] = AES(K_b) ^ K_b
template <int N, class T>
GC_HD void hash_n(const T &tab, const uint32_t *rk, const Lbl *x, const uint64_t *tw, Lbl *out, const uint32_t *rk24 = 0) {
    uint32_t s[N][4], k[N][4];
#pragma unroll
    for (int b = 0; b < N; b++) {
        hash_prep(x[b], tw[b], k[b]);
        s[b][0] = k[b][0]; s[b][1] = k[b][1]; s[b][2] = k[b][2]; s[b][3] = k[b][3];
    }
    aes_encrypt_n<N, T>(tab, rk, s, rk24);
#pragma unroll
    for (int b = 0; b < N; b++) {
        out[b].x = s[b][0] ^ k[b][0]; out[b].y = s[b][1] ^ k[b][1];
        out[b].z = s[b][2] ^ k[b][2]; out[b].w = s[b][3] ^ k[b][3];
    }
}

// host table accessor (plain array)
struct HostTab {
    static const bool kTwoTables = false;
    static const bool kFourTables = false;
    const uint32_t *te0;
    inline uint32_t lkt(int, uint32_t word, int k) const { return lk(word, k); }
    inline uint32_t lk(uint32_t word, int k) const { return te0[(word >> (8 * k)) & 0xffu]; }
    inline uint32_t lk2(uint32_t word, int k) const { return rotl32(lk(word, k), 16); }
};

// ---- hashes that share lookups across the rows of a multiplier array and across the lanes of a half wave.
// The tweak of gate step `step`, lane l, hash h is t = 128 step + 2 l + h, and it enters AES column 0 only (column 1
// from step 2^25 on).  Round r's output column j reads s[j].b0, s[j+1].b1, s[j+2].b2, s[j+3].b3, so a difference in ONE
// byte of column 0 reaches one column after round 1 and one lookup per column in round 2: 15 + 12 of the first 32
// lookups do not see it.  Both forms below return exactly hash_n's value.

// Te_t[byte k of word], Te_t = rotl(Te0, 8 t), from whatever tables T keeps
template <class T>
GC_HD uint32_t te_lk(const T &tab, int t, uint32_t word, int k) {
    if (T::kFourTables) return tab.lkt(t, word, k);
    const uint32_t v = tab.lk(word, k);
    return t ? rotl32(v, 8 * t) : v;
}

// row_hash: the same label hashed at tweaks that differ in byte 1 of the low word only -- operand `a` of the partial
// products of Circ::umul32x2, whose rows are two gate steps apart.  Byte 1 of column 0 is read by column 3 of round 1,
// and column 3 by one lookup per column of round 2: the other 27 lookups fold into five words per hash (RowFix), and a
// row costs 1 + 4 + 128 lookups.  The cache is refilled when the tweak leaves the byte (a wave-uniform branch: `twu`
// is the tweak without its lane bits) or the caller says the label is new.
struct RowFix {
    uint32_t c3;      // round 1, column 3: round key ^ the three lookups that do not read s[0].b1
    uint32_t p[4];    // round 2, column j: round key ^ the three lookups that do not read column 3
};
template <int N>
struct RowCache {
    RowFix f[N];
    uint64_t tw;      // twu of the fill
};
template <int N, class T>
GC_HD void row_fill(const T &tab, const uint32_t *rk, const Lbl *x, uint64_t tw, RowFix *f) {
#pragma unroll
    for (int b = 0; b < N; b++) {
        uint32_t s[4], s1[3];
        hash_prep(x[b], tw, s);
        s[0] ^= rk[0]; s[1] ^= rk[1]; s[2] ^= rk[2]; s[3] ^= rk[3];
#pragma unroll
        for (int j = 0; j < 3; j++)
            s1[j] = xor3(xor3(te_lk(tab, 0, s[j], 0), te_lk(tab, 1, s[j + 1], 1), rk[4 + j]), te_lk(tab, 2, s[(j + 2) & 3], 2),
                         te_lk(tab, 3, s[(j + 3) & 3], 3));
        f[b].c3 = xor3(te_lk(tab, 0, s[3], 0), te_lk(tab, 2, s[1], 2), rk[7]) ^ te_lk(tab, 3, s[2], 3);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint32_t acc = rk[8 + j];
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (((j + k) & 3) != 3) acc ^= te_lk(tab, k, s1[(j + k) & 3], k);
            f[b].p[j] = acc;
        }
    }
}
// tw: the (per-lane) tweak, the same for the N labels; fresh: the labels are not the ones of the last call
template <int N, class T>
GC_HD void row_hash(const T &tab, const uint32_t *rk, const Lbl *x, uint64_t tw, uint64_t twu, bool fresh, RowCache<N> &rc,
                    Lbl *out, const uint32_t *rk24 = 0) {
    if (fresh || ((twu ^ rc.tw) & ~0xff00ull) != 0) {
        row_fill<N, T>(tab, rk, x, tw, rc.f);
        rc.tw = twu;
    }
    uint32_t s[N][4], k[N][4], c3[N];
#pragma unroll
    for (int b = 0; b < N; b++) {
        hash_prep(x[b], tw, k[b]);
        c3[b] = rc.f[b].c3 ^ te_lk(tab, 1, k[b][0] ^ rk[0], 1);
    }
#pragma unroll
    for (int b = 0; b < N; b++) {
#pragma unroll
        for (int j = 0; j < 4; j++) s[b][j] = rc.f[b].p[j] ^ te_lk(tab, 3 - j, c3[b], 3 - j);
    }
    aes_rounds_n<N, T, 3>(tab, rk, s, rk24);
#pragma unroll
    for (int b = 0; b < N; b++) {
        out[b].x = s[b][0] ^ k[b][0]; out[b].y = s[b][1] ^ k[b][1];
        out[b].z = s[b][2] ^ k[b][2]; out[b].w = s[b][3] ^ k[b][3];
    }
}

// hash_lu: ONE label in the 32 lanes of a half wave (operand `b` of a partial-product row, Backend::bcast2), tweaks
// that differ in the lane bits only -- byte 0 of column 0.  That byte is read by column 0 of round 1, and column 0 by
// one lookup per column of round 2; the other 15 + 12 lookups are the same in all 32 lanes.  Lane 4 j + i of a half
// fetches the term of output column j that comes from table i -- byte i of state column lu_col = (j + i) & 3 -- in ONE
// lookup per round (lanes 16 .. 31 repeat lanes 0 .. 15); a lane whose term is lane-dependent contributes zero
// (lu_skip); an XOR over each quad gives the shared part of column j, which every lane then reads from lane 4 j of its
// half.  2 + 5 + 128 lookup instructions per hash.
GC_HD uint32_t lu_col(uint32_t lane) { return ((lane >> 2) + lane) & 3u; }
GC_HD bool lu_skip(uint32_t lane, int rnd) { return rnd == 1 ? (lane & 15u) == 0u : lu_col(lane) == 0u; }

#if defined(__HIPCC__)
__device__ __forceinline__ uint32_t lu_quad_xor(uint32_t v) {
    v ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xb1, 0xf, 0xf, true);    // quad_perm [1, 0, 3, 2]
    v ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4e, 0xf, 0xf, true);    // quad_perm [2, 3, 0, 1]
    return v;
}
// lane `src` of the caller's half wave; hm: all ones in lanes 32 .. 63
__device__ __forceinline__ uint32_t lu_half_bcast(uint32_t v, int src, uint32_t hm) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)v, src), hi = (uint32_t)__builtin_amdgcn_readlane((int)v, 32 + src);
    return lo ^ ((lo ^ hi) & hm);
}
// All 64 lanes must be active.  T::lkl(word): Te_i[byte i of word] with i = lane & 3 (gc_device.h LdsTab4).
template <int N, class T>
__device__ __forceinline__ void hash_lu(const T &tab, const uint32_t *rk, const Lbl *x, uint64_t tw, uint32_t lane, Lbl *out,
                                        const uint32_t *rk24 = 0) {
    const uint32_t col = lu_col(lane), hm = 0u - (lane >> 5);
    const bool skip1 = lu_skip(lane, 1), skip2 = lu_skip(lane, 2);
    uint32_t s[N][4], k[N][4];
#pragma unroll
    for (int rnd = 1; rnd <= 2; rnd++) {
        uint32_t d[N][4], u[N];
#pragma unroll
        for (int b = 0; b < N; b++) {
            if (rnd == 1) {
                hash_prep(x[b], tw, k[b]);
                s[b][0] = k[b][0] ^ rk[0]; s[b][1] = k[b][1] ^ rk[1]; s[b][2] = k[b][2] ^ rk[2]; s[b][3] = k[b][3] ^ rk[3];
                d[b][0] = te_lk(tab, 0, s[b][0], 0);
                d[b][1] = d[b][2] = d[b][3] = 0u;
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) d[b][j] = te_lk(tab, (4 - j) & 3, s[b][0], (4 - j) & 3);
            }
            const uint32_t w = col == 0 ? s[b][0] : (col == 1 ? s[b][1] : (col == 2 ? s[b][2] : s[b][3]));
            u[b] = tab.lkl(w);
        }
#pragma unroll
        for (int b = 0; b < N; b++) {
            u[b] = lu_quad_xor((rnd == 1 ? skip1 : skip2) ? 0u : u[b]);
#pragma unroll
            for (int j = 0; j < 4; j++) s[b][j] = xor3(d[b][j], lu_half_bcast(u[b], 4 * j, hm), rk[4 * rnd + j]);
        }
    }
    aes_rounds_n<N, T, 3>(tab, rk, s, rk24);
#pragma unroll
    for (int b = 0; b < N; b++) {
        out[b].x = s[b][0] ^ k[b][0]; out[b].y = s[b][1] ^ k[b][1];
        out[b].z = s[b][2] ^ k[b][2]; out[b].w = s[b][3] ^ k[b][3];
    }
}
#endif
// The same on the host, the 32 lanes of a half wave as arrays: tw[l] is lane l's tweak.  A second writing of hash_lu's
// lane algebra (lu_col, lu_skip and the rounds are shared, the cross-lane moves are not): comparing it with hash_n
// proves which lookups may be shared and by which lanes, not the device code -- that is compared with hash_n on the
// device (lgc_row_hash_eval) and, inside the MAC kernel, through the garbled tables (tests/test_rowhash_gpu.py).  Every lane takes the shared
// part from the lanes that fetched it, as on the device -- tweaks that differ outside the lane bits give wrong hashes.
template <class T>
inline void hash_lu_emul(const T &tab, const uint32_t *rk, Lbl x, const uint64_t *tw, Lbl *out) {
    uint32_t s[32][4], k[32][4];
    for (int rnd = 1; rnd <= 2; rnd++) {
        uint32_t d[32][4], u[32];
        for (uint32_t l = 0; l < 32; l++) {
            if (rnd == 1) {
                hash_prep(x, tw[l], k[l]);
                for (int j = 0; j < 4; j++) { s[l][j] = k[l][j] ^ rk[j]; d[l][j] = 0u; }
                d[l][0] = te_lk(tab, 0, s[l][0], 0);
            } else {
                for (int j = 0; j < 4; j++) d[l][j] = te_lk(tab, (4 - j) & 3, s[l][0], (4 - j) & 3);
            }
            const int i = (int)(l & 3u);
            u[l] = lu_skip(l, rnd) ? 0u : te_lk(tab, i, s[l][lu_col(l)], i);
        }
        for (uint32_t q = 0; q < 32; q += 4) {
            const uint32_t v = u[q] ^ u[q + 1] ^ u[q + 2] ^ u[q + 3];
            u[q] = u[q + 1] = u[q + 2] = u[q + 3] = v;
        }
        for (uint32_t l = 0; l < 32; l++)
            for (int j = 0; j < 4; j++) s[l][j] = d[l][j] ^ u[4 * j] ^ rk[4 * rnd + j];
    }
    for (uint32_t l = 0; l < 32; l++) {
        uint32_t t[1][4] = {{s[l][0], s[l][1], s[l][2], s[l][3]}};
        aes_rounds_n<1, T, 3>(tab, rk, t);
        out[l].x = t[0][0] ^ k[l][0]; out[l].y = t[0][1] ^ k[l][1];
        out[l].z = t[0][2] ^ k[l][2]; out[l].w = t[0][3] ^ k[l][3];
    }
}

// the half-gates equations on the hashes h = H(a0), H(a0 ^ R), H(b0), H(b0 ^ R) (garbler) / H(a), H(b) (evaluator)
GC_HD Lbl garble_mix(Lbl R, Lbl a0, Lbl b0, const Lbl *h, Lbl &TG, Lbl &TE) {
    uint32_t pa = a0.x & 1u, pb = b0.x & 1u;
    TG = lxor(lxor(h[0], h[1]), lmask(R, pb));
    Lbl WG = lxor(h[0], lmask(TG, pa));
    TE = lxor(lxor(h[2], h[3]), a0);
    Lbl WE = lxor(h[2], lmask(lxor(TE, a0), pb));
    return lxor(WG, WE);
}
GC_HD Lbl eval_mix(Lbl a, Lbl b, const Lbl *h, Lbl TG, Lbl TE) {
    uint32_t sa = a.x & 1u, sb = b.x & 1u;
    Lbl WG = lxor(h[0], lmask(TG, sa));
    Lbl WE = lxor(h[1], lmask(lxor(TE, a), sb));
    return lxor(WG, WE);
}
// ---- half-gates, one AND gate (lane-local).  gid: unique gate id.
// Garbler: a0, b0 zero-labels; returns c0 and the two ciphertexts.
template <class T>
GC_HD Lbl garble_and(const T &tab, const uint32_t *rk, Lbl R, Lbl a0, Lbl b0, uint64_t gid, Lbl &TG, Lbl &TE,
                     const uint32_t *rk24 = 0) {
    Lbl in[4] = {a0, lxor(a0, R), b0, lxor(b0, R)};
    uint64_t tw[4] = {2 * gid, 2 * gid, 2 * gid + 1, 2 * gid + 1};
    Lbl h[4];
    // two pairs of interleaved blocks (four at once need more live registers than four waves per SIMD leave)
    hash_n<2, T>(tab, rk, in, tw, h, rk24);
    hash_n<2, T>(tab, rk, in + 2, tw + 2, h + 2, rk24);
    return garble_mix(R, a0, b0, h, TG, TE);
}
// Evaluator: a, b active labels.
template <class T>
GC_HD Lbl eval_and(const T &tab, const uint32_t *rk, Lbl a, Lbl b, uint64_t gid, Lbl TG, Lbl TE, const uint32_t *rk24 = 0) {
    Lbl in[2] = {a, b};
    uint64_t tw[2] = {2 * gid, 2 * gid + 1};
    Lbl h[2];
    hash_n<2, T>(tab, rk, in, tw, h, rk24);
    return eval_mix(a, b, h, TG, TE);
}

}  // namespace gc
