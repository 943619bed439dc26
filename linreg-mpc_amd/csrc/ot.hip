// ot.hip -- IKNP OT extension (semi-honest) on the MI355X.
//
// Replaces Obliv-C's honestOTExt* / honestCorrelatedOTExt* as called by the reference at
//   src/phase1.c:58-65, 84-89   Gilboa inner products over correlated OT (one OT per bit of a_k)
//   src/input.c:44, 108         1-of-2 OT of wire labels (data provider <- CSP)
// The kappa = 128 base OTs (Naor-Pinkas in Obliv-C, dhRandomInit) are public-key work on the
// host and not part of this path: the entry points take their outputs (seeds).
//
// Protocol (Ishai-Kilian-Nissim-Petrank 2003, with the correlated-OT optimisation of
// Asharov-Lindell-Schneider-Zohner 2013), m OTs, choice vector c:
//   receiver: t_j = G(k_j^0), u_j = t_j ^ G(k_j^1) ^ c            j = 0..127   (sends u: 16 B / OT)
//   sender  : q_j = G(k_j^{D_j}) ^ D_j * u_j       => row i: q_i = t_i ^ c_i * D
//   G       : AES-128-CTR keyed by the seed (per-column key schedule)
//   rows    : 128 x m bit-matrix transpose (wave ballots)
//   hash    : H(i, x) = the fixed-key hash of gc_aes.h with tweak i (unique per session)
//   correlated (Gilboa, payload w bits): x0_i = H(i, q_i), y_i = x0_i + delta_i - H(i, q_i ^ D);
//             receiver gets H(i, t_i) + c_i * y_i.  delta_i = 2^bit * b_k  (phase1.c:43-51)
//   matrix  : (include/linreg_gc_ot_matrix.h) one OT per bit of the receiver's word carries s words: pads H(i * nblk + c, .),
//             y_ij = x0_ij + 2^bit * Xs[k][j] - x1_ij; the extension is per OT, so it shrinks by the factor s
//   half    : (include/linreg_gc_ot_half.h) the matrix OTs and pads; bit `bit` runs mod 2^(W - bit) and is shifted afterwards, so
//             y carries W - bit bits per word: y'_ij = (x0_ij + Xs[k][j] - x1_ij) mod 2^(W - bit), W / 2 + 1 words per (k, ir, j)
//   labels  : e0_i = m0_i ^ H(i, q_i), e1_i = m1_i ^ H(i, q_i ^ D); receiver m_c = e_c ^ H(i, t_i)
#include <hip/hip_runtime.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "../../include/linreg_gc.h"
#include "../../include/linreg_gc_sweep.h"
#include "../../include/linreg_gc_debug.h"
#include "../../include/linreg_gc_ot_matrix.h"
#include "../../include/linreg_gc_ot_half.h"
#include "hip_scope.h"
#include "gc_device.h"

using namespace gc;

int lgc_fail(int code, const char *fmt, ...);
int lgc_need_device(int device);
hipError_t lgc_stream_take(int device, hipStream_t *out);      // gc_engine.hip: pooled streams (hipStreamCreate is ~10 ms)
void lgc_stream_give(int device, hipStream_t st);
__global__ void ot_tu_touch_kernel() {}
hipError_t ot_tu_touch(hipStream_t st) { hipLaunchKernelGGL(ot_tu_touch_kernel, dim3(1), dim3(64), 0, st); return hipGetLastError(); }

#define OTCHK(x)                                                                             \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess) return lgc_fail(LGC_EHIP, "%s: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// ---- column PRG.  grid.y = column j (0..127); each lane produces AES_kj(ctr0 + b) for block b.
// MODE 0 (receiver): T0[j][b] = G(k0), U[j][b] = G(k0) ^ G(k1) ^ c[b]
// MODE 1 (sender)  : Q[j][b]  = G(k)  ^ (delta_j ? U[j][b] : 0)
// Four-table AES image (128 KiB, one workgroup per CU) with the column's own key schedule in LDS.
template <int MODE>
__global__ void __launch_bounds__(1024)
ot_cols_kernel(const uint32_t *rk0, const uint32_t *rk1, uint64_t ctr0, uint32_t m128, const uint4 *cbits,
               const uint4 *Uin, uint4 delta, uint4 *out0, uint4 *out1) {
    __shared__ uint32_t lds_te0[2 * kLdsTabWords];
    __shared__ uint32_t sk0[44], sk1[44];
    lds_tab4_fill(lds_te0);
    const uint32_t j = blockIdx.y;
    if (threadIdx.x < 44) {
        sk0[threadIdx.x] = rk0[j * 44 + threadIdx.x];
        if (MODE == 0) sk1[threadIdx.x] = rk1[j * 44 + threadIdx.x];
    }
    __syncthreads();
    const LdsTab4 lt = lds_tab4_make(lds_te0);
    const uint32_t dw = j < 32 ? delta.x : (j < 64 ? delta.y : (j < 96 ? delta.z : delta.w));
    const bool dj = (dw >> (j & 31)) & 1u;
    // two counter blocks per trip (two AES in flight per key); the grid is a few workgroups per COLUMN, not per 1024
    // blocks: every workgroup stages the 128 KiB table image once (~25 us), which with 64 workgroups per column cost
    // more than the encryption itself
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < m128; b += 2 * stride) {
        const uint32_t b2 = b + stride;
        const bool two = b2 < m128;
        const uint64_t c = ctr0 + b, c2 = ctr0 + (two ? b2 : b);
        uint32_t s0[2][4] = {{(uint32_t)c, (uint32_t)(c >> 32), 0u, 0u}, {(uint32_t)c2, (uint32_t)(c2 >> 32), 0u, 0u}};
        aes_encrypt_n<2, LdsTab4>(lt, sk0, s0);
        if (MODE == 0) {
            uint32_t s1[2][4] = {{(uint32_t)c, (uint32_t)(c >> 32), 0u, 0u}, {(uint32_t)c2, (uint32_t)(c2 >> 32), 0u, 0u}};
            aes_encrypt_n<2, LdsTab4>(lt, sk1, s1);
#pragma unroll
            for (int e = 0; e < 2; e++) {
                if (e == 1 && !two) break;
                const uint32_t bb = e ? b2 : b;
                uint4 cb = cbits[bb];
                out0[(size_t)j * m128 + bb] = make_uint4(s0[e][0], s0[e][1], s0[e][2], s0[e][3]);
                out1[(size_t)j * m128 + bb] = make_uint4(s0[e][0] ^ s1[e][0] ^ cb.x, s0[e][1] ^ s1[e][1] ^ cb.y,
                                                         s0[e][2] ^ s1[e][2] ^ cb.z, s0[e][3] ^ s1[e][3] ^ cb.w);
            }
        } else {
            const uint32_t k = dj ? 0xffffffffu : 0u;
#pragma unroll
            for (int e = 0; e < 2; e++) {
                if (e == 1 && !two) break;
                const uint32_t bb = e ? b2 : b;
                uint4 u = Uin[(size_t)j * m128 + bb];
                out0[(size_t)j * m128 + bb] = make_uint4(s0[e][0] ^ (u.x & k), s0[e][1] ^ (u.y & k), s0[e][2] ^ (u.z & k),
                                                         s0[e][3] ^ (u.w & k));
            }
        }
    }
}

// ---- 128 x m bit transpose: cols[j][m128] (bit i of column j = bit (i & 127) of block i >> 7)
// -> rows[i] = 128 bits (bit j = column j).  One wave per 64 consecutive OTs: lane l loads the 64-bit
// word of column l (and l + 64) that covers them, and the wave transposes the 64 x 64 bit block in
// registers -- six butterfly stages, lane l exchanging with lane l ^ j (ds_bpermute) and swapping the
// off-diagonal j x j sub-blocks -- instead of one ballot per bit.
__device__ __forceinline__ uint64_t transpose64_lanes(uint64_t x, int lane) {
    uint64_t m = 0x00000000ffffffffull;
#pragma unroll
    for (int j = 32; j != 0; j >>= 1, m ^= (m << j)) {
        const int src = (lane ^ j) << 2;
        const uint32_t ylo = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)x);
        const uint32_t yhi = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)(x >> 32));
        const uint64_t y = ((uint64_t)yhi << 32) | ylo;
        // row k (bit j of the lane clear) keeps its low part and takes the partner's low part as its high part;
        // row k + j keeps its high part and takes the partner's high part as its low part
        x = (lane & j) ? ((x & ~m) | ((y >> j) & m)) : ((x & m) | ((y << j) & ~m));
    }
    return x;
}
// One wave transposes EIGHT consecutive 64-OT groups: lane l then reads 64 contiguous bytes of column l (and of column
// 64 + l) -- whole 64-byte sectors.  With one group per wave a lane read 8 bytes per column, each from a cache line of
// its own (the columns are m / 8 bytes apart): an eighth of every sector fetched was used, and the transpose, not the
// hashing, was the longest kernel of a batch (profiles/r3b_ot_kernel_stats.csv: 2 x 0.70 ms of 4.55 ms).
__global__ void __launch_bounds__(256)
ot_transpose_kernel(const uint64_t *cols, uint32_t m128, uint4 *rows, uint64_t m) {
    const int lane = threadIdx.x & 63;
    const uint64_t wv = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t i0 = wv * 512;
    if (i0 >= m) return;
    const uint64_t w64 = (uint64_t)m128 * 2;                       // 64-bit words per column
    const uint64_t first = i0 >> 6;                                // multiple of 8: 64-byte aligned within a column
    uint64_t a[8], b[8];
    const uint64_t *c0 = cols + (uint64_t)lane * w64 + first, *c1 = cols + (uint64_t)(64 + lane) * w64 + first;
#pragma unroll
    for (int t = 0; t < 8; t += 2) {
        if (first + t + 1 < w64) {                                 // (w64 is even: pairs never straddle the end)
            const uint4 u = *reinterpret_cast<const uint4 *>(c0 + t), v = *reinterpret_cast<const uint4 *>(c1 + t);
            a[t] = (uint64_t)u.x | ((uint64_t)u.y << 32); a[t + 1] = (uint64_t)u.z | ((uint64_t)u.w << 32);
            b[t] = (uint64_t)v.x | ((uint64_t)v.y << 32); b[t + 1] = (uint64_t)v.z | ((uint64_t)v.w << 32);
        } else {
            a[t] = a[t + 1] = b[t] = b[t + 1] = 0;
        }
    }
#pragma unroll
    for (int t = 0; t < 8; t++) {
        const uint64_t i = i0 + 64 * (uint64_t)t + (uint64_t)lane;
        if (i0 + 64 * (uint64_t)t >= m) break;                     // wave-uniform
        const uint64_t r0 = transpose64_lanes(a[t], lane), r1 = transpose64_lanes(b[t], lane);
        if (i < m) rows[i] = make_uint4((uint32_t)r0, (uint32_t)(r0 >> 32), (uint32_t)r1, (uint32_t)(r1 >> 32));
    }
}

__device__ __forceinline__ Lbl u4_lbl(uint4 v) { Lbl l = {v.x, v.y, v.z, v.w}; return l; }

// ---- Gilboa sender: OT i = (q * n + k) * w + bit.  y_i and per-pair share -sum x0.
// grid.y strides over the pairs (gridDim.y is limited to 65535).
__global__ void __launch_bounds__(1024)
ot_gilboa_send_kernel(const uint4 *rows, uint4 delta, const uint64_t *bvals, uint64_t n, int w, uint64_t m_per_pair,
                      uint64_t npairs, uint64_t tweak0, uint64_t *y, uint64_t *shares) {
    __shared__ uint32_t lds_te0[2 * kLdsTabWords];
    lds_tab4_fill(lds_te0);
    const LdsTab4 lt = lds_tab4_make(lds_te0);
    const uint64_t mask = w == 32 ? 0xffffffffull : ~0ull;
    const int lw = w == 32 ? 5 : 6;
    for (uint64_t q = blockIdx.y; q < npairs; q += gridDim.y) {
        uint64_t acc = 0;
        const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
        // two OTs per trip: four hashes, two in flight at a time (the pattern of the MAC kernel's garble_and)
        for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m_per_pair; t += 2 * stride) {
            const uint64_t t2 = t + stride;
            const bool two = t2 < m_per_pair;
            const uint64_t i = q * m_per_pair + t, i2 = q * m_per_pair + (two ? t2 : t);
            const Lbl r1 = u4_lbl(rows[i]), r2 = u4_lbl(rows[i2]);
            Lbl x[4] = {r1, lxor(r1, u4_lbl(delta)), r2, lxor(r2, u4_lbl(delta))};
            uint64_t tw[4] = {tweak0 + i, tweak0 + i, tweak0 + i2, tweak0 + i2};
            Lbl h[4];
            hash_n<2, LdsTab4>(lt, c_aes.rk, x, tw, h, c_aes.rk24);
            hash_n<2, LdsTab4>(lt, c_aes.rk, x + 2, tw + 2, h + 2, c_aes.rk24);
#pragma unroll
            for (int e = 0; e < 2; e++) {
                if (e == 1 && !two) break;
                const uint64_t tt = e ? t2 : t, ii = e ? i2 : i;
                const uint64_t k = tt >> lw;            // w is 32 or 64: no 64-bit division in the inner loop
                const int bit = (int)(tt & (uint64_t)(w - 1));
                uint64_t x0 = ((uint64_t)h[2 * e].x | ((uint64_t)h[2 * e].y << 32)) & mask;
                uint64_t h1 = ((uint64_t)h[2 * e + 1].x | ((uint64_t)h[2 * e + 1].y << 32)) & mask;
                uint64_t d = (bvals[q * n + k] << bit) & mask;
                y[ii] = (x0 + d - h1) & mask;
                acc -= x0;
            }
        }
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd((unsigned long long *)&shares[q], (unsigned long long)acc);
    }
}

__global__ void __launch_bounds__(1024)
ot_gilboa_recv_kernel(const uint4 *rows, const uint64_t *avals, uint64_t n, int w, uint64_t m_per_pair, uint64_t npairs,
                      uint64_t tweak0, const uint64_t *y, uint64_t *shares) {
    __shared__ uint32_t lds_te0[2 * kLdsTabWords];
    lds_tab4_fill(lds_te0);
    const LdsTab4 lt = lds_tab4_make(lds_te0);
    const uint64_t mask = w == 32 ? 0xffffffffull : ~0ull;
    const int lw = w == 32 ? 5 : 6;
    for (uint64_t q = blockIdx.y; q < npairs; q += gridDim.y) {
        uint64_t acc = 0;
        const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
        for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m_per_pair; t += 2 * stride) {
            const uint64_t t2 = t + stride;
            const bool two = t2 < m_per_pair;
            const uint64_t i = q * m_per_pair + t, i2 = q * m_per_pair + (two ? t2 : t);
            Lbl x[2] = {u4_lbl(rows[i]), u4_lbl(rows[i2])};
            uint64_t tw[2] = {tweak0 + i, tweak0 + i2};
            const uint64_t yv[2] = {y[i], y[i2]};         // in flight during the hashes
            Lbl h[2];
            hash_n<2, LdsTab4>(lt, c_aes.rk, x, tw, h, c_aes.rk24);
#pragma unroll
            for (int e = 0; e < 2; e++) {
                if (e == 1 && !two) break;
                const uint64_t tt = e ? t2 : t;
                const uint64_t k = tt >> lw;            // w is 32 or 64: no 64-bit division in the inner loop
                const int bit = (int)(tt & (uint64_t)(w - 1));
                uint64_t v = ((uint64_t)h[e].x | ((uint64_t)h[e].y << 32)) & mask;
                if ((avals[q * n + k] >> bit) & 1ull) v += yv[e];
                acc += v;
            }
        }
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd((unsigned long long *)&shares[q], (unsigned long long)acc);
    }
}

// ---- Gilboa on a whole block Xr^T Xs, one VECTOR OT per bit of the receiver's operand (include/linreg_gc_ot_matrix.h):
// OT i = (k * r + ir) * W + bit carries s words, block c of its pads is H(row_i, tweak0 + i * nblk + c), word e of block c is
// sender column j = c * (128 / W) + e.  A lane owns one slot = ir * nblk + c of the r * nblk slots and walks a slice of the
// (k, bit) range: kb = slice, slice + ks, ...; its 128 / W partial sums stay in registers and end in one integer atomicAdd per
// word (exact and order-independent).  A wave is 64 consecutive slots (chunk) of one slice: the nblk lanes of one OT read the
// same 16-byte row and their y words are one contiguous run of s * W / 8 bytes.  Wave g of the grid is chunk g % nsc of slice
// g / nsc; waves past nsc * ks and lanes past the last slot hash a valid row and drop the result.
struct OtMatrixGeom {
    uint32_t r, s, nblk, nslot, nsc, ks;   // nsc = ceil(nslot / 64) chunks, ks slices
    uint64_t kb;                           // units of the walk: rows * W OTs (matrix), rows * W / 2 pairs of OTs (half payload)
    int vec;                               // every OT's y run is 16-byte aligned (s * W % 128 == 0 and y itself is): whole-block stores
};
template <int W> struct OtWord;
template <> struct OtWord<32> { typedef uint32_t T; };
template <> struct OtWord<64> { typedef uint64_t T; };
template <int W> __device__ __forceinline__ uint64_t ot_pad_word(const Lbl &h, int e) {
    if (W == 64) return e ? ((uint64_t)h.z | ((uint64_t)h.w << 32)) : ((uint64_t)h.x | ((uint64_t)h.y << 32));
    return e == 0 ? h.x : (e == 1 ? h.y : (e == 2 ? h.z : h.w));
}
// What the four block kernels (matrix and half payload, each role) share: a lane's place, its y accesses, its pads, its share words.
// A lane's place in the grid: its slot (ir, c), the first of its sender columns j0, its slice of the walk, whether its y runs move
// as whole 16-byte blocks, and its 128 / W partial sums.  Lanes past the last slot are not live: they hash a valid row (slot 0's)
// and drop the result.
template <int W> struct OtLane {
    uint32_t ir, c, j0;
    uint64_t slice;
    bool live, whole;
    uint64_t acc[128 / W];
};
// false: the lane's wave is past the grid's nsc * ks waves, nothing to do
template <int W> __device__ __forceinline__ bool ot_lane_place(const OtMatrixGeom &g, OtLane<W> &ln) {
    const int WPB = 128 / W;
    const uint64_t wv = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (wv >= (uint64_t)g.nsc * g.ks) return false;
    const uint32_t slot = (uint32_t)(wv % g.nsc) * 64u + (threadIdx.x & 63u);
    ln.slice = wv / g.nsc;
    ln.live = slot < g.nslot;
    ln.ir = ln.live ? slot / g.nblk : 0u;
    ln.c = ln.live ? slot - ln.ir * g.nblk : 0u;
    ln.j0 = ln.c * WPB;
    ln.whole = g.vec && ln.j0 + WPB <= g.s;
#pragma unroll
    for (int e = 0; e < WPB; e++) ln.acc[e] = 0;
    return true;
}
// the lane's partial sums into the r x s share block: one integer atomicAdd per word (exact and order-independent)
template <int W> __device__ __forceinline__ void ot_lane_add_shares(const OtMatrixGeom &g, const OtLane<W> &ln, uint64_t *shares) {
    if (!ln.live) return;
#pragma unroll
    for (int e = 0; e < 128 / W; e++)
        if (ln.j0 + e < g.s) atomicAdd((unsigned long long *)&shares[(uint64_t)ln.ir * g.s + ln.j0 + e], (unsigned long long)ln.acc[e]);
}
// the lane's 128 / W words of one run of y: a whole 16-byte block, or word by word what lies inside the s columns
template <int W> __device__ __forceinline__ void ot_y_store(typename OtWord<W>::T *yo, const typename OtWord<W>::T *yv, bool whole, uint32_t j0, uint32_t s) {
    const int WPB = 128 / W;
    if (whole) {
        // a native vector: one 16-byte store.  As a uint4 built from halves of words, the compiler took the block apart again and
        // merged its tail with the word stores below in some of the kernels (profiles/ot_block_refactor.txt)
        typedef typename OtWord<W>::T block __attribute__((ext_vector_type(128 / W)));
        block v;
#pragma unroll
        for (int e = 0; e < WPB; e++) v[e] = yv[e];
        *reinterpret_cast<block *>(yo) = v;
    } else {
#pragma unroll
        for (int e = 0; e < WPB; e++) if (j0 + e < s) yo[e] = yv[e];
    }
}
template <int W> __device__ __forceinline__ void ot_y_load(const typename OtWord<W>::T *yi, typename OtWord<W>::T *yv, bool whole, bool live, uint32_t j0, uint32_t s) {
    typedef typename OtWord<W>::T word;
    const int WPB = 128 / W;
    if (whole) {
        const uint4 v = *reinterpret_cast<const uint4 *>(yi);
        if (W == 64) { yv[0] = (word)((uint64_t)v.x | ((uint64_t)v.y << 32)); yv[1 % WPB] = (word)((uint64_t)v.z | ((uint64_t)v.w << 32)); }
        else { yv[0] = (word)v.x; yv[1] = (word)v.y; yv[2 % WPB] = (word)v.z; yv[3 % WPB] = (word)v.w; }
    } else {
#pragma unroll
        for (int e = 0; e < WPB; e++) yv[e] = live && j0 + e < s ? yi[e] : (word)0;
    }
}
// block c of the pads of the OTs ia and ib, tweaks tweak0 + i * nblk + c.  Sender: h = H(q_ia), H(q_ia ^ D), H(q_ib), H(q_ib ^ D),
// four hashes, two in flight at a time (as ot_gilboa_send_kernel).  Receiver: h = H(t_ia), H(t_ib), one pair in flight.
__device__ __forceinline__ void ot_pads_send(const LdsTab4 &lt, const uint4 *rows, uint4 delta, uint64_t tweak0, uint32_t nblk, uint32_t c,
                                             uint64_t ia, uint64_t ib, Lbl h[4]) {
    const Lbl r1 = u4_lbl(rows[ia]), r2 = u4_lbl(rows[ib]);
    Lbl x[4] = {r1, lxor(r1, u4_lbl(delta)), r2, lxor(r2, u4_lbl(delta))};
    const uint64_t t1 = tweak0 + ia * nblk + c, t2 = tweak0 + ib * nblk + c;
    uint64_t tw[4] = {t1, t1, t2, t2};
    hash_n<2, LdsTab4>(lt, c_aes.rk, x, tw, h, c_aes.rk24);
    hash_n<2, LdsTab4>(lt, c_aes.rk, x + 2, tw + 2, h + 2, c_aes.rk24);
}
__device__ __forceinline__ void ot_pads_recv(const LdsTab4 &lt, const uint4 *rows, uint64_t tweak0, uint32_t nblk, uint32_t c, uint64_t ia,
                                             uint64_t ib, Lbl h[2]) {
    Lbl x[2] = {u4_lbl(rows[ia]), u4_lbl(rows[ib])};
    uint64_t tw[2] = {tweak0 + ia * nblk + c, tweak0 + ib * nblk + c};
    hash_n<2, LdsTab4>(lt, c_aes.rk, x, tw, h, c_aes.rk24);
}
template <int W>
__global__ void __launch_bounds__(1024)
ot_gilboa_matrix_send_kernel(const uint4 *rows, uint4 delta, const uint64_t *xs, OtMatrixGeom g, uint64_t tweak0,
                             typename OtWord<W>::T *y, uint64_t *shares) {
    __shared__ uint32_t lds_te0[2 * kLdsTabWords];
    lds_tab4_fill(lds_te0);
    const LdsTab4 lt = lds_tab4_make(lds_te0);
    typedef typename OtWord<W>::T word;
    const int WPB = 128 / W, lw = W == 32 ? 5 : 6;
    OtLane<W> ln;
    if (!ot_lane_place<W>(g, ln)) return;
    // two OTs per trip
    for (uint64_t kb = ln.slice; kb < g.kb; kb += 2 * (uint64_t)g.ks) {
        const uint64_t kb2 = kb + g.ks;
        const bool two = kb2 < g.kb;
        const uint64_t kk[2] = {kb, two ? kb2 : kb};
        uint64_t i[2];
#pragma unroll
        for (int t = 0; t < 2; t++) i[t] = ((kk[t] >> lw) * g.r + ln.ir) * W + (kk[t] & (uint64_t)(W - 1));
        Lbl h[4];
        ot_pads_send(lt, rows, delta, tweak0, g.nblk, ln.c, i[0], i[1], h);
        if (!ln.live) continue;
#pragma unroll
        for (int t = 0; t < 2; t++) {
            if (t == 1 && !two) break;
            const uint64_t k = kk[t] >> lw;
            const int bit = (int)(kk[t] & (uint64_t)(W - 1));
            word yv[WPB];
#pragma unroll
            for (int e = 0; e < WPB; e++) {
                const uint64_t x0 = ot_pad_word<W>(h[2 * t], e), x1 = ot_pad_word<W>(h[2 * t + 1], e);
                const bool in = ln.j0 + e < g.s;
                const uint64_t d = in ? xs[k * g.s + ln.j0 + e] << bit : 0;
                yv[e] = (word)(x0 + d - x1);
                if (in) ln.acc[e] -= x0;
            }
            ot_y_store<W>(y + i[t] * g.s + ln.j0, yv, ln.whole, ln.j0, g.s);
        }
    }
    ot_lane_add_shares<W>(g, ln, shares);
}
template <int W>
__global__ void __launch_bounds__(1024)
ot_gilboa_matrix_recv_kernel(const uint4 *rows, const uint64_t *xr, OtMatrixGeom g, uint64_t tweak0, const typename OtWord<W>::T *y,
                             uint64_t *shares) {
    __shared__ uint32_t lds_te0[2 * kLdsTabWords];
    lds_tab4_fill(lds_te0);
    const LdsTab4 lt = lds_tab4_make(lds_te0);
    typedef typename OtWord<W>::T word;
    const int WPB = 128 / W, lw = W == 32 ? 5 : 6;
    OtLane<W> ln;
    if (!ot_lane_place<W>(g, ln)) return;
    for (uint64_t kb = ln.slice; kb < g.kb; kb += 2 * (uint64_t)g.ks) {
        const uint64_t kb2 = kb + g.ks;
        const bool two = kb2 < g.kb;
        const uint64_t kk[2] = {kb, two ? kb2 : kb};
        uint64_t i[2];
#pragma unroll
        for (int t = 0; t < 2; t++) i[t] = ((kk[t] >> lw) * g.r + ln.ir) * W + (kk[t] & (uint64_t)(W - 1));
        word yv[2][WPB];                                   // in flight during the hashes
#pragma unroll
        for (int t = 0; t < 2; t++) ot_y_load<W>(y + i[t] * g.s + ln.j0, yv[t], ln.whole, ln.live, ln.j0, g.s);
        Lbl h[2];
        ot_pads_recv(lt, rows, tweak0, g.nblk, ln.c, i[0], i[1], h);
        if (!ln.live) continue;
#pragma unroll
        for (int t = 0; t < 2; t++) {
            if (t == 1 && !two) break;
            const uint64_t k = kk[t] >> lw;
            const int bit = (int)(kk[t] & (uint64_t)(W - 1));
            const bool ci = (xr[k * g.r + ln.ir] >> bit) & 1ull;
#pragma unroll
            for (int e = 0; e < WPB; e++)
                if (ln.j0 + e < g.s) ln.acc[e] += ot_pad_word<W>(h[t], e) + (ci ? (uint64_t)yv[t][e] : 0ull);
        }
    }
    ot_lane_add_shares<W>(g, ln, shares);
}

// ---- The half-payload form of the matrix mode (include/linreg_gc_ot_half.h): the OTs, the pads and the slots are the matrix
// kernels'; bit `bit` of the product runs mod 2^(W - bit) and is shifted afterwards, so OT i carries W - bit bits per column and the
// W fields of one (k, ir, j) pack into H = W / 2 + 1 words: word ((k * r + ir) * H + p) * s + j.  The unit of the walk is the PAIR
// of OTs of one (k, ir) that fills the same words: unit q = 0 is bits (0, W / 2) and writes words 0 and W / 2, unit 1 <= q < W / 2
// is bits (q, W - q) and writes word q (bit q below, bit W - q in the q bits above).  There are g.kb = rows * W / 2 units, unit
// un = k * (W / 2) + q; a wave is one chunk of 64 slots on the units slice, slice + ks, ...: one unit per trip, so a send trip is
// four hashes and a receive trip two, always two in flight, Xs[k][j] and Xr[k][ir] are read once, and every word of y is composed
// in registers and written by one lane, once.  q is the same for a whole wave, so the second run of unit 0 does not diverge.
template <int W> __device__ __forceinline__ uint64_t ot_half_mask(int bit) { return ~0ull >> (64 - W + bit); }   // 2^(W - bit) - 1: a shift by 0 .. 63, never by W
template <int W>
__global__ void __launch_bounds__(1024)
ot_gilboa_half_send_kernel(const uint4 *rows, uint4 delta, const uint64_t *xs, OtMatrixGeom g, uint64_t tweak0,
                           typename OtWord<W>::T *y, uint64_t *shares) {
    __shared__ uint32_t lds_te0[2 * kLdsTabWords];
    lds_tab4_fill(lds_te0);
    const LdsTab4 lt = lds_tab4_make(lds_te0);
    typedef typename OtWord<W>::T word;
    const int WPB = 128 / W, HW = W / 2, H = HW + 1, lh = W == 32 ? 4 : 5;
    OtLane<W> ln;
    if (!ot_lane_place<W>(g, ln)) return;
    for (uint64_t un = ln.slice; un < g.kb; un += g.ks) {
        const uint64_t k = un >> lh, kr = k * g.r + ln.ir;
        const int q = (int)(un & (uint64_t)(HW - 1));
        const int ba = q, bb = q ? W - q : HW;
        Lbl h[4];
        ot_pads_send(lt, rows, delta, tweak0, g.nblk, ln.c, kr * W + ba, kr * W + bb, h);
        if (!ln.live) continue;
        const uint64_t ma = ot_half_mask<W>(ba), mb = ot_half_mask<W>(bb);
        word lo[WPB], hi[WPB];
#pragma unroll
        for (int e = 0; e < WPB; e++) {
            const bool in = ln.j0 + e < g.s;
            const uint64_t xv = in ? xs[k * g.s + ln.j0 + e] : 0;
            const uint64_t x0a = ot_pad_word<W>(h[0], e), x1a = ot_pad_word<W>(h[1], e), x0b = ot_pad_word<W>(h[2], e), x1b = ot_pad_word<W>(h[3], e);
            const uint64_t ya = (x0a + xv - x1a) & ma, yb = (x0b + xv - x1b) & mb;
            if (in) ln.acc[e] -= ((x0a & ma) << ba) + ((x0b & mb) << bb);
            lo[e] = q ? (word)(ya | (yb << bb)) : (word)ya;            // (bb = W - q is 1 .. W - 1 here)
            hi[e] = (word)yb;
        }
        word *yo = y + (kr * H + q) * g.s + ln.j0;
        ot_y_store<W>(yo, lo, ln.whole, ln.j0, g.s);
        if (!q) ot_y_store<W>(yo + (uint64_t)HW * g.s, hi, ln.whole, ln.j0, g.s);
    }
    ot_lane_add_shares<W>(g, ln, shares);
}
template <int W>
__global__ void __launch_bounds__(1024)
ot_gilboa_half_recv_kernel(const uint4 *rows, const uint64_t *xr, OtMatrixGeom g, uint64_t tweak0, const typename OtWord<W>::T *y,
                           uint64_t *shares) {
    __shared__ uint32_t lds_te0[2 * kLdsTabWords];
    lds_tab4_fill(lds_te0);
    const LdsTab4 lt = lds_tab4_make(lds_te0);
    typedef typename OtWord<W>::T word;
    const int WPB = 128 / W, HW = W / 2, H = HW + 1, lh = W == 32 ? 4 : 5;
    OtLane<W> ln;
    if (!ot_lane_place<W>(g, ln)) return;
    for (uint64_t un = ln.slice; un < g.kb; un += g.ks) {
        const uint64_t k = un >> lh, kr = k * g.r + ln.ir;
        const int q = (int)(un & (uint64_t)(HW - 1));
        const int ba = q, bb = q ? W - q : HW;
        const word *yi = y + (kr * H + q) * g.s + ln.j0;
        word lo[WPB], hi[WPB];                             // in flight during the hashes
        ot_y_load<W>(yi, lo, ln.whole, ln.live, ln.j0, g.s);
        if (!q) ot_y_load<W>(yi + (uint64_t)HW * g.s, hi, ln.whole, ln.live, ln.j0, g.s);
        Lbl h[2];
        ot_pads_recv(lt, rows, tweak0, g.nblk, ln.c, kr * W + ba, kr * W + bb, h);
        if (!ln.live) continue;
        const uint64_t xv = xr[kr];
        const bool ca = (xv >> ba) & 1ull, cb = (xv >> bb) & 1ull;
        const uint64_t ma = ot_half_mask<W>(ba), mb = ot_half_mask<W>(bb);
#pragma unroll
        for (int e = 0; e < WPB; e++) {
            if (ln.j0 + e >= g.s) continue;
            const uint64_t ya = (uint64_t)lo[e], yb = q ? (uint64_t)lo[e] >> bb : (uint64_t)hi[e];     // (the masks drop what lies above a field)
            ln.acc[e] += (((ot_pad_word<W>(h[0], e) + (ca ? ya : 0ull)) & ma) << ba) + (((ot_pad_word<W>(h[1], e) + (cb ? yb : 0ull)) & mb) << bb);
        }
    }
    ot_lane_add_shares<W>(g, ln, shares);
}

// choice bits of the Gilboa receiver: bit i = bit (i % w) of a[i / w], packed LSB-first
__global__ void ot_pack_choice_words_kernel(const uint64_t *avals, uint64_t nwords, int w, uint64_t *cbits) {
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w == 64) {
        if (t < nwords) cbits[t] = avals[t];
    } else {
        if (2 * t < nwords) {
            uint64_t lo = avals[2 * t] & 0xffffffffull;
            uint64_t hi = 2 * t + 1 < nwords ? (avals[2 * t + 1] & 0xffffffffull) : 0;
            cbits[t] = lo | (hi << 32);
        }
    }
}
// choice bits of a label transfer: one byte per OT (bool *sel, src/input.c:40-44) -> packed LSB-first
__global__ void ot_pack_choice_bytes_kernel(const uint8_t *choice, uint64_t m, uint64_t *cbits, uint64_t nwords64) {
    const uint64_t wv = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (wv >= nwords64) return;
    const uint64_t i = wv * 64 + lane;
    const uint64_t bits = __ballot(i < m && choice[i] != 0);
    if (lane == 0) cbits[wv] = bits;
}

// ---- 1-of-2 OT of 16-byte messages
__global__ void __launch_bounds__(1024)
ot_labels_send_kernel(const uint4 *rows, uint4 delta, const uint4 *m0, const uint4 *m1, uint64_t m, uint64_t tweak0, uint4 *e) {
    __shared__ uint32_t lds_te0[2 * kLdsTabWords];
    lds_tab4_fill(lds_te0);
    const LdsTab4 lt = lds_tab4_make(lds_te0);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += 2 * stride) {
        const bool two = i + stride < m;
        const uint64_t i2 = two ? i + stride : i;
        const Lbl r1 = u4_lbl(rows[i]), r2 = u4_lbl(rows[i2]);
        Lbl x[4] = {r1, lxor(r1, u4_lbl(delta)), r2, lxor(r2, u4_lbl(delta))};
        uint64_t tw[4] = {tweak0 + i, tweak0 + i, tweak0 + i2, tweak0 + i2};
        Lbl h[4];
        hash_n<2, LdsTab4>(lt, c_aes.rk, x, tw, h, c_aes.rk24);
        hash_n<2, LdsTab4>(lt, c_aes.rk, x + 2, tw + 2, h + 2, c_aes.rk24);
#pragma unroll
        for (int k = 0; k < 2; k++) {
            if (k == 1 && !two) break;
            const uint64_t ii = k ? i2 : i;
            uint4 a = m0[ii], b = m1[ii];
            e[2 * ii] = make_uint4(a.x ^ h[2 * k].x, a.y ^ h[2 * k].y, a.z ^ h[2 * k].z, a.w ^ h[2 * k].w);
            e[2 * ii + 1] = make_uint4(b.x ^ h[2 * k + 1].x, b.y ^ h[2 * k + 1].y, b.z ^ h[2 * k + 1].z, b.w ^ h[2 * k + 1].w);
        }
    }
}
__global__ void __launch_bounds__(1024)
ot_labels_recv_kernel(const uint4 *rows, const uint64_t *cbits, const uint4 *e, uint64_t m, uint64_t tweak0, uint4 *out) {
    __shared__ uint32_t lds_te0[2 * kLdsTabWords];
    lds_tab4_fill(lds_te0);
    const LdsTab4 lt = lds_tab4_make(lds_te0);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += 2 * stride) {
        const bool two = i + stride < m;
        const uint64_t i2 = two ? i + stride : i;
        Lbl x[2] = {u4_lbl(rows[i]), u4_lbl(rows[i2])};
        uint64_t tw[2] = {tweak0 + i, tweak0 + i2};
        const uint32_t c1 = (uint32_t)(cbits[i >> 6] >> (i & 63)) & 1u, c2 = (uint32_t)(cbits[i2 >> 6] >> (i2 & 63)) & 1u;
        const uint4 ev1 = e[2 * i + c1], ev2 = e[2 * i2 + c2];      // in flight during the hashes
        Lbl h[2];
        hash_n<2, LdsTab4>(lt, c_aes.rk, x, tw, h, c_aes.rk24);
        out[i] = make_uint4(ev1.x ^ h[0].x, ev1.y ^ h[0].y, ev1.z ^ h[0].z, ev1.w ^ h[0].w);
        if (two) out[i2] = make_uint4(ev2.x ^ h[1].x, ev2.y ^ h[1].y, ev2.z ^ h[1].z, ev2.w ^ h[1].w);
    }
}

// Launch geometry.  Every workgroup of these kernels stages the 128 KiB four-table AES image in LDS before its first
// block (one workgroup per CU, ~25 us), so a launch uses about two workgroups per CU and lets them loop -- not one
// workgroup per 1024 items: with 16 384 workgroups for a 64-pair batch the staging alone took 1.7 ms of each 2.1 ms
// payload kernel (profiles/r2e_ot_kernel_stats.csv; after: profiles/r3_ot_kernel_stats.csv).
static const unsigned kOtGroups = 512;
static unsigned ot_cols_groups(uint64_t m128) {           // workgroups per column (grid.y = 128 columns)
    unsigned gx = (unsigned)((m128 + 2047) / 2048);
    const unsigned cap = kOtGroups / 128;
    return gx > cap ? cap : (gx ? gx : 1);
}
static void ot_pair_grid(uint64_t mpp, uint64_t npairs, unsigned &gx, unsigned &gy) {   // grid.y strides over the pairs
    gy = npairs > kOtGroups ? kOtGroups : (unsigned)(npairs ? npairs : 1);
    gx = (unsigned)((mpp + 2047) / 2048);
    const unsigned cap = kOtGroups / gy ? kOtGroups / gy : 1;
    if (gx > cap) gx = cap;
    if (!gx) gx = 1;
}

// =============================================================== sessions
// Every session owns a HIP stream and grow-only device buffers: no hipMalloc / hipFree on the transfer
// paths after the first call of a given size.  Host arguments move with hipMemcpyAsync on the session
// stream (full PCIe rate for page-locked buffers, lgc_host_alloc); with device I/O switched on
// (lgc_ot_*_set_device_io) the pointer arguments ARE device memory and the kernels use them in place --
// the hand-off for callers that already hold the operands in HBM (lgc_p1_* outputs, a peer's u / y
// mapped over hipIpc), without a host round trip.
struct DevBuf {
    void *p;
    size_t cap;
    DevBuf() : p(0), cap(0) {}
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { (void)hipMemset(p, 0, cap); (void)hipFree(p); }   // q-rows / messages never stay behind in freed memory
        p = 0; cap = 0;
        size_t want = bytes + bytes / 8;                  // headroom: batches of slightly different size do not reallocate
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = 0; cap = 0; }
};
struct lgc_ot_sender {
    int device;
    uint4 delta;
    uint32_t *rk;          // 128 x 44 round keys of G(k_j^{Delta_j})
    uint64_t ctr;          // PRG stream position (blocks), same on both sides
    uint64_t tweak;        // hash tweak counter (OT index), same on both sides
    hipStream_t st;
    bool dev_io;
    DevBuf Q, U, rows, b, y, sh, m0, m1, e;
};
static const size_t kMaxRecvInFlight = 4;
enum { kSlotLabels = 0, kSlotGilboa = 1, kSlotMatrix = 2, kSlotHalf = 3 };   // what a receive in flight is: its finish must be of the same kind
struct lgc_ot_receiver {
    int device;
    uint32_t *rk0, *rk1;
    uint64_t ctr, tweak;
    hipStream_t st;
    bool dev_io;
    DevBuf T0, U, y, sh, e, out, choice;
    // receives started but not finished yet, oldest first: *_recv_start fills the next slot and
    // *_recv_finish takes the oldest, so a caller may keep a few batches in flight (one thread
    // starting and sending u, another receiving the replies and finishing)
    struct Slot {
        DevBuf rows, cbits, avals;
        const uint64_t *avals_dev;     // device I/O: the caller's a stays where it is
        uint64_t m, npairs, n; int w; uint64_t tweak_cur; int kind;   // kSlot*; a matrix or half receive: npairs = r, n = s, rows = m / (r w)
    } slot[kMaxRecvInFlight];
    size_t head, count;                // ring of slots in use
    std::mutex mu;
};

static int upload_keys(const uint8_t seeds[][16], uint32_t **out) {
    std::vector<uint32_t> rk(128 * 44);
    for (int j = 0; j < 128; j++) {
        AesTables t;
        aes_build_tables(t, seeds[j]);
        memcpy(&rk[j * 44], t.rk, sizeof(t.rk));
    }
    OTCHK(hipMalloc(out, rk.size() * 4));
    OTCHK(hipMemcpy(*out, rk.data(), rk.size() * 4, hipMemcpyHostToDevice));
    return LGC_OK;
}

extern "C" void lgc_ot_sender_destroy(lgc_ot_sender *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->st) { (void)hipStreamSynchronize(s->st); lgc_stream_give(s->device, s->st); }
    // q-rows and the sender's messages (both labels of every input bit) must not outlive the session in freed memory
    DevBuf *all[] = {&s->Q, &s->U, &s->rows, &s->b, &s->y, &s->sh, &s->m0, &s->m1, &s->e};
    for (DevBuf *d : all) { if (d->p) (void)hipMemset(d->p, 0, d->cap); d->release(); }
    if (s->rk) (void)hipFree(s->rk);
    delete s;
}
extern "C" int lgc_ot_sender_create(lgc_ot_sender **out, int device, const uint8_t delta[16], const uint8_t seeds[128][16]) {
    if (!out || !delta || !seeds) return lgc_fail(LGC_EINVAL, "null argument");
    int rc = lgc_need_device(device);
    if (rc) return rc;
    lgc_ot_sender *s = new lgc_ot_sender();
    s->device = device; s->ctr = 0; s->tweak = 0; s->rk = 0; s->st = 0; s->dev_io = false;
    memcpy(&s->delta, delta, 16);
    rc = upload_keys(seeds, &s->rk);
    if (rc) { lgc_ot_sender_destroy(s); return rc; }
    *out = s;
    return LGC_OK;
}
extern "C" void lgc_ot_receiver_destroy(lgc_ot_receiver *r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    if (r->st) { (void)hipStreamSynchronize(r->st); lgc_stream_give(r->device, r->st); }
    DevBuf *all[] = {&r->T0, &r->U, &r->y, &r->sh, &r->e, &r->out, &r->choice};
    for (DevBuf *d : all) { if (d->p) (void)hipMemset(d->p, 0, d->cap); d->release(); }
    for (size_t k = 0; k < kMaxRecvInFlight; k++) {
        DevBuf *sl[] = {&r->slot[k].rows, &r->slot[k].cbits, &r->slot[k].avals};
        for (DevBuf *d : sl) { if (d->p) (void)hipMemset(d->p, 0, d->cap); d->release(); }
    }
    if (r->rk0) (void)hipFree(r->rk0);
    if (r->rk1) (void)hipFree(r->rk1);
    delete r;
}
extern "C" int lgc_ot_receiver_create(lgc_ot_receiver **out, int device, const uint8_t seeds0[128][16], const uint8_t seeds1[128][16]) {
    if (!out || !seeds0 || !seeds1) return lgc_fail(LGC_EINVAL, "null argument");
    int rc = lgc_need_device(device);
    if (rc) return rc;
    lgc_ot_receiver *r = new lgc_ot_receiver();
    r->device = device; r->rk0 = 0; r->rk1 = 0; r->ctr = 0; r->tweak = 0; r->st = 0; r->dev_io = false; r->head = 0; r->count = 0;
    rc = upload_keys(seeds0, &r->rk0);
    if (!rc) rc = upload_keys(seeds1, &r->rk1);
    if (rc) { lgc_ot_receiver_destroy(r); return rc; }
    *out = r;
    return LGC_OK;
}
extern "C" int lgc_ot_sender_set_device_io(lgc_ot_sender *s, int on) {
    if (!s) return lgc_fail(LGC_EINVAL, "null session");
    s->dev_io = on != 0;
    return LGC_OK;
}
extern "C" int lgc_ot_receiver_set_device_io(lgc_ot_receiver *r, int on) {
    if (!r) return lgc_fail(LGC_EINVAL, "null session");
    r->dev_io = on != 0;
    return LGC_OK;
}

static inline uint64_t round128(uint64_t m) { return (m + 127) / 128 * 128; }
#define OTLAUNCH() OTCHK(hipGetLastError())

// receiver: columns + u + transpose for the choice bits in slot->cbits (padded to m128 blocks)
static int recv_extend(lgc_ot_receiver *r, lgc_ot_receiver::Slot *sl, uint64_t m, uint8_t *u_out) {
    const uint32_t m128 = (uint32_t)(round128(m) / 128);
    const size_t cbytes = (size_t)128 * m128 * 16;
    OTCHK(r->T0.ensure(cbytes));
    uint4 *U = reinterpret_cast<uint4 *>(u_out);
    if (!r->dev_io) { OTCHK(r->U.ensure(cbytes)); U = static_cast<uint4 *>(r->U.p); }
    OTCHK(sl->rows.ensure((size_t)m128 * 128 * 16));
    unsigned gx = ot_cols_groups(m128);
    hipLaunchKernelGGL((ot_cols_kernel<0>), dim3(gx, 128), dim3(1024), 0, r->st, r->rk0, r->rk1, r->ctr, m128,
                       (const uint4 *)sl->cbits.p, (const uint4 *)0, make_uint4(0, 0, 0, 0), (uint4 *)r->T0.p, U);
    OTLAUNCH();
    if (!r->dev_io) OTCHK(hipMemcpyAsync(u_out, U, cbytes, hipMemcpyDeviceToHost, r->st));   // overlaps the transpose
    const uint64_t mp = (uint64_t)m128 * 128;
    hipLaunchKernelGGL(ot_transpose_kernel, dim3((unsigned)((mp / 512 + 4) / 4)), dim3(256), 0, r->st, (const uint64_t *)r->T0.p, m128,
                       (uint4 *)sl->rows.p, mp);
    OTLAUNCH();
    OTCHK(hipStreamSynchronize(r->st));
    r->ctr += m128;
    return LGC_OK;
}
static int send_extend(lgc_ot_sender *s, uint64_t m, const uint8_t *u_in) {
    const uint32_t m128 = (uint32_t)(round128(m) / 128);
    const size_t cbytes = (size_t)128 * m128 * 16;
    OTCHK(s->Q.ensure(cbytes));
    OTCHK(s->rows.ensure((size_t)m128 * 128 * 16));
    const uint4 *U = reinterpret_cast<const uint4 *>(u_in);
    if (!s->dev_io) {
        OTCHK(s->U.ensure(cbytes));
        OTCHK(hipMemcpyAsync(s->U.p, u_in, cbytes, hipMemcpyHostToDevice, s->st));
        U = static_cast<const uint4 *>(s->U.p);
    }
    unsigned gx = ot_cols_groups(m128);
    hipLaunchKernelGGL((ot_cols_kernel<1>), dim3(gx, 128), dim3(1024), 0, s->st, s->rk, (const uint32_t *)0, s->ctr, m128,
                       (const uint4 *)0, U, s->delta, (uint4 *)s->Q.p, (uint4 *)0);
    OTLAUNCH();
    const uint64_t mp = (uint64_t)m128 * 128;
    hipLaunchKernelGGL(ot_transpose_kernel, dim3((unsigned)((mp / 512 + 4) / 4)), dim3(256), 0, s->st, (const uint64_t *)s->Q.p, m128,
                       (uint4 *)s->rows.p, mp);
    OTLAUNCH();
    s->ctr += m128;
    return LGC_OK;
}

extern "C" size_t lgc_ot_u_bytes(uint64_t m) { return (size_t)(round128(m) / 128) * 128 * 16; }

static lgc_ot_receiver::Slot *slot_push(lgc_ot_receiver *r) {
    if (r->count >= kMaxRecvInFlight) return 0;
    lgc_ot_receiver::Slot *sl = &r->slot[(r->head + r->count) % kMaxRecvInFlight];
    r->count++;
    return sl;
}
static void slot_unpush(lgc_ot_receiver *r) { r->count--; }
static lgc_ot_receiver::Slot *slot_front(lgc_ot_receiver *r) { return r->count ? &r->slot[r->head] : 0; }
static void slot_pop(lgc_ot_receiver *r) { r->head = (r->head + 1) % kMaxRecvInFlight; r->count--; }
// the slot a *_recv_start took goes back unless the start goes through; the one a *_recv_finish works on is consumed on every path
struct Undo { lgc_ot_receiver *r; bool armed; ~Undo() { if (armed) slot_unpush(r); } };
struct Pop { lgc_ot_receiver *r; ~Pop() { slot_pop(r); } };

// ---------------------------------------------------------------- Gilboa
// What every Gilboa entry point (per pair, matrix, half payload) does around its payload kernel.
// A host argument of `bytes` bytes as the kernels see it: staged in `buf` (copied there first when copy_in), or, with device I/O, where it is
static int stage(hipStream_t st, bool dev_io, DevBuf &buf, const void *arg, size_t bytes, bool copy_in, const void **dev) {
    *dev = arg;
    if (dev_io) return LGC_OK;
    OTCHK(buf.ensure(bytes));
    if (copy_in) OTCHK(hipMemcpyAsync(buf.p, arg, bytes, hipMemcpyHostToDevice, st));
    *dev = buf.p;
    return LGC_OK;
}
// the nsh share words a payload kernel sums into, zeroed
static int shares_zero(hipStream_t st, DevBuf &sh, uint64_t nsh) {
    OTCHK(sh.ensure(nsh * 8));
    OTCHK(hipMemsetAsync(sh.p, 0, nsh * 8, st));
    return LGC_OK;
}
// and those words to the caller, the stream run dry; host words of a 32-bit run masked
static int shares_out(hipStream_t st, bool dev_io, const DevBuf &sh, uint64_t nsh, int width, uint64_t *shares) {
    OTCHK(hipMemcpyAsync(shares, sh.p, nsh * 8, dev_io ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    OTCHK(hipStreamSynchronize(st));
    if (width == 32 && !dev_io) for (uint64_t q = 0; q < nsh; q++) shares[q] &= 0xffffffffull;
    return LGC_OK;
}
// A receive of `kind` on the nw operand words a (arguments checked): a slot, the words staged for it with their bits packed as the
// choice bits, the extension.  The slot keeps npairs and n for the finish; every OT moves the tweak counter on by tweaks_per_ot.
static int recv_start_words(lgc_ot_receiver *r, const uint64_t *a, uint64_t nw, int width, uint64_t npairs, uint64_t n, int kind,
                            uint64_t tweaks_per_ot, uint8_t *u_out) {
    std::lock_guard<std::mutex> lock(r->mu);
    if (!r->st && lgc_stream_take(r->device, &r->st) != hipSuccess) return lgc_fail(LGC_EHIP, "hipStreamCreate failed");
    lgc_ot_receiver::Slot *sl = slot_push(r);
    if (!sl) return lgc_fail(LGC_ESTATE, "too many receives in flight (%zu)", r->count);
    Undo undo = {r, true};
    OTCHK(hipSetDevice(r->device));
    const uint64_t m = nw * (uint64_t)width, m128 = round128(m) / 128;
    const void *da;
    int rc = stage(r->st, r->dev_io, sl->avals, a, nw * 8, true, &da);
    if (rc) return rc;
    sl->avals_dev = static_cast<const uint64_t *>(da);
    OTCHK(sl->cbits.ensure(m128 * 16));
    OTCHK(hipMemsetAsync(sl->cbits.p, 0, m128 * 16, r->st));
    hipLaunchKernelGGL(ot_pack_choice_words_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, r->st, sl->avals_dev, nw, width,
                       (uint64_t *)sl->cbits.p);
    OTLAUNCH();
    sl->m = m; sl->npairs = npairs; sl->n = n; sl->w = width; sl->tweak_cur = r->tweak; sl->kind = kind;
    rc = recv_extend(r, sl, m, u_out);
    if (rc) return rc;
    r->tweak += m * tweaks_per_ot;
    undo.armed = false;
    return LGC_OK;
}
extern "C" int lgc_ot_gilboa_recv_start(lgc_ot_receiver *r, const uint64_t *a, size_t npairs, size_t n, int width, uint8_t *u_out) {
    if (!r || !a || !u_out) return lgc_fail(LGC_EINVAL, "null argument");
    if (width != 32 && width != 64) return lgc_fail(LGC_EINVAL, "width must be 32 or 64");
    return recv_start_words(r, a, (uint64_t)npairs * n, width, npairs, n, kSlotGilboa, 1, u_out);
}
extern "C" int lgc_ot_gilboa_send(lgc_ot_sender *s, const uint64_t *b, size_t npairs, size_t n, int width, const uint8_t *u_in,
                                  uint64_t *y_out, uint64_t *shares) {
    if (!s || !b || !u_in || !y_out || !shares) return lgc_fail(LGC_EINVAL, "null argument");
    if (width != 32 && width != 64) return lgc_fail(LGC_EINVAL, "width must be 32 or 64");
    OTCHK(hipSetDevice(s->device));
    if (!s->st && lgc_stream_take(s->device, &s->st) != hipSuccess) return lgc_fail(LGC_EHIP, "hipStreamCreate failed");
    const uint64_t nw = (uint64_t)npairs * n, m = nw * (uint64_t)width, mpp = (uint64_t)n * width;
    int rc = send_extend(s, m, u_in);
    if (rc) return rc;
    const void *db, *dy;
    if ((rc = stage(s->st, s->dev_io, s->b, b, nw * 8, true, &db)) || (rc = stage(s->st, s->dev_io, s->y, y_out, m * 8, false, &dy)) ||
        (rc = shares_zero(s->st, s->sh, npairs)))
        return rc;
    unsigned gx, gy;
    ot_pair_grid(mpp, npairs, gx, gy);
    hipLaunchKernelGGL(ot_gilboa_send_kernel, dim3(gx, gy), dim3(1024), 0, s->st, (const uint4 *)s->rows.p, s->delta, (const uint64_t *)db,
                       (uint64_t)n, width, mpp, (uint64_t)npairs, s->tweak, (uint64_t *)dy, (uint64_t *)s->sh.p);
    OTLAUNCH();
    if (!s->dev_io) OTCHK(hipMemcpyAsync(y_out, dy, m * 8, hipMemcpyDeviceToHost, s->st));
    rc = shares_out(s->st, s->dev_io, s->sh, npairs, width, shares);
    if (rc) return rc;
    s->tweak += m;
    return LGC_OK;
}
extern "C" int lgc_ot_gilboa_recv_finish(lgc_ot_receiver *r, const uint64_t *y_in, uint64_t *shares) {
    if (!r || !y_in || !shares) return lgc_fail(LGC_EINVAL, "null argument");
    std::lock_guard<std::mutex> lock(r->mu);
    lgc_ot_receiver::Slot *sl = slot_front(r);
    if (!sl || sl->kind != kSlotGilboa) return lgc_fail(LGC_ESTATE, "no Gilboa receive in flight");
    Pop pop = {r};
    OTCHK(hipSetDevice(r->device));
    const void *dy;
    int rc = stage(r->st, r->dev_io, r->y, y_in, sl->m * 8, true, &dy);
    if (!rc) rc = shares_zero(r->st, r->sh, sl->npairs);
    if (rc) return rc;
    const uint64_t mpp = sl->n * (uint64_t)sl->w;
    unsigned gx, gy;
    ot_pair_grid(mpp, sl->npairs, gx, gy);
    hipLaunchKernelGGL(ot_gilboa_recv_kernel, dim3(gx, gy), dim3(1024), 0, r->st, (const uint4 *)sl->rows.p, sl->avals_dev, sl->n, sl->w,
                       mpp, sl->npairs, sl->tweak_cur, (const uint64_t *)dy, (uint64_t *)r->sh.p);
    OTLAUNCH();
    return shares_out(r->st, r->dev_io, r->sh, sl->npairs, sl->w, shares);
}

// ---------------------------------------------------------------- Gilboa on a whole block, one vector OT per operand bit
// The matrix form (linreg_gc_ot_matrix.h) and the half-payload form (linreg_gc_ot_half.h) are one path: the same OTs, choice bits,
// extension, pads, tweaks, slots and share block.  A form is what differs: the unit of a lane's walk (unit_ots OTs of one
// (k, ir): a single OT, or the pair that fills the same words of the half y), how many units a lane takes per trip, and the words
// of y per (k, ir, j), W / unit_ots + y_extra -- beside the arithmetic of its two kernels.
enum OtForm { kFormMatrix = 0, kFormHalf = 1 };
struct OtFormDesc {
    int slot;                  // kSlot*: a finish must be of the form of the oldest start
    int unit_ots, per_trip, y_extra;
    const char *noun;          // in the LGC_ESTATE message
};
static const OtFormDesc kOtForms[2] = {{kSlotMatrix, 1, 2, 0, "matrix"}, {kSlotHalf, 2, 1, 1, "half-payload"}};

// rows r (words of y per (k, ir, j)) s W / 8, or 0 when that does not fit 63 bits
static size_t ot_block_y_bytes(OtForm form, size_t rows, size_t r, size_t s, int width) {
    if (width != 32 && width != 64) return 0;
    const OtFormDesc &f = kOtForms[form];
    uint64_t v = rows;
    const uint64_t fac[4] = {r, (uint64_t)(width / f.unit_ots + f.y_extra), s, (uint64_t)(width / 8)};
    for (int k = 0; k < 4; k++)
        if (__builtin_mul_overflow(v, fac[k], &v)) return 0;
    return v >> 63 ? 0 : (size_t)v;
}
// Launch geometry of the payload kernels.  A wave is one chunk of 64 slots on one slice of the kb = rows * W / unit_ots units; a
// workgroup is 16 waves.  ks = ceil(kb / per_trip) slices give every lane one trip; more than 16 kOtGroups / nsc slices would be
// more than kOtGroups workgroups, so beyond that the lanes take further trips.  Only a block of more than 16 kOtGroups chunks
// (r * nblk > 524 288 slots) launches more workgroups than kOtGroups: one wave per chunk.
static int ot_block_geom(OtForm form, size_t rows, size_t r, size_t s, int width, OtMatrixGeom *g, unsigned *gx) {
    if (width != 32 && width != 64) return lgc_fail(LGC_EINVAL, "width must be 32 or 64");
    if (!rows || !r || !s) return lgc_fail(LGC_EINVAL, "empty block (rows, r and s must be positive)");
    const uint64_t lim = 1ull << 32;
    if (rows >= lim || r >= lim || s >= lim || (uint64_t)rows * r >= lim / width) return lgc_fail(LGC_EINVAL, "batch of 2^32 OTs or more");
    const uint64_t nblk = ((uint64_t)s * width + 127) / 128, nslot = (uint64_t)r * nblk;
    if (nslot >= (1ull << 31)) return lgc_fail(LGC_EINVAL, "block too wide (r * ceil(s W / 128) must be below 2^31)");
    if (!ot_block_y_bytes(form, rows, r, s, width)) return lgc_fail(LGC_EINVAL, "y of 2^63 bytes or more");
    const OtFormDesc &f = kOtForms[form];
    g->r = (uint32_t)r; g->s = (uint32_t)s; g->nblk = (uint32_t)nblk; g->nslot = (uint32_t)nslot;
    g->nsc = (uint32_t)((nslot + 63) / 64);
    g->kb = (uint64_t)rows * (width / f.unit_ots);
    const uint64_t waves = 16ull * kOtGroups, cap = waves / g->nsc ? waves / g->nsc : 1, want = (g->kb + f.per_trip - 1) / f.per_trip;
    g->ks = (uint32_t)(want < cap ? want : cap);
    g->vec = ((uint64_t)s * width) % 128 == 0;        // (the caller clears it for a y that is not 16-byte aligned)
    *gx = (unsigned)(((uint64_t)g->nsc * g->ks + 15) / 16);
    return LGC_OK;
}
// the one place that picks a payload kernel: by form, role and width.  x is the role's operand and delta the sender's; the receive
// kernels only read y
template <int W>
static void ot_block_launch_w(OtForm form, bool send, unsigned gx, hipStream_t st, const uint4 *rows, uint4 delta, const uint64_t *x,
                              const OtMatrixGeom &g, uint64_t tweak0, void *y, uint64_t *sh) {
    typedef typename OtWord<W>::T word;
    if (send) {
        auto kern = form == kFormHalf ? ot_gilboa_half_send_kernel<W> : ot_gilboa_matrix_send_kernel<W>;
        hipLaunchKernelGGL(kern, dim3(gx), dim3(1024), 0, st, rows, delta, x, g, tweak0, (word *)y, sh);
    } else {
        auto kern = form == kFormHalf ? ot_gilboa_half_recv_kernel<W> : ot_gilboa_matrix_recv_kernel<W>;
        hipLaunchKernelGGL(kern, dim3(gx), dim3(1024), 0, st, rows, x, g, tweak0, (const word *)y, sh);
    }
}
static void ot_block_launch(OtForm form, bool send, int width, unsigned gx, hipStream_t st, const uint4 *rows, uint4 delta, const uint64_t *x,
                            const OtMatrixGeom &g, uint64_t tweak0, void *y, uint64_t *sh) {
    if (width == 64) ot_block_launch_w<64>(form, send, gx, st, rows, delta, x, g, tweak0, y, sh);
    else ot_block_launch_w<32>(form, send, gx, st, rows, delta, x, g, tweak0, y, sh);
}
static int block_recv_start(OtForm form, lgc_ot_receiver *r, const uint64_t *xr, size_t rows, size_t nr, size_t ns, int width, uint8_t *u_out) {
    if (!r || !xr || !u_out) return lgc_fail(LGC_EINVAL, "null argument");
    OtMatrixGeom g;
    unsigned gx;
    int rc = ot_block_geom(form, rows, nr, ns, width, &g, &gx);
    if (rc) return rc;
    return recv_start_words(r, xr, (uint64_t)rows * nr, width, nr, ns, kOtForms[form].slot, g.nblk, u_out);   // the slot: npairs = r, n = s
}
static int block_send(OtForm form, lgc_ot_sender *s, const uint64_t *xs, size_t rows, size_t nr, size_t ns, int width, const uint8_t *u_in,
                      void *y_out, uint64_t *shares) {
    if (!s || !xs || !u_in || !y_out || !shares) return lgc_fail(LGC_EINVAL, "null argument");
    OtMatrixGeom g;
    unsigned gx;
    int rc = ot_block_geom(form, rows, nr, ns, width, &g, &gx);
    if (rc) return rc;
    if (s->dev_io && ((uintptr_t)y_out & 15)) g.vec = 0;
    OTCHK(hipSetDevice(s->device));
    if (!s->st && lgc_stream_take(s->device, &s->st) != hipSuccess) return lgc_fail(LGC_EHIP, "hipStreamCreate failed");
    const uint64_t m = (uint64_t)rows * nr * (uint64_t)width, nx = (uint64_t)rows * ns, nsh = (uint64_t)nr * ns;
    const size_t yb = ot_block_y_bytes(form, rows, nr, ns, width);
    rc = send_extend(s, m, u_in);
    if (rc) return rc;
    const void *dx, *dy;
    if ((rc = stage(s->st, s->dev_io, s->b, xs, nx * 8, true, &dx)) || (rc = stage(s->st, s->dev_io, s->y, y_out, yb, false, &dy)) ||
        (rc = shares_zero(s->st, s->sh, nsh)))
        return rc;
    ot_block_launch(form, true, width, gx, s->st, (const uint4 *)s->rows.p, s->delta, (const uint64_t *)dx, g, s->tweak, const_cast<void *>(dy),
                    (uint64_t *)s->sh.p);
    OTLAUNCH();
    if (!s->dev_io) OTCHK(hipMemcpyAsync(y_out, dy, yb, hipMemcpyDeviceToHost, s->st));
    rc = shares_out(s->st, s->dev_io, s->sh, nsh, width, shares);
    if (rc) return rc;
    s->tweak += m * g.nblk;
    return LGC_OK;
}
static int block_recv_finish(OtForm form, lgc_ot_receiver *r, const void *y_in, uint64_t *shares) {
    if (!r || !y_in || !shares) return lgc_fail(LGC_EINVAL, "null argument");
    std::lock_guard<std::mutex> lock(r->mu);
    lgc_ot_receiver::Slot *sl = slot_front(r);
    if (!sl || sl->kind != kOtForms[form].slot) return lgc_fail(LGC_ESTATE, "no %s Gilboa receive in flight", kOtForms[form].noun);
    Pop pop = {r};
    OTCHK(hipSetDevice(r->device));
    const size_t nr = sl->npairs, ns = sl->n, rows = sl->m / (nr * (uint64_t)sl->w);
    const void *dy;
    int rc = stage(r->st, r->dev_io, r->y, y_in, ot_block_y_bytes(form, rows, nr, ns, sl->w), true, &dy);
    if (rc) return rc;
    OtMatrixGeom g;
    unsigned gx;
    rc = ot_block_geom(form, rows, nr, ns, sl->w, &g, &gx);
    if (rc) return rc;
    if ((uintptr_t)dy & 15) g.vec = 0;
    const uint64_t nsh = (uint64_t)nr * ns;
    rc = shares_zero(r->st, r->sh, nsh);
    if (rc) return rc;
    ot_block_launch(form, false, sl->w, gx, r->st, (const uint4 *)sl->rows.p, make_uint4(0, 0, 0, 0), sl->avals_dev, g, sl->tweak_cur,
                    const_cast<void *>(dy), (uint64_t *)r->sh.p);
    OTLAUNCH();
    return shares_out(r->st, r->dev_io, r->sh, nsh, sl->w, shares);
}
extern "C" size_t lgc_ot_gilboa_matrix_y_bytes(size_t rows, size_t r, size_t s, int width) { return ot_block_y_bytes(kFormMatrix, rows, r, s, width); }
extern "C" int lgc_ot_gilboa_matrix_recv_start(lgc_ot_receiver *r, const uint64_t *xr, size_t rows, size_t nr, size_t ns, int width,
                                               uint8_t *u_out) { return block_recv_start(kFormMatrix, r, xr, rows, nr, ns, width, u_out); }
extern "C" int lgc_ot_gilboa_matrix_send(lgc_ot_sender *s, const uint64_t *xs, size_t rows, size_t nr, size_t ns, int width,
                                         const uint8_t *u_in, void *y_out, uint64_t *shares) { return block_send(kFormMatrix, s, xs, rows, nr, ns, width, u_in, y_out, shares); }
extern "C" int lgc_ot_gilboa_matrix_recv_finish(lgc_ot_receiver *r, const void *y_in, uint64_t *shares) { return block_recv_finish(kFormMatrix, r, y_in, shares); }
// ---- Gilboa, half payload (linreg_gc_ot_half.h)
extern "C" size_t lgc_ot_gilboa_half_y_bytes(size_t rows, size_t r, size_t s, int width) { return ot_block_y_bytes(kFormHalf, rows, r, s, width); }
extern "C" int lgc_ot_gilboa_half_recv_start(lgc_ot_receiver *r, const uint64_t *xr, size_t rows, size_t nr, size_t ns, int width,
                                             uint8_t *u_out) { return block_recv_start(kFormHalf, r, xr, rows, nr, ns, width, u_out); }
extern "C" int lgc_ot_gilboa_half_send(lgc_ot_sender *s, const uint64_t *xs, size_t rows, size_t nr, size_t ns, int width,
                                       const uint8_t *u_in, void *y_out, uint64_t *shares) { return block_send(kFormHalf, s, xs, rows, nr, ns, width, u_in, y_out, shares); }
extern "C" int lgc_ot_gilboa_half_recv_finish(lgc_ot_receiver *r, const void *y_in, uint64_t *shares) { return block_recv_finish(kFormHalf, r, y_in, shares); }

// ---------------------------------------------------------------- labels
// choice: m bytes, one per OT (the reference's bool* sel, src/input.c:40-44)
extern "C" int lgc_ot_labels_recv_start(lgc_ot_receiver *r, const uint8_t *choice, size_t m, uint8_t *u_out) {
    if (!r || !choice || !u_out) return lgc_fail(LGC_EINVAL, "null argument");
    std::lock_guard<std::mutex> lock(r->mu);
    lgc_ot_receiver::Slot *sl = slot_push(r);
    if (!sl) return lgc_fail(LGC_ESTATE, "too many receives in flight (%zu)", r->count);
    Undo undo = {r, true};
    OTCHK(hipSetDevice(r->device));
    const uint64_t m128 = round128(m) / 128;
    const uint8_t *dc = choice;
    if (!r->dev_io) {
        OTCHK(r->choice.ensure(m));
        OTCHK(hipMemcpyAsync(r->choice.p, choice, m, hipMemcpyHostToDevice, r->st));
        dc = static_cast<const uint8_t *>(r->choice.p);
    }
    OTCHK(sl->cbits.ensure(m128 * 16));
    const uint64_t nwords = m128 * 2;
    hipLaunchKernelGGL(ot_pack_choice_bytes_kernel, dim3((unsigned)((nwords * 64 + 255) / 256)), dim3(256), 0, r->st, dc, (uint64_t)m,
                       (uint64_t *)sl->cbits.p, nwords);
    OTLAUNCH();
    sl->m = m; sl->npairs = 0; sl->n = 0; sl->w = 0; sl->tweak_cur = r->tweak; sl->kind = kSlotLabels; sl->avals_dev = 0;
    int rc = recv_extend(r, sl, m, u_out);
    if (rc) return rc;
    r->tweak += m;
    undo.armed = false;
    return LGC_OK;
}
extern "C" int lgc_ot_labels_send(lgc_ot_sender *s, const uint8_t *msg0, const uint8_t *msg1, size_t m, const uint8_t *u_in, uint8_t *e_out) {
    if (!s || !msg0 || !msg1 || !u_in || !e_out) return lgc_fail(LGC_EINVAL, "null argument");
    OTCHK(hipSetDevice(s->device));
    int rc = send_extend(s, m, u_in);
    if (rc) return rc;
    const uint4 *d0 = reinterpret_cast<const uint4 *>(msg0), *d1 = reinterpret_cast<const uint4 *>(msg1);
    uint4 *de = reinterpret_cast<uint4 *>(e_out);
    if (!s->dev_io) {
        OTCHK(s->m0.ensure(m * 16)); OTCHK(s->m1.ensure(m * 16)); OTCHK(s->e.ensure(m * 32));
        OTCHK(hipMemcpyAsync(s->m0.p, msg0, m * 16, hipMemcpyHostToDevice, s->st));
        OTCHK(hipMemcpyAsync(s->m1.p, msg1, m * 16, hipMemcpyHostToDevice, s->st));
        d0 = (const uint4 *)s->m0.p; d1 = (const uint4 *)s->m1.p; de = (uint4 *)s->e.p;
    }
    unsigned gx = (unsigned)((m + 2047) / 2048); if (gx > kOtGroups) gx = kOtGroups;
    hipLaunchKernelGGL(ot_labels_send_kernel, dim3(gx), dim3(1024), 0, s->st, (const uint4 *)s->rows.p, s->delta, d0, d1, (uint64_t)m,
                       s->tweak, de);
    OTLAUNCH();
    if (!s->dev_io) OTCHK(hipMemcpyAsync(e_out, de, m * 32, hipMemcpyDeviceToHost, s->st));
    OTCHK(hipStreamSynchronize(s->st));
    s->tweak += m;
    return LGC_OK;
}
extern "C" int lgc_ot_labels_recv_finish(lgc_ot_receiver *r, const uint8_t *e_in, uint8_t *out) {
    if (!r || !e_in || !out) return lgc_fail(LGC_EINVAL, "null argument");
    std::lock_guard<std::mutex> lock(r->mu);
    lgc_ot_receiver::Slot *sl = slot_front(r);
    if (!sl || sl->kind != kSlotLabels) return lgc_fail(LGC_ESTATE, "no label receive in flight");
    Pop pop = {r};
    OTCHK(hipSetDevice(r->device));
    const uint4 *de = reinterpret_cast<const uint4 *>(e_in);
    uint4 *dout = reinterpret_cast<uint4 *>(out);
    if (!r->dev_io) {
        OTCHK(r->e.ensure(sl->m * 32)); OTCHK(r->out.ensure(sl->m * 16));
        OTCHK(hipMemcpyAsync(r->e.p, e_in, sl->m * 32, hipMemcpyHostToDevice, r->st));
        de = (const uint4 *)r->e.p; dout = (uint4 *)r->out.p;
    }
    unsigned gx = (unsigned)((sl->m + 2047) / 2048); if (gx > kOtGroups) gx = kOtGroups;
    hipLaunchKernelGGL(ot_labels_recv_kernel, dim3(gx), dim3(1024), 0, r->st, (const uint4 *)sl->rows.p, (const uint64_t *)sl->cbits.p, de,
                       sl->m, sl->tweak_cur, dout);
    OTLAUNCH();
    if (!r->dev_io) OTCHK(hipMemcpyAsync(out, dout, sl->m * 16, hipMemcpyDeviceToHost, r->st));
    OTCHK(hipStreamSynchronize(r->st));
    return LGC_OK;
}
