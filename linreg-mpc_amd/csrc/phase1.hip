// phase1.hip -- phase-1 aggregation on the MI355X: additive shares of X^T X and
// X^T y in the ring Z_2^w (w = 32 or 64).
//
// Replaces the arithmetic of the reference's src/phase1.c:
//   inner_product_local (14-20)            -> p1_tile_mac, the one LDS-tiled wrap-around u64 body, under two tiled kernels:
//                                             p1_gram_folds_kernel (Gram blocks of row ranges), p1_rect_kernel (X^T Y);
//                                             p1_scan_kernel (tall-skinny, one column per thread) has a shape of its own;
//                                             p1_cross_kernel: the same body on two matrices (matrix-triple mode)
//   diagonal special case (562-567, 364-369)-> p1_diag_kernel  (IEEE double, k ascending, no FMA)
//   run_trusted_initializer PRG + <x,y> (241-287) -> ti_prg_kernel (AES-128-CTR) + p1_dot_kernel
//   inner_product_ti masking / shares (148-236)   -> p1_mask_kernel, p1_dot_kernel
// The transport (TCP mesh, length-prefixed protobuf messages, phase1.c:100-145) stays on
// the host and is out of scope here; these entry points take and return host buffers.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/linreg_gc.h"
#include "../../include/linreg_gc_sweep.h"
#include "../../include/linreg_gc_debug.h"
#include "../../include/linreg_gc_targets.h"
#include "../../include/linreg_gc_folds.h"
#include "../../include/linreg_gc_folds_yy.h"
#include "../../include/linreg_gc_inference.h"
#include "../../include/linreg_gc_scan.h"
#include "../../include/linreg_gc_p1_matrix.h"
#include "hip_scope.h"
#include "gc_device.h"

using namespace gc;

int lgc_fail(int code, const char *fmt, ...);
int lgc_need_device(int device);
__global__ void p1_tu_touch_kernel() {}
hipError_t p1_tu_touch(hipStream_t st) { hipLaunchKernelGGL(p1_tu_touch_kernel, dim3(1), dim3(64), 0, st); return hipGetLastError(); }

#define P1CHK(x)                                                                             \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess) return lgc_fail(LGC_EHIP, "%s: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

struct lgc_p1 {
    int device, w, p;
    size_t n, d;     // n: rows of the current window (lgc_p1_set_rows), all rows on a fresh object
    size_t k;        // target columns after X: 1 (y) from lgc_p1_create, k from lgc_p1_create_targets
    int64_t *X;      // n x (d + k) row-major, column d + t = target t (zero when this party does not own it): row 0 of the window
    size_t n_all;    // the rows the object was created with, and
    int64_t *X_all;  // the allocation: X = X_all + r0 * ld(), n = r1 - r0
    bool have_y;
    size_t ld() const { return d + k; }
    bool dev_io;     // lgc_p1_set_device_io: the vector arguments of mask / dot / ti_a_batch are device memory
    size_t divisor;  // of the floating-point diagonal: d unless lgc_p1_set_divisor changed it (linreg_gc_scan.h)
};

// ---- the tile body of the three tiled kernels below.  A workgroup of 256 threads owns a 64 x 64 output tile, a thread 4 x 4 of
// it: acc[u][v] += sum over rows k0 <= k < k1 of A[k][ty * 4 + u] * B[k][tx * 4 + v]  (mod 2^64), A and B being the 64 columns
// on the tile's row side and on its column side, staged through LDS in slabs of 16 rows.  Each side is a row-major matrix of its
// own: a base, a leading dimension and a word type (int64_t for X; uint32_t / uint64_t for a keystream or a block in wire
// form, zero-extended).  The Gram and rect kernels pass X twice.  Loader: thread t brings in column t % 64 of each side
// (column ca of PA for A if la, cb of PB for B if lb, zeros otherwise), rows t / 64 + 0, 4, 8, 12 of a slab.
#define P1_KT 16
template <typename TA, typename TB>
__device__ __forceinline__ void p1_tile_mac(const TA *PA, size_t lda, const TB *PB, size_t ldb, size_t k0, size_t k1, bool la, size_t ca,
                                            bool lb, size_t cb, uint64_t (&acc)[4][4]) {
    __shared__ uint64_t As[P1_KT][64], Bs[P1_KT][64];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int lc = threadIdx.x & 63, lr = threadIdx.x >> 6;   // loader: 4 rows x 64 columns per pass
    for (size_t kb = k0; kb < k1; kb += P1_KT) {
#pragma unroll
        for (int r = 0; r < P1_KT; r += 4) {
            size_t k = kb + r + lr;
            As[r + lr][lc] = (k < k1 && la) ? (uint64_t)PA[k * lda + ca] : 0;
            Bs[r + lr][lc] = (k < k1 && lb) ? (uint64_t)PB[k * ldb + cb] : 0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < P1_KT; kk++) {
            uint64_t a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { a[u] = As[kk][ty * 4 + u]; b[u] = Bs[kk][tx * 4 + u]; }
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int v = 0; v < 4; v++) acc[u][v] += a[u] * b[v];
        }
        __syncthreads();
    }
}

// ---- wrap-around Gram blocks: C[f][a][b] = sum over the rows k of range f of X[k][cols[a]] * X[k][cols[b]]  (mod 2^64), the
// lower triangle only.  blockIdx.z walks a table of row ranges, each inside ONE output block (a split never straddles a block
// boundary), and the partial sums of a range go with integer atomics into that block's L x L words: exact and
// order-independent.  The whole window is a table over one block; K row folds are a table over K.
struct P1FoldSplit { unsigned long long k0, k1; uint32_t fold, pad; };
__global__ void __launch_bounds__(256)
p1_gram_folds_kernel(const int64_t *X, size_t ld, const uint32_t *cols, uint32_t L, uint64_t *C, const P1FoldSplit *splits) {
    const uint32_t i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    if (j0 > i0) return;   // lower triangle of tiles only
    const P1FoldSplit sp = splits[blockIdx.z];
    uint64_t *Cf = C + (size_t)sp.fold * L * L;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, lc = threadIdx.x & 63;
    const bool la = i0 + lc < L, lb = j0 + lc < L;
    uint64_t acc[4][4] = {};
    p1_tile_mac(X, ld, X, ld, sp.k0, sp.k1, la, la ? cols[i0 + lc] : 0, lb, lb ? cols[j0 + lc] : 0, acc);
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int v = 0; v < 4; v++) {
            uint32_t i = i0 + ty * 4 + u, j = j0 + tx * 4 + v;
            if (i < L && j < L && j <= i) atomicAdd((unsigned long long *)&Cf[(size_t)i * L + j], (unsigned long long)acc[u][v]);
        }
}

// ---- wrap-around rectangular block: C[t][i] = sum_k X[k][c0 + i] * X[k][y0 + t]  (mod 2^64), i < own, t < nt, over the
// own x target tiles only: the targets x targets triangle that a Gram block over own + k columns would also form is never
// computed.  blockIdx.z is the split of K, its partial sums combined with integer atomics.
__global__ void __launch_bounds__(256)
p1_rect_kernel(const int64_t *X, size_t n, size_t ld, uint32_t c0, uint32_t own, uint32_t y0, uint32_t nt, uint64_t *C,
               size_t kchunk) {
    const uint32_t i0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
    const size_t k0 = (size_t)blockIdx.z * kchunk;
    const size_t k1 = k0 + kchunk < n ? k0 + kchunk : n;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, lc = threadIdx.x & 63;
    uint64_t acc[4][4] = {};
    p1_tile_mac(X, ld, X, ld, k0, k1, i0 + lc < own, (size_t)c0 + i0 + lc, j0 + lc < nt, (size_t)y0 + j0 + lc, acc);
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int v = 0; v < 4; v++) {
            uint32_t i = i0 + ty * 4 + u, t = j0 + tx * 4 + v;
            if (i < own && t < nt) atomicAdd((unsigned long long *)&C[(size_t)t * own + i], (unsigned long long)acc[u][v]);
        }
}

// ---- wrap-around cross product of two column blocks (matrix-triple mode, linreg_gc_p1_matrix.h):
// C[i][j] += sum_k P[k][i] * Q[k][j]  (mod 2^64), i < a, j < b, over rows [0, n).  A side is a dense row-major matrix (cols ==
// NULL: column i is word i of a row of ld words) or columns of it picked by an index list (X and the columns a provider owns).
// One workgroup per 64 x 64 tile and split of K (blockIdx.z); partial sums go into C with integer atomics.
template <typename TP, typename TQ>
__global__ void __launch_bounds__(256)
p1_cross_kernel(const TP *P, size_t ldp, const uint32_t *pcols, uint32_t a, const TQ *Q, size_t ldq, const uint32_t *qcols, uint32_t b,
                size_t n, uint64_t *C, size_t kchunk) {
    const uint32_t i0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
    const size_t k0 = (size_t)blockIdx.z * kchunk;
    const size_t k1 = k0 + kchunk < n ? k0 + kchunk : n;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, lc = threadIdx.x & 63;
    const bool la = i0 + lc < a, lb = j0 + lc < b;
    const size_t ca = la ? (pcols ? pcols[i0 + lc] : i0 + lc) : 0, cb = lb ? (qcols ? qcols[j0 + lc] : j0 + lc) : 0;
    uint64_t acc[4][4] = {};
    p1_tile_mac(P, ldp, Q, ldq, k0, k1, la, ca, lb, cb, acc);
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int v = 0; v < 4; v++) {
            uint32_t i = i0 + ty * 4 + u, j = j0 + tx * 4 + v;
            if (i < a && j < b) atomicAdd((unsigned long long *)&C[(size_t)i * b + j], (unsigned long long)acc[u][v]);
        }
}
// out[t] = (C[t] + add[t]) & m  (sign > 0: a share takes S or T in) or (C[t] - add[t]) & m  (the initializer's T), t < count
template <typename TW, typename TO>
__global__ void p1_cross_finish_kernel(const uint64_t *C, const TW *add, int sign, size_t count, uint64_t m, TO *out) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (size_t)gridDim.x * blockDim.x) {
        const uint64_t c = C[t], s = (uint64_t)add[t];
        out[t] = (TO)((sign > 0 ? c + s : c - s) & m);
    }
}
// the masked block: E[k][i] = (X[k][cols[i]] - R[k][i]) & m in wire form, R the n x ncols keystream words
template <typename TW>
__global__ void p1_matrix_mask_kernel(const int64_t *X, size_t n, size_t ld, const uint32_t *cols, uint32_t ncols, const TW *R, TW *E,
                                      uint64_t m) {
    const size_t total = n * ncols;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t k = t / ncols;
        const uint32_t i = (uint32_t)(t - k * ncols);
        E[t] = (TW)(((uint64_t)X[k * ld + cols[i]] - (uint64_t)R[t]) & m);
    }
}

// ---- tall-skinny block of an association scan (linreg_gc_scan.h): C[m][z0 + q] = sum_k X[k][s0 + m] * Z[k][z0 + q]  (mod 2^64),
// m < ns candidate columns, Z = [the nc own covariate columns from c0, then column ycol] of nz columns, q < NZ (a pass of at
// most 32 of them; NZ is the pass width rounded up to a power of two, the surplus columns are zero).  A workgroup owns 256
// consecutive candidate columns and a range of rows; a thread owns ONE column and keeps its NZ sums in registers.  Z is staged
// through LDS in slabs of 16 rows and every lane reads the same word of it (a broadcast); the candidate block, the one large
// object, is read row by row, fully coalesced and exactly once per pass.  Split-K partial sums are combined with integer
// atomics (exact and order-independent), as in the kernels above.
template <int NZ>
__global__ void __launch_bounds__(256)
p1_scan_kernel(const int64_t *X, size_t n, size_t ld, uint32_t s0, uint32_t ns, uint32_t c0, uint32_t nc, uint32_t ycol,
               uint32_t z0, uint32_t nz, uint64_t *C, size_t kchunk) {
    __shared__ uint64_t Zs[P1_KT][NZ];
    const uint32_t m = blockIdx.x * 256 + threadIdx.x;
    const bool live = m < ns;
    const size_t k0 = (size_t)blockIdx.y * kchunk;
    const size_t k1 = k0 + kchunk < n ? k0 + kchunk : n;
    const int64_t *G = X + s0 + (live ? m : 0);
    uint64_t acc[NZ] = {};
    for (size_t kb = k0; kb < k1; kb += P1_KT) {
        for (int t = threadIdx.x; t < P1_KT * NZ; t += 256) {
            const int r = t / NZ, q = t % NZ;
            const size_t k = kb + r;
            const uint32_t gq = z0 + q;
            Zs[r][q] = (k < k1 && gq < nz) ? (uint64_t)X[k * ld + (gq < nc ? c0 + gq : ycol)] : 0;
        }
        uint64_t g[P1_KT];
#pragma unroll
        for (int kk = 0; kk < P1_KT; kk++) g[kk] = (live && kb + kk < k1) ? (uint64_t)G[(kb + kk) * ld] : 0;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < P1_KT; kk++)
#pragma unroll
            for (int q = 0; q < NZ; q++) acc[q] += g[kk] * Zs[kk][q];
        __syncthreads();
    }
    if (!live) return;
#pragma unroll
    for (int q = 0; q < NZ; q++)
        if (z0 + q < nz) atomicAdd((unsigned long long *)&C[(size_t)m * nz + z0 + q], (unsigned long long)acc[q]);
}

// ---- diagonal: xy += pow(fixed_to_double(x_k, p), 2) * pow(2, p), k ascending, in IEEE double;
// share = double_to_fixed(xy / d, p)  (src/phase1.c:562-567).  Explicit round-to-nearest
// multiplies/adds so that no FMA contraction can change the rounding.  Only the additions are
// order-dependent: a workgroup owns 16 columns; 15 loader waves compute the terms of a 600-row
// chunk in parallel into LDS while wave 0 adds the previous chunk's terms in k order (the bound
// is n dependent double additions per column).
#define P1_DC 16        /* columns per workgroup */
#define P1_DR 600       /* rows per chunk: 15 waves x 4 row phases x 10 rows */
__global__ void __launch_bounds__(1024)
p1_diag_kernel(const int64_t *X, size_t n, size_t ld, const uint32_t *cols, uint32_t L,
               int p, int w, double normalizer2, uint64_t *out) {
    __shared__ double term[2][P1_DR][P1_DC];      // 150 KiB
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t t = blockIdx.x * P1_DC + (lane & 15);
    const bool live = t < L;
    const uint32_t c = live ? cols[t] : 0;
    const double scale = (double)(1ll << p);
    const size_t nchunks = (n + P1_DR - 1) / P1_DR;
    double xy = 0.0;
    for (size_t ch = 0; ch <= nchunks; ch++) {
        if (wave > 0 && ch < nchunks) {             // loaders: chunk ch -> term[ch & 1]
            const size_t k0 = ch * P1_DR;
            const int r0 = (wave - 1) * 4 + (lane >> 4);          // 0..59
            int64_t x[10];
#pragma unroll
            for (int u = 0; u < 10; u++) {
                size_t k = k0 + (size_t)(r0 + 60 * u);
                x[u] = (live && k < n) ? X[k * ld + c] : 0;
            }
#pragma unroll
            for (int u = 0; u < 10; u++) {
                double v = __ddiv_rn((double)x[u], scale);
                term[ch & 1][r0 + 60 * u][lane & 15] = __dmul_rn(__dmul_rn(v, v), scale);
            }
        }
        if (wave == 0 && ch > 0 && lane < P1_DC) {  // adder: chunk ch - 1, rows in k order
            const size_t k0 = (ch - 1) * P1_DR;
            const int rows = (int)((n - k0 < (size_t)P1_DR) ? n - k0 : (size_t)P1_DR);
            const double *tp = &term[(ch - 1) & 1][0][lane];
            for (int r = 0; r < rows; r++) xy = __dadd_rn(xy, tp[r * P1_DC]);
        }
        __syncthreads();
    }
    if (wave != 0 || lane >= P1_DC || !live) return;
    double tq = __dmul_rn(__ddiv_rn(xy, normalizer2), scale);
    uint64_t r;
    if (w == 32) {   // (int32_t) cast with the x86 "integer indefinite" result when out of range
        if (!(tq > -2147483649.0 && tq < 2147483648.0)) r = 0x80000000ull;
        else r = (uint64_t)(uint32_t)(int32_t)tq;
    } else {
        if (!(tq >= -9223372036854775808.0 && tq < 9223372036854775808.0)) r = 0x8000000000000000ull;
        else r = (uint64_t)(int64_t)tq;
    }
    out[t] = r;
}

// ---- batched masking: out[q][k] = X[k][col[q]] + sign * V[q][k]   (mod 2^64)
// m = 2^w - 1: the message is truncated to the protocol width HERE, so that a buffer another party maps (--ti_ring)
// never holds bits 32..63 of X +- v at w = 32 (X is stored sign-extended)
__global__ void p1_mask_kernel(const int64_t *X, size_t n, size_t ld, const uint32_t *cols, const uint64_t *V,
                               int sign, uint64_t *out, uint64_t m) {
    const uint32_t q = blockIdx.y;
    const uint32_t c = cols[q];
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
        uint64_t x = (uint64_t)X[k * ld + c], v = V[(size_t)q * n + k];
        out[(size_t)q * n + k] = (sign > 0 ? x + v : x - v) & m;
    }
}

// ---- single-pair forms used by the per-pair TI protocol: no column-index upload, the sum lands
// next to the vector it belongs to (one copy back); up to 64 workgroups keep the strided column
// reads in flight (a single workgroup was latency-bound: config 4 went from 90 s to 105 s)
__device__ __forceinline__ uint64_t p1_block_sum(uint64_t acc) {
    __shared__ uint64_t part[16];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    uint64_t t = 0;
    if (threadIdx.x == 0) for (unsigned i = 0; i < (blockDim.x + 63) / 64; i++) t += part[i];
    return t;   // valid in thread 0
}
// out[k] = X[k][col] + sign * V[k]
__global__ void __launch_bounds__(1024)
p1_mask1_kernel(const int64_t *X, size_t n, size_t ld, uint32_t col, const uint64_t *V, int sign, uint64_t *out, uint64_t m) {
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
        uint64_t x = (uint64_t)X[k * ld + col], v = V[k];
        out[k] = (sign > 0 ? x + v : x - v) & m;
    }
}
// out[0] = sum_k A[k] * (Bv ? Bv[k] : X[k][col])
__global__ void __launch_bounds__(1024)
p1_dot1_kernel(const uint64_t *A, const uint64_t *Bv, const int64_t *X, size_t ld, uint32_t col, size_t n, uint64_t *out) {
    uint64_t acc = 0;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x)
        acc += A[k] * (Bv ? Bv[k] : (uint64_t)X[k * ld + col]);
    uint64_t t = p1_block_sum(acc);
    if (threadIdx.x == 0) atomicAdd((unsigned long long *)&out[0], (unsigned long long)t);   // out[0] zeroed by the host
}
// party a of inner_product_ti in one pass (phase1.c:186-196): out[k] = a[k] - y[k] for k < n, and
// out[n] = sum_k in[k] * y[k]   (in = b + x from party b, y from the TI)
__global__ void __launch_bounds__(1024)
p1_ti_a_kernel(const int64_t *X, size_t n, size_t ld, uint32_t col, const uint64_t *y, const uint64_t *in, uint64_t *out, uint64_t m) {
    uint64_t acc = 0;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
        uint64_t yk = y[k];
        out[k] = ((uint64_t)X[k * ld + col] - yk) & m;
        acc += in[k] * yk;
    }
    uint64_t t = p1_block_sum(acc);
    if (threadIdx.x == 0) atomicAdd((unsigned long long *)&out[n], (unsigned long long)t);   // out[n] zeroed by the host
}

// the same for a run of pairs with one peer: grid.y strides over the pairs; acc[q] zeroed by the host
__global__ void __launch_bounds__(256)
p1_ti_a_batch_kernel(const int64_t *X, size_t n, size_t ld, const uint32_t *cols, size_t npairs, const uint64_t *y, const uint64_t *in,
                     uint64_t *out, uint64_t *acc_out, uint64_t m) {
    for (size_t q = blockIdx.y; q < npairs; q += gridDim.y) {
        const uint32_t col = cols[q];
        uint64_t acc = 0;
        for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
            uint64_t yk = y[q * n + k];
            out[q * n + k] = ((uint64_t)X[k * ld + col] - yk) & m;
            acc += in[q * n + k] * yk;
        }
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd((unsigned long long *)&acc_out[q], (unsigned long long)acc);
    }
}

// ---- batched wrap-around dot products: out[q] = sum_k A[q][k] * B[q][k]; B is either a vector
// batch (colsB == NULL) or columns of X
__global__ void __launch_bounds__(256)
p1_dot_kernel(const uint64_t *A, const uint64_t *Bv, const int64_t *X, size_t ld, const uint32_t *colsB, size_t n,
              uint64_t *out) {
    const uint32_t q = blockIdx.y;
    uint64_t acc = 0;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
        uint64_t a = A[(size_t)q * n + k];
        uint64_t b = colsB ? (uint64_t)X[k * ld + colsB[q]] : Bv[(size_t)q * n + k];
        acc += a * b;
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd((unsigned long long *)&out[q], (unsigned long long)acc);
}

// ---- AES-128-CTR keystream: block c = AES_k(c) (little-endian 128-bit counter, nonce 0).
// rk: 44 round-key words of the session key.  One block per lane per iteration.
__global__ void __launch_bounds__(1024)
ti_prg_kernel(const uint32_t *rk, uint64_t first_block, uint64_t nblocks, uint4 *out) {
    __shared__ uint32_t lds_te0[kLdsTabWords];
    __shared__ uint32_t srk[44];
    lds_tab_fill(lds_te0);
    if (threadIdx.x < 44) srk[threadIdx.x] = rk[threadIdx.x];
    __syncthreads();
    LdsTab lt = lds_tab_make(lds_te0);
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nblocks; b += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t c = first_block + b;
        uint32_t s[1][4] = {{(uint32_t)c, (uint32_t)(c >> 32), 0u, 0u}};
        aes_encrypt_n<1, LdsTab>(lt, srk, s);
        out[b] = make_uint4(s[0][0], s[0][1], s[0][2], s[0][3]);
    }
}

// split the TI keystream into x[q][n], y[q][n], r[q]: word t of pair q sits at stream word
// q * (2n + 1) + t  (w-bit little-endian words; `skip` = byte offset of the first word in ks)
__global__ void ti_unpack_kernel(const uint8_t *ks, size_t skip, size_t npairs, size_t n, int wb, uint64_t *x, uint64_t *y,
                                 uint64_t *r) {
    const size_t per = 2 * n + 1, total = npairs * per;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const uint8_t *p = ks + skip + i * (size_t)wb;
        uint64_t v = 0;
        for (int b = 0; b < wb; b++) v |= (uint64_t)p[b] << (8 * b);
        size_t q = i / per, t = i % per;
        if (t < n) x[q * n + t] = v;
        else if (t < 2 * n) y[q * n + (t - n)] = v;
        else r[q] = v;
    }
}

// =============================================================== C ABI
static int p1_create(lgc_p1 **out, int device, size_t n, size_t d, size_t k, int width, int precision) {
    if (!out) return lgc_fail(LGC_EINVAL, "null out");
    if (width != 32 && width != 64) return lgc_fail(LGC_EINVAL, "width must be 32 or 64");
    if (precision < 0 || precision >= width) return lgc_fail(LGC_EINVAL, "precision must satisfy 0 <= p < width");
    if (n < 1 || d < 1) return lgc_fail(LGC_EINVAL, "empty data");
    int rc = lgc_need_device(device);
    if (rc) return rc;
    lgc_p1 *h = new lgc_p1();
    h->device = device; h->w = width; h->p = precision; h->n = h->n_all = n; h->d = d; h->k = k; h->X = h->X_all = 0; h->have_y = false; h->dev_io = false; h->divisor = d;
    hipError_t e = hipMalloc(&h->X_all, n * h->ld() * sizeof(int64_t));
    h->X = h->X_all;
    if (e != hipSuccess) { delete h; return lgc_fail(LGC_ENOMEM, "hipMalloc: %s", hipGetErrorString(e)); }
    *out = h;
    return LGC_OK;
}
extern "C" int lgc_p1_create(lgc_p1 **out, int device, size_t n, size_t d, int width, int precision) {
    return p1_create(out, device, n, d, 1, width, precision);
}
extern "C" int lgc_p1_create_targets(lgc_p1 **out, int device, size_t n, size_t d, size_t k, int width, int precision) {
    if (k < 1 || k > LGC_MAX_TARGETS) return lgc_fail(LGC_EINVAL, "the target count must be in 1..%d", LGC_MAX_TARGETS);
    return p1_create(out, device, n, d, k, width, precision);
}
extern "C" void lgc_p1_destroy(lgc_p1 *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->X_all) (void)hipFree(h->X_all);
    delete h;
}
// X and the target columns; Y: n x ny row-major (ny <= k; the other targets are zero) or NULL
static int p1_set(lgc_p1 *h, const int64_t *Xq, const int64_t *Y, size_t ny) {
    if (!h || !Xq) return lgc_fail(LGC_EINVAL, "null argument");
    P1CHK(hipSetDevice(h->device));
    const size_t ld = h->ld();
    std::vector<int64_t> tmp(h->n_all * ld, 0);    // all rows, whatever the window
    for (size_t k = 0; k < h->n_all; k++) {
        memcpy(&tmp[k * ld], Xq + k * h->d, h->d * sizeof(int64_t));
        if (Y) memcpy(&tmp[k * ld + h->d], Y + k * ny, ny * sizeof(int64_t));
    }
    P1CHK(hipMemcpy(h->X_all, tmp.data(), tmp.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    h->have_y = Y != 0;
    return LGC_OK;
}
extern "C" int lgc_p1_set_data(lgc_p1 *h, const int64_t *Xq, const int64_t *yq) { return p1_set(h, Xq, yq, 1); }
extern "C" int lgc_p1_set_targets(lgc_p1 *h, const int64_t *Xq, const int64_t *Yq) { return p1_set(h, Xq, Yq, h ? h->k : 0); }

static uint64_t maskw(int w) { return w == 32 ? 0xffffffffull : ~0ull; }
// the pairs of one launch of a kernel that takes its pair from blockIdx.y: HIP's limit on grid.y
#define P1_MAX_PAIRS 65535

// ---- the split-K rule of every block kernel above: the split count doubles while the grid has fewer than 2048 workgroups
// (enough for 256 CUs) and a split keeps at least 256 rows; a chunk is whole slabs of P1_KT rows.  Returns the splits of `rows`
// rows, every one *kchunk rows but the last.
static size_t p1_split_k(size_t workgroups_per_split, size_t rows, size_t *kchunk) {
    size_t ksplit = 1;
    while (workgroups_per_split * ksplit < 2048 && rows / (ksplit * 2) >= 256) ksplit *= 2;
    *kchunk = (rows + ksplit - 1) / ksplit;
    *kchunk = (*kchunk + P1_KT - 1) / P1_KT * P1_KT;
    return (rows + *kchunk - 1) / *kchunk;
}
// dC[t][i] (nt x own words, zeroed by the caller) += <column c0 + i, column y0 + t> over the window: p1_rect_kernel
static void p1_rect_block(const lgc_p1 *h, uint32_t c0, uint32_t own, uint32_t y0, uint32_t nt, uint64_t *dC) {
    const uint32_t otiles = (own + 63) / 64, ttiles = (nt + 63) / 64;
    size_t kchunk;
    const size_t ksplit = p1_split_k((size_t)otiles * ttiles, h->n, &kchunk);
    hipLaunchKernelGGL(p1_rect_kernel, dim3(otiles, ttiles, (unsigned)ksplit), dim3(256), 0, 0, h->X, h->n, h->ld(), c0, own, y0, nt, dC,
                       kchunk);
}
// out[i] = the floating-point diagonal word of column dcols[i], i < L, over `rows` rows from X: p1_diag_kernel
static void p1_diag(const lgc_p1 *h, const int64_t *X, size_t rows, const uint32_t *dcols, uint32_t L, uint64_t *out) {
    hipLaunchKernelGGL(p1_diag_kernel, dim3((L + P1_DC - 1) / P1_DC), dim3(1024), 0, 0, X, rows, h->ld(), dcols, L, h->p, h->w,
                       (double)h->divisor, out);
}

// the argument checks of the Gram-block entries
static int p1_local_args(const lgc_p1 *h, size_t c0, size_t c1, int with_y, const uint64_t *out_A, const uint64_t *out_b) {
    if (!h || !out_A) return lgc_fail(LGC_EINVAL, "null argument");
    if (c0 >= c1 || c1 > h->d) return lgc_fail(LGC_EINVAL, "bad column range");
    if (with_y && (!h->have_y || !out_b)) return lgc_fail(LGC_EINVAL, "y requested but not set");
    return LGC_OK;
}
// shares of the block a data provider can compute alone (src/phase1.c:562-571; 359-384 in OT mode), once per row range:
// range f is rows [fr[f], fr[f + 1]) of the window, and its block lands at out_A + f * own (own + 1) / 2, out_b + f * own,
// out_yy + f.  One p1_gram_folds_kernel launch over all ranges, then the diagonal, which is order-dependent (k ascending): once
// per range, on that range's rows.
// out_yy (with_y; may be null): entry (own, own) of every block, sum y_q y_q, which the Gram launch forms with the rest of the
// lower triangle (linreg_gc_inference.h, linreg_gc_folds_yy.h)
static int p1_gram_blocks(lgc_p1 *h, size_t c0, size_t c1, int with_y, size_t nranges, const size_t *fr, uint64_t *out_A, uint64_t *out_b,
                          uint64_t *out_yy) {
    DevFree dev_guard;   // temporary device buffers are released on every return path
    P1CHK(hipSetDevice(h->device));
    const uint32_t own = (uint32_t)(c1 - c0), L = own + (with_y ? 1u : 0u);
    const uint32_t tiles = (L + 63) / 64;
    // the splits of every range by p1_split_k, the ranges counted into the grid; the last chunk of a range ends with the range
    std::vector<P1FoldSplit> splits;
    for (size_t f = 0; f < nranges; f++) {
        size_t kchunk;
        p1_split_k((size_t)tiles * tiles * nranges, fr[f + 1] - fr[f], &kchunk);
        for (size_t k0 = fr[f]; k0 < fr[f + 1]; k0 += kchunk) {
            P1FoldSplit sp = {(unsigned long long)k0, (unsigned long long)(k0 + kchunk < fr[f + 1] ? k0 + kchunk : fr[f + 1]), (uint32_t)f, 0u};
            splits.push_back(sp);
        }
    }
    if (splits.size() > 65535) return lgc_fail(LGC_EINVAL, "internal: %zu row splits", splits.size());
    // one upload: the table of splits, then cols
    const size_t sbytes = splits.size() * sizeof(P1FoldSplit);
    std::vector<unsigned char> tab(sbytes + L * sizeof(uint32_t));
    memcpy(tab.data(), splits.data(), sbytes);
    uint32_t *cols = (uint32_t *)(tab.data() + sbytes);
    for (uint32_t i = 0; i < own; i++) cols[i] = (uint32_t)(c0 + i);
    if (with_y) cols[own] = (uint32_t)h->d;
    unsigned char *dtab = 0;
    uint64_t *dC = 0, *ddiag = 0;
    const size_t cwords = nranges * (size_t)L * L;
    P1CHK(hipMalloc(&dtab, tab.size())); dev_guard.add(dtab);
    P1CHK(hipMalloc(&dC, cwords * sizeof(uint64_t))); dev_guard.add(dC);
    P1CHK(hipMalloc(&ddiag, nranges * own * sizeof(uint64_t))); dev_guard.add(ddiag);
    P1CHK(hipMemcpy(dtab, tab.data(), tab.size(), hipMemcpyHostToDevice));
    const P1FoldSplit *dsplits = (const P1FoldSplit *)dtab;
    const uint32_t *dcols = (const uint32_t *)(dtab + sbytes);
    P1CHK(hipMemset(dC, 0, cwords * sizeof(uint64_t)));
    hipLaunchKernelGGL(p1_gram_folds_kernel, dim3(tiles, tiles, (unsigned)splits.size()), dim3(256), 0, 0, h->X, h->ld(), dcols, L, dC,
                       dsplits);
    for (size_t f = 0; f < nranges; f++) p1_diag(h, h->X + fr[f] * h->ld(), fr[f + 1] - fr[f], dcols, own, ddiag + f * own);
    P1CHK(hipGetLastError());
    std::vector<uint64_t> C(cwords), diag(nranges * own);
    P1CHK(hipMemcpy(C.data(), dC, C.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    P1CHK(hipMemcpy(diag.data(), ddiag, diag.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));

    const uint64_t m = maskw(h->w);
    const size_t T = (size_t)own * (own + 1) / 2;
    for (size_t f = 0; f < nranges; f++) {
        const uint64_t *Cf = &C[f * (size_t)L * L];
        for (uint32_t i = 0; i < own; i++)
            for (uint32_t j = 0; j <= i; j++)
                out_A[f * T + (size_t)i * (i + 1) / 2 + j] = (i == j ? diag[f * own + i] : Cf[(size_t)i * L + j]) & m;
        if (with_y)
            for (uint32_t i = 0; i < own; i++) out_b[f * own + i] = Cf[(size_t)own * L + i] & m;
        if (with_y && out_yy) out_yy[f] = Cf[(size_t)own * L + own] & m;
    }
    return LGC_OK;
}
static int p1_local(lgc_p1 *h, size_t c0, size_t c1, int with_y, uint64_t *out_A, uint64_t *out_b, uint64_t *out_yy) {
    int rc = p1_local_args(h, c0, c1, with_y, out_A, out_b);
    if (rc) return rc;
    const size_t fr[2] = {0, h->n};   // one range: the whole window
    return p1_gram_blocks(h, c0, c1, with_y, 1, fr, out_A, out_b, out_yy);
}
extern "C" int lgc_p1_local(lgc_p1 *h, size_t c0, size_t c1, int with_y, uint64_t *out_A, uint64_t *out_b) {
    return p1_local(h, c0, c1, with_y, out_A, out_b, 0);
}
extern "C" int lgc_p1_local_yy(lgc_p1 *h, size_t c0, size_t c1, uint64_t *out_A, uint64_t *out_b, uint64_t *out_yy) {
    if (!out_yy) return lgc_fail(LGC_EINVAL, "null argument");
    if (h && !h->have_y) return lgc_fail(LGC_EINVAL, "y^T y needs y: the object has none");
    return p1_local(h, c0, c1, 1, out_A, out_b, out_yy);
}

// ---- row folds (include/linreg_gc_folds.h)
extern "C" int lgc_fold_rows(size_t n, size_t folds, size_t k, size_t *r0, size_t *r1) {
    if (!r0 || !r1) return lgc_fail(LGC_EINVAL, "null argument");
    if (folds < 2 || folds > LGC_MAX_FOLDS) return lgc_fail(LGC_EINVAL, "wants 2..%d folds (got %zu)", LGC_MAX_FOLDS, folds);
    if (folds > n) return lgc_fail(LGC_EINVAL, "%zu folds of %zu rows: a fold would be empty", folds, n);
    if (k >= folds) return lgc_fail(LGC_EINVAL, "fold %zu of %zu", k, folds);
    const size_t q = n / folds, r = n % folds;               // floor(k n / K) = k q + floor(k r / K), without overflow
    *r0 = k * q + k * r / folds;
    *r1 = (k + 1) * q + (k + 1) * r / folds;
    return LGC_OK;
}
extern "C" int lgc_p1_set_rows(lgc_p1 *h, size_t r0, size_t r1) {
    if (!h) return lgc_fail(LGC_EINVAL, "null handle");
    if (r0 >= r1 || r1 > h->n_all) return lgc_fail(LGC_EINVAL, "bad row window [%zu, %zu) of %zu rows", r0, r1, h->n_all);
    h->X = h->X_all + r0 * h->ld();
    h->n = r1 - r0;
    return LGC_OK;
}
// K windowed lgc_p1_local calls from one read of X: p1_gram_blocks over the K row folds of the window
static int p1_local_folds(lgc_p1 *h, size_t c0, size_t c1, int with_y, size_t folds, uint64_t *out_A, uint64_t *out_b, uint64_t *out_yy) {
    int rc = p1_local_args(h, c0, c1, with_y, out_A, out_b);
    if (rc) return rc;
    std::vector<size_t> fr(folds + 1, 0);
    for (size_t f = 0; f < folds; f++) {
        rc = lgc_fold_rows(h->n, folds, f, &fr[f], &fr[f + 1]);
        if (rc) return rc;
    }
    return p1_gram_blocks(h, c0, c1, with_y, folds, fr.data(), out_A, out_b, out_yy);
}
extern "C" int lgc_p1_local_folds(lgc_p1 *h, size_t c0, size_t c1, int with_y, size_t folds, uint64_t *out_A, uint64_t *out_b) {
    return p1_local_folds(h, c0, c1, with_y, folds, out_A, out_b, 0);
}
extern "C" int lgc_p1_local_folds_yy(lgc_p1 *h, size_t c0, size_t c1, size_t folds, uint64_t *out_A, uint64_t *out_b, uint64_t *out_yy) {
    if (!out_yy) return lgc_fail(LGC_EINVAL, "null argument");
    if (h && !h->have_y) return lgc_fail(LGC_EINVAL, "the folds' y^T y needs y: the object has none");
    return p1_local_folds(h, c0, c1, 1, folds, out_A, out_b, out_yy);
}

// ---- association scan (include/linreg_gc_scan.h)
extern "C" int lgc_p1_set_divisor(lgc_p1 *h, size_t divisor) {
    if (!h) return lgc_fail(LGC_EINVAL, "null handle");
    if (!divisor) return lgc_fail(LGC_EINVAL, "the divisor of the diagonal must be >= 1");
    h->divisor = divisor;
    return LGC_OK;
}
template <int NZ>
static void p1_scan_launch(const lgc_p1 *h, dim3 grid, uint32_t s0, uint32_t ns, uint32_t c0, uint32_t nc, uint32_t z0, uint32_t nz,
                           uint64_t *dC, size_t kchunk) {
    hipLaunchKernelGGL(p1_scan_kernel<NZ>, grid, dim3(256), 0, 0, h->X, h->n, h->ld(), s0, ns, c0, nc, (uint32_t)h->d, z0, nz, dC, kchunk);
}
// the launches of p1_scan_kernel for one block: dC[m][q] (ns x nz words, zeroed by the caller) += <column s0 + m, column q of Z>
static int p1_scan_block(const lgc_p1 *h, uint32_t c0, uint32_t nc, uint32_t s0, uint32_t ns, uint32_t nz, uint64_t *dC) {
    const uint32_t groups = (ns + 255) / 256;
    size_t kchunk;
    const size_t ksplit = p1_split_k(groups, h->n, &kchunk);
    if (ksplit > 65535) return lgc_fail(LGC_EINVAL, "internal: %zu row splits", ksplit);
    const dim3 grid(groups, (unsigned)ksplit);
    for (uint32_t z0 = 0; z0 < nz; z0 += 32) {       // passes of 32 columns of Z
        const uint32_t left = nz - z0;
        if (left > 16) p1_scan_launch<32>(h, grid, s0, ns, c0, nc, z0, nz, dC, kchunk);
        else if (left > 8) p1_scan_launch<16>(h, grid, s0, ns, c0, nc, z0, nz, dC, kchunk);
        else if (left > 4) p1_scan_launch<8>(h, grid, s0, ns, c0, nc, z0, nz, dC, kchunk);
        else if (left > 2) p1_scan_launch<4>(h, grid, s0, ns, c0, nc, z0, nz, dC, kchunk);
        else if (left > 1) p1_scan_launch<2>(h, grid, s0, ns, c0, nc, z0, nz, dC, kchunk);
        else p1_scan_launch<1>(h, grid, s0, ns, c0, nc, z0, nz, dC, kchunk);
    }
    return LGC_OK;
}
// A/B hook (linreg_gc_debug.h): the integer block of lgc_p1_local_scan alone, by p1_scan_kernel (use_rect = 0) or by
// p1_rect_kernel (use_rect = 1: Z must be contiguous columns, i.e. c1 == d when with_y), timed by HIP events around the kernels
extern "C" int lgc_test_p1_scan_block(lgc_p1 *h, size_t c0, size_t c1, size_t s0, size_t s1, int with_y, int use_rect, uint64_t *out,
                                      double *ms) {
    DevFree dev_guard;
    if (!h || !out || !ms) return lgc_fail(LGC_EINVAL, "null argument");
    if (c0 > c1 || c1 > h->d || s0 >= s1 || s1 > h->d || (c0 < c1 && s0 < c1 && c0 < s1)) return lgc_fail(LGC_EINVAL, "bad column ranges");
    if (with_y && !h->have_y) return lgc_fail(LGC_EINVAL, "y requested but not set");
    const uint32_t ns = (uint32_t)(s1 - s0), nc = (uint32_t)(c1 - c0), nz = nc + (with_y ? 1u : 0u);
    if (!nz) return lgc_fail(LGC_EINVAL, "no column of Z");
    if (use_rect && with_y && nc && c1 != h->d) return lgc_fail(LGC_EINVAL, "p1_rect_kernel reads contiguous target columns: c1 must be d");
    P1CHK(hipSetDevice(h->device));
    uint64_t *dC = 0;
    struct Events {   // destroyed on every return path
        hipEvent_t e0 = 0, e1 = 0;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    const size_t cwords = (size_t)ns * nz;
    P1CHK(hipMalloc(&dC, cwords * sizeof(uint64_t))); dev_guard.add(dC);
    P1CHK(hipMemset(dC, 0, cwords * sizeof(uint64_t)));
    P1CHK(hipEventCreate(&ev.e0)); P1CHK(hipEventCreate(&ev.e1));
    P1CHK(hipEventRecord(ev.e0, 0));
    if (use_rect) {
        p1_rect_block(h, (uint32_t)s0, ns, (uint32_t)(nc ? c0 : h->d), nz, dC);
    } else {
        int rc = p1_scan_block(h, (uint32_t)c0, nc, (uint32_t)s0, ns, nz, dC);
        if (rc) return rc;
    }
    P1CHK(hipEventRecord(ev.e1, 0));
    P1CHK(hipEventSynchronize(ev.e1));
    float t = 0;
    P1CHK(hipEventElapsedTime(&t, ev.e0, ev.e1));
    *ms = (double)t;
    std::vector<uint64_t> C(cwords);
    P1CHK(hipMemcpy(C.data(), dC, cwords * sizeof(uint64_t), hipMemcpyDeviceToHost));
    const uint64_t m = maskw(h->w);
    for (uint32_t i = 0; i < ns; i++)      // p1_rect_kernel writes C[t][i], p1_scan_kernel C[i][t]
        for (uint32_t q = 0; q < nz; q++) out[(size_t)i * nz + q] = (use_rect ? C[(size_t)q * ns + i] : C[(size_t)i * nz + q]) & m;
    return LGC_OK;
}
// the candidates' block of a data provider: H and gy from p1_scan_kernel, gg from p1_diag_kernel
extern "C" int lgc_p1_local_scan(lgc_p1 *h, size_t c0, size_t c1, size_t s0, size_t s1, int with_y,
                                 uint64_t *out_H, uint64_t *out_gg, uint64_t *out_gy) {
    DevFree dev_guard;   // temporary device buffers are released on every return path
    if (!h || !out_gg) return lgc_fail(LGC_EINVAL, "null argument");
    if (c0 > c1 || c1 > h->d) return lgc_fail(LGC_EINVAL, "bad covariate range");
    if (s0 >= s1 || s1 > h->d) return lgc_fail(LGC_EINVAL, "bad candidate range");
    if (c0 < c1 && s0 < c1 && c0 < s1) return lgc_fail(LGC_EINVAL, "the candidate columns [%zu, %zu) overlap the covariates [%zu, %zu)", s0, s1, c0, c1);
    if (c0 < c1 && !out_H) return lgc_fail(LGC_EINVAL, "null out_H");
    if (with_y && (!h->have_y || !out_gy)) return lgc_fail(LGC_EINVAL, "y requested but not set");
    P1CHK(hipSetDevice(h->device));
    const uint32_t ns = (uint32_t)(s1 - s0), nc = (uint32_t)(c1 - c0), nz = nc + (with_y ? 1u : 0u);
    std::vector<uint32_t> cols(ns);
    for (uint32_t i = 0; i < ns; i++) cols[i] = (uint32_t)(s0 + i);
    uint32_t *dcols = 0;
    uint64_t *dC = 0, *ddiag = 0;
    P1CHK(hipMalloc(&dcols, ns * sizeof(uint32_t))); dev_guard.add(dcols);
    P1CHK(hipMalloc(&ddiag, ns * sizeof(uint64_t))); dev_guard.add(ddiag);
    P1CHK(hipMemcpy(dcols, cols.data(), ns * sizeof(uint32_t), hipMemcpyHostToDevice));
    const size_t cwords = (size_t)ns * nz;
    if (nz) {
        P1CHK(hipMalloc(&dC, cwords * sizeof(uint64_t))); dev_guard.add(dC);
        P1CHK(hipMemset(dC, 0, cwords * sizeof(uint64_t)));
        int rc = p1_scan_block(h, (uint32_t)c0, nc, (uint32_t)s0, ns, nz, dC);
        if (rc) return rc;
    }
    p1_diag(h, h->X, h->n, dcols, ns, ddiag);
    P1CHK(hipGetLastError());
    std::vector<uint64_t> C(cwords);
    if (nz) P1CHK(hipMemcpy(C.data(), dC, cwords * sizeof(uint64_t), hipMemcpyDeviceToHost));
    P1CHK(hipMemcpy(out_gg, ddiag, ns * sizeof(uint64_t), hipMemcpyDeviceToHost));
    const uint64_t m = maskw(h->w);
    for (uint32_t i = 0; i < ns; i++) {
        out_gg[i] &= m;
        for (uint32_t q = 0; q < nc; q++) out_H[(size_t)i * nc + q] = C[(size_t)i * nz + q] & m;
        if (with_y) out_gy[i] = C[(size_t)i * nz + nc] & m;
    }
    return LGC_OK;
}

// lgc_p1_local for a handle with k targets: out_A exactly as lgc_p1_local (Gram kernel over the own columns, the diagonal in
// double), out_B[t][i] = <column c0 + i, target t> from the rectangular kernel
extern "C" int lgc_p1_local_targets(lgc_p1 *h, size_t c0, size_t c1, uint64_t *out_A, uint64_t *out_B) {
    DevFree dev_guard;   // temporary device buffers are released on every return path
    int rc = lgc_p1_local(h, c0, c1, 0, out_A, 0);   // (and the argument checks)
    if (rc || !out_B) return rc;
    P1CHK(hipSetDevice(h->device));
    const uint32_t own = (uint32_t)(c1 - c0), nt = (uint32_t)h->k;
    uint64_t *dC = 0;
    P1CHK(hipMalloc(&dC, (size_t)nt * own * sizeof(uint64_t))); dev_guard.add(dC);
    P1CHK(hipMemset(dC, 0, (size_t)nt * own * sizeof(uint64_t)));
    p1_rect_block(h, (uint32_t)c0, own, (uint32_t)h->d, nt, dC);
    P1CHK(hipGetLastError());
    P1CHK(hipMemcpy(out_B, dC, (size_t)nt * own * sizeof(uint64_t), hipMemcpyDeviceToHost));
    const uint64_t m = maskw(h->w);
    for (size_t i = 0; i < (size_t)nt * own; i++) out_B[i] &= m;
    return LGC_OK;
}

// Per-thread device scratch for the per-pair calls below (a data provider runs one worker thread
// per peer; hipMalloc/hipFree per pair would dominate at small n).  Grown on demand, released
// when the thread exits.
struct P1Scratch {
    void *ptr[4];
    size_t cap[4];
    int device;
    P1Scratch() : device(-1) { for (int i = 0; i < 4; i++) { ptr[i] = 0; cap[i] = 0; } }
    ~P1Scratch() { release(); }
    void release() {
        for (int i = 0; i < 4; i++) { if (ptr[i]) (void)hipFree(ptr[i]); ptr[i] = 0; cap[i] = 0; }
    }
    hipError_t get(int dev, int slot, size_t bytes, void **out) {
        if (dev != device) { release(); device = dev; }
        if (cap[slot] < bytes) {
            if (ptr[slot]) (void)hipFree(ptr[slot]);
            ptr[slot] = 0; cap[slot] = 0;
            size_t want = bytes + bytes / 4 + 256;
            hipError_t e = hipMalloc(&ptr[slot], want);
            if (e != hipSuccess) return e;
            cap[slot] = want;
        }
        *out = ptr[slot];
        return hipSuccess;
    }
};
static thread_local P1Scratch t_scratch;

// Stream policy of the per-pair / per-batch calls.  A data provider runs a worker thread per peer, and five
// provider processes share one GPU in the single-box runs.  A stream (= a hardware queue) per worker thread
// oversubscribes the queues, which the scheduler then time-slices at millisecond granularity: config 4 takes
// 65.7 s that way against 21.5 s with all calls of a process taking turns on ONE stream -- measured again in
// round 2 with one call per batch of 16 pairs (per-thread streams: not kept).
#include <mutex>
static std::mutex g_p1_mutex;
static bool p1_shared_stream() { return true; }
struct P1Serial {
    bool locked;
    P1Serial() : locked(p1_shared_stream()) { if (locked) g_p1_mutex.lock(); }
    ~P1Serial() { if (locked) g_p1_mutex.unlock(); }
};
struct P1ThreadStream {
    hipStream_t st; int device;
    P1ThreadStream() : st(0), device(-1) {}
    ~P1ThreadStream() { if (st) (void)hipStreamDestroy(st); }
};
static thread_local P1ThreadStream t_stream;
static hipStream_t p1_stream() {
    if (p1_shared_stream()) return 0;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (!t_stream.st || t_stream.device != dev) {
        if (t_stream.st) (void)hipStreamDestroy(t_stream.st);
        t_stream.st = 0; t_stream.device = dev;
        if (hipStreamCreateWithFlags(&t_stream.st, hipStreamNonBlocking) != hipSuccess) t_stream.st = 0;
    }
    return t_stream.st;
}

// out[q][k] = column cols[q] (d means y) +/- V[q][k]: the vectors a DP sends in inner_product_ti
// (b + x at phase1.c:201-207, a - y at 186-191).  Safe to call from several threads on one handle.
extern "C" int lgc_p1_mask(lgc_p1 *h, const uint32_t *cols, size_t npairs, const uint64_t *V, int sign, uint64_t *out) {
    if (!h || !cols || !V || !out) return lgc_fail(LGC_EINVAL, "null argument");
    if (npairs == 0) return LGC_OK;
    for (size_t q = 0; q < npairs; q++) if (cols[q] >= h->ld()) return lgc_fail(LGC_EINVAL, "column out of range");
    // grid.y is the pair: the device-I/O branch launches in chunks, the host paths take one launch
    if (!h->dev_io && npairs > P1_MAX_PAIRS) return lgc_fail(LGC_EINVAL, "too many pairs in one call (at most %d)", P1_MAX_PAIRS);
    P1CHK(hipSetDevice(h->device));
    P1Serial serial_; hipStream_t st = p1_stream();
    uint32_t *dcols = 0; uint64_t *dV = 0, *dout = 0;
    size_t bytes = npairs * h->n * sizeof(uint64_t);
    if (h->dev_io) {     // V and out are device memory (same-node rings): no copies
        P1CHK(t_scratch.get(h->device, 0, npairs * sizeof(uint32_t), (void **)&dcols));
        P1CHK(hipMemcpyAsync(dcols, cols, npairs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        unsigned gx = (unsigned)((h->n + 255) / 256); if (gx > 64) gx = 64;
        for (size_t q0 = 0; q0 < npairs; q0 += 65535) {
            unsigned gy = (unsigned)(npairs - q0 < 65535 ? npairs - q0 : 65535);
            hipLaunchKernelGGL(p1_mask_kernel, dim3(gx, gy), dim3(256), 0, st, h->X, h->n, h->ld(), dcols + q0, V + q0 * h->n, sign, out + q0 * h->n, maskw(h->w));
            P1CHK(hipGetLastError());
        }
        P1CHK(hipGetLastError());
        P1CHK(hipStreamSynchronize(st));
        return LGC_OK;
    }
    if (npairs == 1) {   // per-pair protocol step: three operations
        P1CHK(t_scratch.get(h->device, 1, bytes, (void **)&dV));
        P1CHK(t_scratch.get(h->device, 2, bytes, (void **)&dout));
        P1CHK(hipMemcpyAsync(dV, V, bytes, hipMemcpyHostToDevice, st));
        unsigned g1 = (unsigned)((h->n + 1023) / 1024); if (g1 > 64) g1 = 64;
        hipLaunchKernelGGL(p1_mask1_kernel, dim3(g1), dim3(1024), 0, st, h->X, h->n, h->ld(), cols[0], dV, sign, dout, maskw(h->w));
        P1CHK(hipGetLastError());
        P1CHK(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, st));
        P1CHK(hipStreamSynchronize(st));
        if (h->w == 32) for (size_t i = 0; i < h->n; i++) out[i] &= 0xffffffffull;
        return LGC_OK;
    }
    P1CHK(t_scratch.get(h->device, 0, npairs * sizeof(uint32_t), (void **)&dcols));
    P1CHK(t_scratch.get(h->device, 1, bytes, (void **)&dV));
    P1CHK(t_scratch.get(h->device, 2, bytes, (void **)&dout));
    P1CHK(hipMemcpyAsync(dcols, cols, npairs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    P1CHK(hipMemcpyAsync(dV, V, bytes, hipMemcpyHostToDevice, st));
    unsigned gx = (unsigned)((h->n + 255) / 256); if (gx > 64) gx = 64;
    hipLaunchKernelGGL(p1_mask_kernel, dim3(gx, (unsigned)npairs), dim3(256), 0, st, h->X, h->n, h->ld(), dcols, dV, sign, dout, maskw(h->w));
    P1CHK(hipGetLastError());
    P1CHK(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, st));
    P1CHK(hipStreamSynchronize(st));
    const uint64_t m = maskw(h->w);
    if (h->w == 32) for (size_t i = 0; i < npairs * h->n; i++) out[i] &= m;
    return LGC_OK;
}

// out[q] = <A[q], B[q]> (colsB == NULL) or <A[q], column colsB[q]>, minus sub[q]  (mod 2^w):
// the share arithmetic of inner_product_ti (phase1.c:194-196, 220-222).  Thread-safe like lgc_p1_mask.
extern "C" int lgc_p1_dot(lgc_p1 *h, const uint64_t *A, const uint64_t *B, const uint32_t *colsB, size_t npairs,
                          const uint64_t *sub, uint64_t *out) {
    if (!h || !A || !out || (!B && !colsB)) return lgc_fail(LGC_EINVAL, "null argument");
    if (npairs == 0) return LGC_OK;
    if (colsB) for (size_t q = 0; q < npairs; q++) if (colsB[q] >= h->ld()) return lgc_fail(LGC_EINVAL, "column out of range");
    if (npairs > P1_MAX_PAIRS) return lgc_fail(LGC_EINVAL, "too many pairs in one call (at most %d)", P1_MAX_PAIRS);   // grid.y is the pair
    P1CHK(hipSetDevice(h->device));
    P1Serial serial_; hipStream_t st = p1_stream();
    size_t bytes = npairs * h->n * sizeof(uint64_t);
    uint64_t *dA = 0, *dB = 0, *dout = 0; uint32_t *dcols = 0;
    if (h->dev_io) {     // A (and B) are device memory; the sums still return to the host
        if (colsB) {
            P1CHK(t_scratch.get(h->device, 0, npairs * sizeof(uint32_t), (void **)&dcols));
            P1CHK(hipMemcpyAsync(dcols, colsB, npairs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        }
        P1CHK(t_scratch.get(h->device, 3, npairs * sizeof(uint64_t), (void **)&dout));
        P1CHK(hipMemsetAsync(dout, 0, npairs * sizeof(uint64_t), st));
        unsigned gx = (unsigned)((h->n + 255) / 256); if (gx > 64) gx = 64;
        hipLaunchKernelGGL(p1_dot_kernel, dim3(gx, (unsigned)npairs), dim3(256), 0, st, A, B, h->X, h->ld(), dcols, h->n, dout);
        P1CHK(hipGetLastError());
        P1CHK(hipMemcpyAsync(out, dout, npairs * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        P1CHK(hipStreamSynchronize(st));
        const uint64_t mm = maskw(h->w);
        for (size_t q = 0; q < npairs; q++) out[q] = (out[q] - (sub ? sub[q] : 0)) & mm;
        return LGC_OK;
    }
    P1CHK(t_scratch.get(h->device, 1, bytes, (void **)&dA));
    P1CHK(hipMemcpyAsync(dA, A, bytes, hipMemcpyHostToDevice, st));
    if (npairs == 1) {   // per-pair protocol step: one workgroup writes the sum, no memset
        if (!colsB) {
            P1CHK(t_scratch.get(h->device, 2, bytes, (void **)&dB));
            P1CHK(hipMemcpyAsync(dB, B, bytes, hipMemcpyHostToDevice, st));
        }
        P1CHK(t_scratch.get(h->device, 3, sizeof(uint64_t), (void **)&dout));
        P1CHK(hipMemsetAsync(dout, 0, sizeof(uint64_t), st));
        unsigned g1 = (unsigned)((h->n + 1023) / 1024); if (g1 > 64) g1 = 64;
        hipLaunchKernelGGL(p1_dot1_kernel, dim3(g1), dim3(1024), 0, st, dA, dB, h->X, h->ld(), colsB ? colsB[0] : 0u, h->n, dout);
        P1CHK(hipGetLastError());
        P1CHK(hipMemcpyAsync(out, dout, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        P1CHK(hipStreamSynchronize(st));
        out[0] = (out[0] - (sub ? sub[0] : 0)) & maskw(h->w);
        return LGC_OK;
    }
    if (colsB) {
        P1CHK(t_scratch.get(h->device, 0, npairs * sizeof(uint32_t), (void **)&dcols));
        P1CHK(hipMemcpyAsync(dcols, colsB, npairs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    } else {
        P1CHK(t_scratch.get(h->device, 2, bytes, (void **)&dB));
        P1CHK(hipMemcpyAsync(dB, B, bytes, hipMemcpyHostToDevice, st));
    }
    P1CHK(t_scratch.get(h->device, 3, npairs * sizeof(uint64_t), (void **)&dout));
    P1CHK(hipMemsetAsync(dout, 0, npairs * sizeof(uint64_t), st));
    unsigned gx = (unsigned)((h->n + 255) / 256); if (gx > 64) gx = 64;
    hipLaunchKernelGGL(p1_dot_kernel, dim3(gx, (unsigned)npairs), dim3(256), 0, st, dA, dB, h->X, h->ld(), dcols, h->n, dout);
    P1CHK(hipGetLastError());
    P1CHK(hipMemcpyAsync(out, dout, npairs * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    P1CHK(hipStreamSynchronize(st));
    const uint64_t m = maskw(h->w);
    for (size_t q = 0; q < npairs; q++) out[q] = (out[q] - (sub ? sub[q] : 0)) & m;
    return LGC_OK;
}

// Party a of one inner_product_ti (phase1.c:171-197) in a single pass: out_mask = a - y (sent to
// party b) and *share = <in, y> - sub, where `in` = b + x is party b's message, (y, sub) the TI's.
extern "C" int lgc_p1_ti_a(lgc_p1 *h, uint32_t col, const uint64_t *y, const uint64_t *in, uint64_t sub,
                           uint64_t *out_mask, uint64_t *share) {
    if (!h || !y || !in || !out_mask || !share) return lgc_fail(LGC_EINVAL, "null argument");
    if (col >= h->ld()) return lgc_fail(LGC_EINVAL, "column out of range");
    P1CHK(hipSetDevice(h->device));
    P1Serial serial_; hipStream_t st = p1_stream();
    const size_t n = h->n, bytes = n * sizeof(uint64_t);
    uint64_t *dy = 0, *din = 0, *dout = 0;
    P1CHK(t_scratch.get(h->device, 1, bytes, (void **)&dy));
    P1CHK(t_scratch.get(h->device, 2, bytes, (void **)&din));
    P1CHK(t_scratch.get(h->device, 3, bytes + sizeof(uint64_t), (void **)&dout));
    P1CHK(hipMemcpyAsync(dy, y, bytes, hipMemcpyHostToDevice, st));
    P1CHK(hipMemcpyAsync(din, in, bytes, hipMemcpyHostToDevice, st));
    P1CHK(hipMemsetAsync(dout + n, 0, sizeof(uint64_t), st));
    unsigned g1 = (unsigned)((n + 1023) / 1024); if (g1 > 64) g1 = 64;
    hipLaunchKernelGGL(p1_ti_a_kernel, dim3(g1), dim3(1024), 0, st, h->X, n, h->ld(), col, dy, din, dout, maskw(h->w));
    P1CHK(hipGetLastError());
    P1CHK(hipMemcpyAsync(out_mask, dout, bytes, hipMemcpyDeviceToHost, st));
    uint64_t acc = 0;
    P1CHK(hipMemcpyAsync(&acc, dout + n, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    P1CHK(hipStreamSynchronize(st));
    const uint64_t m = maskw(h->w);
    if (h->w == 32) for (size_t i = 0; i < n; i++) out_mask[i] &= m;
    *share = (acc - sub) & m;
    return LGC_OK;
}

// Party a for a run of pairs with the same peer in one device call: y, in, out_mask are npairs x n words
// (page-locked host buffers move at the PCIe rate), cols / sub / shares have npairs entries.
extern "C" int lgc_p1_ti_a_batch(lgc_p1 *h, const uint32_t *cols, size_t npairs, const uint64_t *y, const uint64_t *in,
                                 const uint64_t *sub, uint64_t *out_mask, uint64_t *shares) {
    if (!h || !cols || !y || !in || !sub || !out_mask || !shares) return lgc_fail(LGC_EINVAL, "null argument");
    if (npairs == 0) return LGC_OK;
    for (size_t q = 0; q < npairs; q++) if (cols[q] >= h->ld()) return lgc_fail(LGC_EINVAL, "column out of range");
    P1CHK(hipSetDevice(h->device));
    P1Serial serial_; hipStream_t st = p1_stream();
    const size_t n = h->n, bytes = npairs * n * sizeof(uint64_t);
    uint64_t *dy = 0, *din = 0, *dout = 0; uint32_t *dcols = 0;
    if (h->dev_io) {     // y, in and out_mask are device memory
        uint64_t *dacc = 0;
        P1CHK(t_scratch.get(h->device, 0, npairs * sizeof(uint32_t), (void **)&dcols));
        P1CHK(t_scratch.get(h->device, 3, npairs * sizeof(uint64_t), (void **)&dacc));
        P1CHK(hipMemcpyAsync(dcols, cols, npairs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        P1CHK(hipMemsetAsync(dacc, 0, npairs * sizeof(uint64_t), st));
        unsigned gx = (unsigned)((n + 255) / 256); if (gx > 64) gx = 64;
        unsigned gy = npairs > 65535 ? 65535u : (unsigned)npairs;
        hipLaunchKernelGGL(p1_ti_a_batch_kernel, dim3(gx, gy), dim3(256), 0, st, h->X, n, h->ld(), dcols, npairs, y, in, out_mask, dacc, maskw(h->w));
        P1CHK(hipGetLastError());
        P1CHK(hipMemcpyAsync(shares, dacc, npairs * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        P1CHK(hipStreamSynchronize(st));
        const uint64_t mm = maskw(h->w);
        for (size_t q = 0; q < npairs; q++) shares[q] = (shares[q] - sub[q]) & mm;
        return LGC_OK;
    }
    P1CHK(t_scratch.get(h->device, 0, npairs * sizeof(uint32_t), (void **)&dcols));
    P1CHK(t_scratch.get(h->device, 1, bytes, (void **)&dy));
    P1CHK(t_scratch.get(h->device, 2, bytes, (void **)&din));
    P1CHK(t_scratch.get(h->device, 3, bytes + npairs * sizeof(uint64_t), (void **)&dout));
    P1CHK(hipMemcpyAsync(dcols, cols, npairs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    P1CHK(hipMemcpyAsync(dy, y, bytes, hipMemcpyHostToDevice, st));
    P1CHK(hipMemcpyAsync(din, in, bytes, hipMemcpyHostToDevice, st));
    P1CHK(hipMemsetAsync(dout + npairs * n, 0, npairs * sizeof(uint64_t), st));
    unsigned gx = (unsigned)((n + 255) / 256); if (gx > 64) gx = 64;
    unsigned gy = npairs > 65535 ? 65535u : (unsigned)npairs;
    hipLaunchKernelGGL(p1_ti_a_batch_kernel, dim3(gx, gy), dim3(256), 0, st, h->X, n, h->ld(), dcols, npairs, dy, din, dout, dout + npairs * n, maskw(h->w));
    P1CHK(hipGetLastError());
    P1CHK(hipMemcpyAsync(out_mask, dout, bytes, hipMemcpyDeviceToHost, st));
    P1CHK(hipMemcpyAsync(shares, dout + npairs * n, npairs * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    P1CHK(hipStreamSynchronize(st));
    const uint64_t m = maskw(h->w);
    if (h->w == 32) for (size_t i = 0; i < npairs * n; i++) out_mask[i] &= m;
    for (size_t q = 0; q < npairs; q++) shares[q] = (shares[q] - sub[q]) & m;
    return LGC_OK;
}

extern "C" int lgc_p1_set_device_io(lgc_p1 *h, int on) {
    if (!h) return lgc_fail(LGC_EINVAL, "null handle");
    h->dev_io = on != 0;
    return LGC_OK;
}

// the TI's keystream split straight into per-pair destinations (device rings of the data providers): word t of
// pair q sits at stream word q (2n + 1) + t; x -> xdst[q], y -> ydst[q], r -> r[q].  Aligned word loads
// (the stream offset of a batch is a multiple of the word size).
template <typename WT>
__global__ void ti_unpack_scatter_kernel(const WT *ks, size_t npairs, size_t n, uint64_t *const *xdst, uint64_t *const *ydst, uint64_t *r) {
    const size_t per = 2 * n + 1;
    for (size_t q = blockIdx.y; q < npairs; q += gridDim.y) {
        const WT *src = ks + q * per;
        uint64_t *dx = xdst[q], *dy = ydst[q];
        for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < per; t += (size_t)gridDim.x * blockDim.x) {
            const uint64_t v = (uint64_t)src[t];
            if (t < n) dx[t] = v;
            else if (t < 2 * n) dy[t - n] = v;
            else r[q] = v;
        }
    }
}
// out[q] = <xdst[q], ydst[q]>  (mod 2^64); out zeroed by the host
__global__ void __launch_bounds__(256)
p1_dot_ptr_kernel(uint64_t *const *xdst, uint64_t *const *ydst, size_t npairs, size_t n, uint64_t *out) {
    for (size_t q = blockIdx.y; q < npairs; q += gridDim.y) {
        const uint64_t *a = xdst[q], *b = ydst[q];
        uint64_t acc = 0;
        for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) acc += a[k] * b[k];
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd((unsigned long long *)&out[q], (unsigned long long)acc);
    }
}

// Trusted initializer (phase1.c:241-287): for pairs [first_pair, first_pair + npairs) of the
// (i, j) enumeration, words x[n], y[n], r drawn in this order from one AES-128-CTR stream keyed
// by `seed`; xy_minus_r[q] = <x,y> - r.  Stream position of pair q is q * (2n + 1) words.
static int ti_generate(int device, const uint8_t seed[16], uint64_t first_pair, size_t npairs, size_t n, int width,
                       uint64_t *x, uint64_t *y, void *const *x_dst, void *const *y_dst, uint64_t *r, uint64_t *xy_minus_r) {
    DevFree dev_guard;   // temporary device buffers are released on every return path
    if (!seed || !r || !xy_minus_r || (!x && !x_dst) || (!y && !y_dst)) return lgc_fail(LGC_EINVAL, "null argument");
    if (width != 32 && width != 64) return lgc_fail(LGC_EINVAL, "width must be 32 or 64");
    if (npairs == 0) return LGC_OK;
    if (npairs > P1_MAX_PAIRS) return lgc_fail(LGC_EINVAL, "too many pairs in one call (at most %d)", P1_MAX_PAIRS);   // p1_dot_kernel below
    int rc = lgc_need_device(device);
    if (rc) return rc;
    AesTables t;
    aes_build_tables(t, seed);
    uint32_t *drk = 0;
    P1CHK(hipMalloc(&drk, sizeof(t.rk))); dev_guard.add(drk);
    P1CHK(hipMemcpy(drk, t.rk, sizeof(t.rk), hipMemcpyHostToDevice));
    const size_t wb = width / 8;
    const uint64_t words_per_pair = 2 * n + 1;
    const uint64_t byte0 = first_pair * words_per_pair * wb, byte1 = (first_pair + npairs) * words_per_pair * wb;
    const uint64_t blk0 = byte0 / 16, blk1 = (byte1 + 15) / 16;
    uint4 *dks = 0;
    P1CHK(hipMalloc(&dks, (blk1 - blk0) * 16)); dev_guard.add(dks);
    hipLaunchKernelGGL(ti_prg_kernel, dim3(512), dim3(1024), 0, 0, drk, blk0, blk1 - blk0, dks);
    P1CHK(hipGetLastError());
    const uint64_t m = maskw(width);
    uint64_t *dA = 0, *dB = 0, *dr = 0, *dout = 0;
    size_t bytes = npairs * n * 8;
    P1CHK(hipMalloc(&dA, bytes)); dev_guard.add(dA); P1CHK(hipMalloc(&dB, bytes)); dev_guard.add(dB); P1CHK(hipMalloc(&dr, npairs * 8)); dev_guard.add(dr); P1CHK(hipMalloc(&dout, npairs * 8)); dev_guard.add(dout);
    hipLaunchKernelGGL(ti_unpack_kernel, dim3(1024), dim3(256), 0, 0, (const uint8_t *)dks, (size_t)(byte0 - blk0 * 16), npairs, n,
                       (int)wb, dA, dB, dr);
    P1CHK(hipGetLastError());
    P1CHK(hipMemset(dout, 0, npairs * 8));
    unsigned gx = (unsigned)((n + 255) / 256); if (gx > 64) gx = 64;
    hipLaunchKernelGGL(p1_dot_kernel, dim3(gx, (unsigned)npairs), dim3(256), 0, 0, dA, dB, (const int64_t *)0, (size_t)0,
                       (const uint32_t *)0, n, dout);
    P1CHK(hipGetLastError());
    if (x_dst) {
        return lgc_fail(LGC_EINVAL, "internal: scatter requests go through ti_generate_scatter");
    } else {
        P1CHK(hipMemcpy(x, dA, bytes, hipMemcpyDeviceToHost));
        P1CHK(hipMemcpy(y, dB, bytes, hipMemcpyDeviceToHost));
    }
    P1CHK(hipMemcpy(r, dr, npairs * 8, hipMemcpyDeviceToHost));
    P1CHK(hipMemcpy(xy_minus_r, dout, npairs * 8, hipMemcpyDeviceToHost));

    for (size_t q = 0; q < npairs; q++) xy_minus_r[q] = (xy_minus_r[q] - r[q]) & m;
    return LGC_OK;
}
extern "C" int lgc_ti_generate(int device, const uint8_t seed[16], uint64_t first_pair, size_t npairs, size_t n, int width,
                               uint64_t *x, uint64_t *y, uint64_t *r, uint64_t *xy_minus_r) {
    if (!x || !y) return lgc_fail(LGC_EINVAL, "null argument");
    return ti_generate(device, seed, first_pair, npairs, n, width, x, y, 0, 0, r, xy_minus_r);
}
// the same, x[q] / y[q] written to the device addresses x_dst[q] / y_dst[q] (host arrays of device pointers)
extern "C" int lgc_ti_generate_scatter(int device, const uint8_t seed[16], uint64_t first_pair, size_t npairs, size_t n, int width,
                                       void *const *x_dst, void *const *y_dst, uint64_t *r, uint64_t *xy_minus_r) {
    if (!x_dst || !y_dst || !seed || !r || !xy_minus_r) return lgc_fail(LGC_EINVAL, "null argument");
    if (width != 32 && width != 64) return lgc_fail(LGC_EINVAL, "width must be 32 or 64");
    if (npairs == 0) return LGC_OK;
    int rc = lgc_need_device(device);
    if (rc) return rc;
    // keystream -> destinations -> <x, y>: three kernels on grow-only per-thread scratch, no allocation per batch
    AesTables t;
    aes_build_tables(t, seed);
    const size_t wb = width / 8;
    const uint64_t words_per_pair = 2 * n + 1;
    const uint64_t byte0 = first_pair * words_per_pair * wb, byte1 = (first_pair + npairs) * words_per_pair * wb;
    const uint64_t blk0 = byte0 / 16, blk1 = (byte1 + 15) / 16;
    char *small = 0; uint4 *dks = 0;
    const size_t ptr_bytes = 2 * npairs * sizeof(void *), small_bytes = 256 + ptr_bytes + 2 * npairs * 8;
    P1CHK(t_scratch.get(device, 0, small_bytes, (void **)&small));
    P1CHK(t_scratch.get(device, 1, (blk1 - blk0) * 16, (void **)&dks));
    uint32_t *drk = reinterpret_cast<uint32_t *>(small);
    uint64_t **dptr = reinterpret_cast<uint64_t **>(small + 256);
    uint64_t *dr = reinterpret_cast<uint64_t *>(small + 256 + ptr_bytes), *dout = dr + npairs;
    P1CHK(hipMemcpyAsync(drk, t.rk, sizeof(t.rk), hipMemcpyHostToDevice, 0));
    P1CHK(hipMemcpyAsync(dptr, x_dst, npairs * sizeof(void *), hipMemcpyHostToDevice, 0));
    P1CHK(hipMemcpyAsync(dptr + npairs, y_dst, npairs * sizeof(void *), hipMemcpyHostToDevice, 0));
    P1CHK(hipMemsetAsync(dout, 0, npairs * 8, 0));
    hipLaunchKernelGGL(ti_prg_kernel, dim3(512), dim3(1024), 0, 0, drk, blk0, blk1 - blk0, dks);
    P1CHK(hipGetLastError());
    const char *ks0 = reinterpret_cast<const char *>(dks) + (byte0 - blk0 * 16);
    unsigned gx = (unsigned)((2 * n + 1 + 255) / 256); if (gx > 128) gx = 128;
    unsigned gy = npairs > 65535 ? 65535u : (unsigned)npairs;
    if (wb == 8) hipLaunchKernelGGL((ti_unpack_scatter_kernel<uint64_t>), dim3(gx, gy), dim3(256), 0, 0, (const uint64_t *)ks0, npairs, n, dptr, dptr + npairs, dr);
    else hipLaunchKernelGGL((ti_unpack_scatter_kernel<uint32_t>), dim3(gx, gy), dim3(256), 0, 0, (const uint32_t *)ks0, npairs, n, dptr, dptr + npairs, dr);
    unsigned gd = (unsigned)((n + 255) / 256); if (gd > 64) gd = 64;
    hipLaunchKernelGGL(p1_dot_ptr_kernel, dim3(gd, gy), dim3(256), 0, 0, dptr, dptr + npairs, npairs, n, dout);
    P1CHK(hipGetLastError());
    P1CHK(hipMemcpy(r, dr, npairs * 8, hipMemcpyDeviceToHost));
    P1CHK(hipMemcpy(xy_minus_r, dout, npairs * 8, hipMemcpyDeviceToHost));
    const uint64_t m = maskw(width);
    for (size_t q = 0; q < npairs; q++) xy_minus_r[q] = (xy_minus_r[q] - r[q]) & m;
    return LGC_OK;
}

// =============================================================== matrix-triple mode (include/linreg_gc_p1_matrix.h)
// One triple (R_a, R_b, S; T = R_a^T R_b - S) per pair of providers.  The keystreams are expanded by ti_prg_kernel into the
// per-thread scratch first and read from there as row-major matrices of W-bit words (a block of the stream IS 16 bytes of
// little-endian words, so there is nothing to unpack); the cross products are p1_cross_kernel, one finishing launch adds S or
// T and masks.  Scratch slots: 0 = round keys and column lists, 1 and 2 = the two operands, 3 = C and what is added to it.
#include "p1_matrix_seeds.h"
static size_t p1_up(size_t bytes, size_t to) { return (bytes + to - 1) / to * to; }
enum { kP1MaxBlockCols = 1 << 20 };
// the keystream of `seed`, blocks 0 .. ceil(bytes / 16) - 1, at dst (room for whole blocks); drk: 44 words of device scratch,
// t: host tables that must outlive the stream's work
static hipError_t p1_keystream(AesTables &t, const uint8_t seed[16], uint32_t *drk, size_t bytes, void *dst, hipStream_t st) {
    aes_build_tables(t, seed);
    hipError_t e = hipMemcpyAsync(drk, t.rk, sizeof(t.rk), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    const uint64_t nblocks = (bytes + 15) / 16;
    unsigned g = (unsigned)((nblocks + 1023) / 1024); if (g > 512) g = 512;
    hipLaunchKernelGGL(ti_prg_kernel, dim3(g), dim3(1024), 0, st, drk, (uint64_t)0, nblocks, (uint4 *)dst);
    return hipGetLastError();
}
// dC (a x b words, zeroed by the caller) += P^T Q over n rows: p1_cross_kernel over ceil(a / 64) x ceil(b / 64) tiles and the
// splits of p1_split_k
template <typename TP, typename TQ>
static int p1_cross_block(const TP *P, size_t ldp, const uint32_t *pcols, uint32_t a, const TQ *Q, size_t ldq, const uint32_t *qcols,
                          uint32_t b, size_t n, uint64_t *dC, hipStream_t st) {
    const uint32_t at = (a + 63) / 64, bt = (b + 63) / 64;
    size_t kchunk;
    const size_t ksplit = p1_split_k((size_t)at * bt, n, &kchunk);
    if (ksplit > 65535) return lgc_fail(LGC_EINVAL, "internal: %zu row splits", ksplit);
    hipLaunchKernelGGL((p1_cross_kernel<TP, TQ>), dim3(at, bt, (unsigned)ksplit), dim3(256), 0, st, P, ldp, pcols, a, Q, ldq, qcols, b, n, dC,
                       kchunk);
    P1CHK(hipGetLastError());
    return LGC_OK;
}
template <typename TW, typename TO>
static void p1_cross_finish(const uint64_t *dC, const TW *add, int sign, size_t count, uint64_t m, TO *out, hipStream_t st) {
    unsigned g = (unsigned)((count + 255) / 256); if (g > 1024) g = 1024;
    hipLaunchKernelGGL((p1_cross_finish_kernel<TW, TO>), dim3(g), dim3(256), 0, st, dC, add, sign, count, m, out);
}
// a column list of a matrix call: every index <= d, and d only when y is set
static int p1_matrix_cols(const lgc_p1 *h, const uint32_t *cols, size_t ncols) {
    if (ncols > kP1MaxBlockCols) return lgc_fail(LGC_EINVAL, "a column block takes at most %d columns", (int)kP1MaxBlockCols);
    for (size_t i = 0; i < ncols; i++) {
        if (cols[i] > h->d) return lgc_fail(LGC_EINVAL, "column %u out of range (d = %zu)", cols[i], h->d);
        if (cols[i] == h->d && !h->have_y) return lgc_fail(LGC_EINVAL, "column d is y, and y is not set");
    }
    return LGC_OK;
}

template <typename TW>
static int p1_matrix_mask(lgc_p1 *h, const uint32_t *cols, size_t ncols, const uint8_t seed[16], void *out_E) {
    P1CHK(hipSetDevice(h->device));
    P1Serial serial_; hipStream_t st = p1_stream();
    const size_t words = h->n * ncols, bytes = words * sizeof(TW);
    char *small = 0; TW *dR = 0, *dE = 0;
    P1CHK(t_scratch.get(h->device, 0, 256 + ncols * sizeof(uint32_t), (void **)&small));
    P1CHK(t_scratch.get(h->device, 1, p1_up(bytes, 16), (void **)&dR));
    if (h->dev_io) dE = (TW *)out_E;
    else P1CHK(t_scratch.get(h->device, 2, bytes, (void **)&dE));
    uint32_t *dcols = (uint32_t *)(small + 256);
    AesTables t;
    P1CHK(hipMemcpyAsync(dcols, cols, ncols * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    P1CHK(p1_keystream(t, seed, (uint32_t *)small, bytes, dR, st));
    unsigned g = (unsigned)((words + 255) / 256); if (g > 4096) g = 4096;
    hipLaunchKernelGGL((p1_matrix_mask_kernel<TW>), dim3(g), dim3(256), 0, st, h->X, h->n, h->ld(), dcols, (uint32_t)ncols, dR, dE, maskw(h->w));
    P1CHK(hipGetLastError());
    if (!h->dev_io) P1CHK(hipMemcpyAsync(out_E, dE, bytes, hipMemcpyDeviceToHost, st));
    P1CHK(hipStreamSynchronize(st));
    return LGC_OK;
}
extern "C" int lgc_p1_matrix_mask(lgc_p1 *h, const uint32_t *cols, size_t ncols, const uint8_t seed[16], void *out_E) {
    if (!h || !cols || !seed || !out_E) return lgc_fail(LGC_EINVAL, "null argument");
    int rc = p1_matrix_cols(h, cols, ncols);
    if (rc) return rc;
    if (ncols == 0) return LGC_OK;
    return h->w == 32 ? p1_matrix_mask<uint32_t>(h, cols, ncols, seed, out_E) : p1_matrix_mask<uint64_t>(h, cols, ncols, seed, out_E);
}

template <typename TW>
static int p1_matrix_share_a(lgc_p1 *h, size_t a, const uint8_t seed_a[16], const uint8_t seed_s[16], const void *F, size_t b, uint64_t *out) {
    P1CHK(hipSetDevice(h->device));
    P1Serial serial_; hipStream_t st = p1_stream();
    const size_t n = h->n, cwords = a * b, cbytes = p1_up(cwords * sizeof(uint64_t), 256);
    char *small = 0, *cs = 0; TW *dR = 0; const TW *dF = (const TW *)F;
    P1CHK(t_scratch.get(h->device, 0, 512, (void **)&small));
    P1CHK(t_scratch.get(h->device, 1, p1_up(n * a * sizeof(TW), 16), (void **)&dR));
    P1CHK(t_scratch.get(h->device, 3, cbytes + p1_up(cwords * sizeof(TW), 16), (void **)&cs));
    if (!h->dev_io) {
        TW *up = 0;
        P1CHK(t_scratch.get(h->device, 2, n * b * sizeof(TW), (void **)&up));
        P1CHK(hipMemcpyAsync(up, F, n * b * sizeof(TW), hipMemcpyHostToDevice, st));
        dF = up;
    }
    uint64_t *dC = (uint64_t *)cs;
    TW *dS = (TW *)(cs + cbytes);
    AesTables ta, ts;
    P1CHK(hipMemsetAsync(dC, 0, cwords * sizeof(uint64_t), st));
    P1CHK(p1_keystream(ta, seed_a, (uint32_t *)small, n * a * sizeof(TW), dR, st));
    P1CHK(p1_keystream(ts, seed_s, (uint32_t *)(small + 256), cwords * sizeof(TW), dS, st));
    int rc = p1_cross_block<TW, TW>(dR, a, 0, (uint32_t)a, dF, b, 0, (uint32_t)b, n, dC, st);
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    p1_cross_finish<TW, uint64_t>(dC, dS, +1, cwords, maskw(h->w), dC, st);
    P1CHK(hipGetLastError());
    P1CHK(hipMemcpyAsync(out, dC, cwords * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    P1CHK(hipStreamSynchronize(st));
    return LGC_OK;
}
extern "C" int lgc_p1_matrix_share_a(lgc_p1 *h, size_t ncols_a, const uint8_t seed_a[16], const uint8_t seed_s[16], const void *F,
                                     size_t ncols_b, uint64_t *out) {
    if (!h || !seed_a || !seed_s || !F || !out) return lgc_fail(LGC_EINVAL, "null argument");
    if (ncols_a > kP1MaxBlockCols || ncols_b > kP1MaxBlockCols) return lgc_fail(LGC_EINVAL, "a column block takes at most %d columns", (int)kP1MaxBlockCols);
    if (ncols_a == 0 || ncols_b == 0) return LGC_OK;
    return h->w == 32 ? p1_matrix_share_a<uint32_t>(h, ncols_a, seed_a, seed_s, F, ncols_b, out)
                      : p1_matrix_share_a<uint64_t>(h, ncols_a, seed_a, seed_s, F, ncols_b, out);
}

template <typename TW>
static int p1_matrix_share_b(lgc_p1 *h, const uint32_t *cols_b, size_t b, const void *E, size_t a, const void *T, uint64_t *out) {
    P1CHK(hipSetDevice(h->device));
    P1Serial serial_; hipStream_t st = p1_stream();
    const size_t n = h->n, cwords = a * b, cbytes = p1_up(cwords * sizeof(uint64_t), 256);
    uint32_t *dcols = 0; char *cs = 0; const TW *dE = (const TW *)E;
    P1CHK(t_scratch.get(h->device, 0, b * sizeof(uint32_t), (void **)&dcols));
    P1CHK(t_scratch.get(h->device, 3, cbytes + cwords * sizeof(TW), (void **)&cs));
    if (!h->dev_io) {
        TW *up = 0;
        P1CHK(t_scratch.get(h->device, 1, n * a * sizeof(TW), (void **)&up));
        P1CHK(hipMemcpyAsync(up, E, n * a * sizeof(TW), hipMemcpyHostToDevice, st));
        dE = up;
    }
    uint64_t *dC = (uint64_t *)cs;
    TW *dT = (TW *)(cs + cbytes);
    P1CHK(hipMemcpyAsync(dcols, cols_b, b * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    P1CHK(hipMemcpyAsync(dT, T, cwords * sizeof(TW), hipMemcpyHostToDevice, st));
    P1CHK(hipMemsetAsync(dC, 0, cwords * sizeof(uint64_t), st));
    int rc = p1_cross_block<TW, int64_t>(dE, a, 0, (uint32_t)a, h->X, h->ld(), dcols, (uint32_t)b, n, dC, st);
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    p1_cross_finish<TW, uint64_t>(dC, dT, +1, cwords, maskw(h->w), dC, st);
    P1CHK(hipGetLastError());
    P1CHK(hipMemcpyAsync(out, dC, cwords * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    P1CHK(hipStreamSynchronize(st));
    return LGC_OK;
}
extern "C" int lgc_p1_matrix_share_b(lgc_p1 *h, const uint32_t *cols_b, size_t ncols_b, const void *E, size_t ncols_a, const void *T,
                                     uint64_t *out) {
    if (!h || !cols_b || !E || !T || !out) return lgc_fail(LGC_EINVAL, "null argument");
    if (ncols_a > kP1MaxBlockCols) return lgc_fail(LGC_EINVAL, "a column block takes at most %d columns", (int)kP1MaxBlockCols);
    int rc = p1_matrix_cols(h, cols_b, ncols_b);
    if (rc) return rc;
    if (ncols_a == 0 || ncols_b == 0) return LGC_OK;
    return h->w == 32 ? p1_matrix_share_b<uint32_t>(h, cols_b, ncols_b, E, ncols_a, T, out)
                      : p1_matrix_share_b<uint64_t>(h, cols_b, ncols_b, E, ncols_a, T, out);
}

// the initializer's T = (R_a^T R_b - S) & m: three streams, one cross product, one subtraction
template <typename TW>
static int ti_matrix_generate(int device, const uint8_t seed_a[16], const uint8_t seed_b[16], const uint8_t seed_s[16], size_t n, size_t a,
                              size_t b, int width, void *out_T) {
    P1CHK(hipSetDevice(device));
    P1Serial serial_; hipStream_t st = p1_stream();
    const size_t cwords = a * b, cbytes = p1_up(cwords * sizeof(uint64_t), 256), sbytes = p1_up(cwords * sizeof(TW), 256);
    char *small = 0, *cs = 0; TW *dRa = 0, *dRb = 0;
    P1CHK(t_scratch.get(device, 0, 768, (void **)&small));
    P1CHK(t_scratch.get(device, 1, p1_up(n * a * sizeof(TW), 16), (void **)&dRa));
    P1CHK(t_scratch.get(device, 2, p1_up(n * b * sizeof(TW), 16), (void **)&dRb));
    P1CHK(t_scratch.get(device, 3, cbytes + 2 * sbytes, (void **)&cs));
    uint64_t *dC = (uint64_t *)cs;
    TW *dS = (TW *)(cs + cbytes), *dT = (TW *)(cs + cbytes + sbytes);
    AesTables ta, tb, ts;
    P1CHK(hipMemsetAsync(dC, 0, cwords * sizeof(uint64_t), st));
    P1CHK(p1_keystream(ta, seed_a, (uint32_t *)small, n * a * sizeof(TW), dRa, st));
    P1CHK(p1_keystream(tb, seed_b, (uint32_t *)(small + 256), n * b * sizeof(TW), dRb, st));
    P1CHK(p1_keystream(ts, seed_s, (uint32_t *)(small + 512), cwords * sizeof(TW), dS, st));
    int rc = p1_cross_block<TW, TW>(dRa, a, 0, (uint32_t)a, dRb, b, 0, (uint32_t)b, n, dC, st);
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    p1_cross_finish<TW, TW>(dC, dS, -1, cwords, maskw(width), dT, st);
    P1CHK(hipGetLastError());
    P1CHK(hipMemcpyAsync(out_T, dT, cwords * sizeof(TW), hipMemcpyDeviceToHost, st));
    P1CHK(hipStreamSynchronize(st));
    return LGC_OK;
}
extern "C" int lgc_ti_matrix_generate(int device, const uint8_t seed_a[16], const uint8_t seed_b[16], const uint8_t seed_s[16], size_t n,
                                      size_t a, size_t b, int width, void *out_T) {
    if (!seed_a || !seed_b || !seed_s || !out_T) return lgc_fail(LGC_EINVAL, "null argument");
    if (width != 32 && width != 64) return lgc_fail(LGC_EINVAL, "width must be 32 or 64");
    if (n < 1) return lgc_fail(LGC_EINVAL, "empty data");
    if (a > kP1MaxBlockCols || b > kP1MaxBlockCols) return lgc_fail(LGC_EINVAL, "a column block takes at most %d columns", (int)kP1MaxBlockCols);
    if (a == 0 || b == 0) return LGC_OK;
    int rc = lgc_need_device(device);
    if (rc) return rc;
    return width == 32 ? ti_matrix_generate<uint32_t>(device, seed_a, seed_b, seed_s, n, a, b, width, out_T)
                       : ti_matrix_generate<uint64_t>(device, seed_a, seed_b, seed_s, n, a, b, width, out_T);
}
// blocks 3u, 3u + 1, 3u + 2 of the master seed's keystream, on the host
extern "C" int lgc_ti_matrix_seeds(const uint8_t master[16], uint64_t u, uint8_t seed_a[16], uint8_t seed_b[16], uint8_t seed_s[16]) {
    if (!master || !seed_a || !seed_b || !seed_s) return lgc_fail(LGC_EINVAL, "null argument");
    if (u > (~0ull - 2) / 3) return lgc_fail(LGC_EINVAL, "instance number out of range");
    p1_matrix_seeds(master, u, seed_a, seed_b, seed_s);
    return LGC_OK;
}
