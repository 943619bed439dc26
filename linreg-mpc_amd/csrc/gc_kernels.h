// gc_kernels.h -- the kernel dispatch of a launch: included by gc_kern.hip only, which is compiled once per (role, kernel
// family) (csrc/Makefile) and exports the pieces as plain functions (declared in gc_launch.h).  Everything else in the
// library calls those.
#pragma once
#include <hip/hip_runtime.h>

#include "gc_device.h"
#include "gc_split.h"
#include "gc_launch.h"

namespace gc {

static inline hipError_t gc_launch_tabfill_impl(const Launch &L, const Lbl *stash, Lbl *tab, Lbl R, hipStream_t st) {
    const uint64_t per = kTpbTabfill / 64;
    uint64_t blocks = (L.steps + per - 1) / per;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL((gc_tabfill_kernel<kTpbTabfill>), dim3((unsigned)blocks), dim3(kTpbTabfill), 0, st, stash, tab,
                       (uint32_t)L.steps, L.step0, R);
    return hipGetLastError();
}

// the record kernel of a launch in mode `m` (garbler in a critical-path mode: `tab` is the stash)
// PART: which kernels this translation unit instantiates (gc_kern.hip): 0 = MAC, 1 = generic one wave per record (wide),
// 2 = column-split, 3 = generic 4 waves per record
template <bool G, int PART>
static inline hipError_t gc_launch_records_impl(LaunchMode m, const Rec *recs, const Launch &L, Lbl *words, uint64_t *dec, Lbl *tab, Lbl R, int w,
                                    int p, hipStream_t st) {
    switch (m) {
    case LM_NONE:
        return hipSuccess;
    case LM_MAC: if constexpr (PART == 0) {
        constexpr int TPB = G ? kTpbMacG : kTpbMacE;
        const LaunchShape sh = gc_launch_shape(m, G, L.nrec, gc_num_cus());
        hipLaunchKernelGGL((gc_mac_kernel<G, TPB>), dim3(sh.grid), dim3(sh.threads), 0, st, recs + L.first_rec, L.nrec, sh.per_wg,
                           words, tab, L.step0, R, w, p);
    } break;
    case LM_MACK: if constexpr (PART == 0) {
        constexpr int TPB = G ? kTpbMackG : kTpbMackE;
        const LaunchShape sh = gc_launch_shape(m, G, L.nrec, gc_num_cus());
        hipLaunchKernelGGL((gc_mack_kernel<G, TPB>), dim3(sh.grid), dim3(sh.threads), 0, st,
                           recs + L.first_rec, L.nrec, sh.per_wg, words, tab, L.step0, R, w, p);
    } break;
    case LM_WIDE: if constexpr (PART == 1) {
        const LaunchShape sh = gc_launch_shape(m, G, L.nrec, gc_num_cus());
        hipLaunchKernelGGL((gc_exec_kernel<G, false, 4, kTpbWide>), dim3(sh.grid), dim3(sh.threads), 0, st,
                           recs + L.first_rec, L.nrec, words, tab, dec, L.step0, R, w, p);
    } break;
    case LM_SPLIT:
        if constexpr (PART == 2) {
            const LaunchShape sh = gc_launch_shape(m, G, L.nrec, gc_num_cus());
            hipLaunchKernelGGL((gc_split_kernel<G>), dim3(sh.grid), dim3(sh.threads), 0, st, recs + L.first_rec, L.nrec, words, tab, dec,
                               L.step0, R, w, p);
        }
        break;
    case LM_SPLIT2:
        if constexpr (PART == 2) {
            const LaunchShape sh = gc_launch_shape(m, G, L.nrec, gc_num_cus());
            hipLaunchKernelGGL((gc_split_kernel<G, 2>), dim3(sh.grid), dim3(sh.threads), 0, st, recs + L.first_rec, L.nrec, words, tab, dec,
                               L.step0, R, w, p);
        }
        break;
    case LM_PAIRED: break;    // (not a mode)
    case LM_QUAD2:
        if constexpr (PART == 3) {
            const LaunchShape sh = gc_launch_shape(m, G, L.nrec, gc_num_cus());
            hipLaunchKernelGGL((gc_exec_kernel<G, true, 2, 256>), dim3(sh.grid), dim3(sh.threads), 0, st, recs + L.first_rec, L.nrec, words,
                               tab, dec, L.step0, R, w, p);
        }
        break;
    }
    return hipGetLastError();
}

}  // namespace gc
