// The scan the site kernels share (site_profile_kernel, site_vplot_kernel, site_ends_kernel; included by their .hip
// files only).  A workgroup holds the cells of one run of sites in LDS - 32-bit counts and, with weights, 64-bit sums -
// clears them (site_cells_clear), lets each of its waves take one site at a time and walk the site's candidates
// (site_scan), and at the end of the run adds the non-zero cells to the zeroed outputs (site_cells_flush).  What a
// candidate adds, and to which cell, is the kernel's own: it hands site_scan a lambda defined in the kernel, so the whole
// loop inlines and what the lambda captures by reference stays in registers.
#pragma once

#include "ftk_device.h"
#include "ftk_siteprofile.h"

namespace ftk {

// Loads in flight per lane and column in site_scan.
#ifndef FTK_SITE_UNROLL
#define FTK_SITE_UNROLL 4
#endif
constexpr int kSiteUnroll = FTK_SITE_UNROLL;

// The integer quotient x / b from its float estimate, rinv = 1.0f / (float)b.  0 <= x < 2^21 (kSiteMaxHalfWidth; the
// V-plot's rows: < 2^16) and 1 <= b: x is exact in float, and the two roundings (of 1 / b and of the product) move the
// estimate by less than x * 2^-22 / b < 1, so it is within one of the quotient and one step either way corrects it.
__device__ __forceinline__ int quot(int x, int b, float rinv) {
    int k = (int)((float)x * rinv);
    const int r = x - k * b;
    return k + (r >= b) - (r < 0);
}

// The candidates of the site at centre c, for fragments no longer than lmax whose event lies in [c - H, c + H): the
// range comes from the 512-bp index as weighted_window_kernel takes its own, [index_bound(c - H - lmax),
// index_bound(c + H, 1)).  The 64 lanes of the wave stride over it, kSiteUnroll loads in flight per lane and column,
// with coalesced reads of start, end and mapq (9 bytes per candidate; 13 with the weight, which is read only when
// WEIGHTED).  each(valid, start, end, mapq, weight) is called kSiteUnroll times per step by EVERY lane, so that it can
// stay branch-free: valid is false behind the range's end, where the other arguments are those of a fragment that is
// none of the lane's.
template <bool WEIGHTED, class Each>
__device__ __forceinline__ void site_scan(const ContigView& cv, const uint32_t* __restrict__ weights, int c, int H, int lmax, int lane,
                                          Each&& each) {
    const int lo = index_bound(cv, (long long)c - H - lmax, 0);
    int hi = index_bound(cv, (long long)c + H, 1);
    if (hi < lo) hi = lo;
    for (int base = lo; base < hi; base += 64 * kSiteUnroll) {
        int fs[kSiteUnroll], fe[kSiteUnroll], q[kSiteUnroll];
        uint32_t wt[kSiteUnroll];
        bool valid[kSiteUnroll];
#pragma unroll
        for (int u = 0; u < kSiteUnroll; ++u) {
            const int j = base + u * 64 + lane;  // (hi <= n < 2^31 - 1024: no overflow)
            valid[u] = j < hi;
            const int i = valid[u] ? j : base;  // (lo <= base < hi <= n: a fragment of the contig)
            fs[u] = cv.start[i];
            fe[u] = cv.end[i];
            q[u] = cv.mapq[i];
            wt[u] = WEIGHTED ? weights[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < kSiteUnroll; ++u) each(valid[u], fs[u], fe[u], q[u], wt[u]);
    }
}

// The workgroup's `cells` LDS cells - counts, and sums when WEIGHTED (sum_s is not touched otherwise) - set to zero ...
template <bool WEIGHTED>
__device__ __forceinline__ void site_cells_clear(unsigned long long* sum_s, unsigned int* cnt_s, int cells) {
    for (int k = threadIdx.x; k < cells; k += kSiteThreads) {
        if (WEIGHTED) sum_s[k] = 0;
        cnt_s[k] = 0;
    }
    __syncthreads();
}

// ... and, once every wave is through its sites, added to the outputs from cell `first` on: one 64-bit global atomic per
// non-zero cell and array.  Without weights the sum is the count times FTK_WEIGHT_ONE, and only the count was kept.
template <bool WEIGHTED>
__device__ __forceinline__ void site_cells_flush(const unsigned long long* sum_s, const unsigned int* cnt_s, int cells, size_t first,
                                                 unsigned long long* __restrict__ sum_out, unsigned long long* __restrict__ cnt_out) {
    __syncthreads();
    for (int k = threadIdx.x; k < cells; k += kSiteThreads) {
        const unsigned long long n = cnt_s[k];
        const unsigned long long w = WEIGHTED ? sum_s[k] : n * FTK_WEIGHT_ONE;
        if (w) atomicAdd(&sum_out[first + k], w);
        if (cnt_out && n) atomicAdd(&cnt_out[first + k], n);
    }
}

}  // namespace ftk
