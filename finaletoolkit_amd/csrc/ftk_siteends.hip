// Fragment-end profiles around sites (ftk_site_ends): the rule of ftk_site_profile with two events per fragment on two
// tracks.  A fragment [start, end) that passes the MAPQ / length rule and holds a base has its U end on base `start` and
// its D end on base `end - 1`.  An end at x with d = x - c in [-H, H) of a site counts in bin (d + H) / b of track 0 (U)
// or 1 (D) of the site's group - bin n_bins - 1 - k of the OTHER track for a flipped site.  Per site, and in genome
// orientation (no flip), the ends inside [-p - w, -p + w] and [p - w, p + w] are summed too: left_up, left_down, right_up,
// right_down.  Sums and counts are integers, so no result depends on the order of arrival.
//
// One candidate range serves both ends: [index_bound(c - H - lmax), index_bound(c + H, 1)), the midpoint kernel's.  The
// index is sorted by start.  A U end in the window has c - H <= start < c + H.  A D end in the window has c - H <= end - 1
// < c + H; the fragment holds a base, so start <= end - 1 < c + H, and it is no longer than lmax, so start = end - len >=
// c - H + 1 - lmax.  Either way c - H - lmax <= start < c + H, which is what the two index bounds enclose.
//
// site_ends_kernel  one workgroup per RUN of sites (the runs of site_profile_kernel: sites sorted by (group, centre), cut
//                   inside a group) and, when the launch is split, per TRACK (blockIdx.y).  The run's tracks live in
//                   LDS: per track n_bins 32-bit counts and, with weights, n_bins 64-bit sums in front of them (4 or
//                   12 bytes per bin; both tracks of 4096 weighted bins take 96 KiB: above a threshold the launch is
//                   split, and for whole launches above 64 KiB the kernel's dynamic-LDS limit is raised,
//                   ftk_siteends.h).  The scan is the shared one of ftk_sitescan.h: a wave takes one site at a time and
//                   its lanes stride over the site's candidates.  The predicate is branch-free and each end's bin is
//                   the integer quotient (quot).  An end in the window adds to its bin with LDS atomics.  With SITES
//                   the four window counts (and, weighted, four 64-bit sums) of the wave's site stay in registers per
//                   lane over the candidate loop (locals that the scan's lambda captures by reference), are summed
//                   across the wave once per site, and lane 0 writes them with plain stores to the row of the site's
//                   place in the caller's list (order[]): no atomics, so they are deterministic.  A split workgroup
//                   handles one end of every site (the one that lands in its track: U for track 0 of an unflipped site,
//                   D of a flipped one) and writes that end's two columns.  At the end of the run the non-zero bins go
//                   to the zeroed outputs of the run's group.
//
// The 32-bit LDS counts cannot wrap under site_run_sites_of's bound per_run <= (2^32 - 1) / n_frag: a fragment has one U
// end and one D end, a site sends all its U ends to one track and all its D ends to the other, so although a site may
// add 2 n_frag to its group's two tracks together it adds at most n_frag to any ONE bin - a length-1 fragment, whose two
// ends share a base, adds to the same bin NUMBER of two different tracks, two different LDS words.  per_run sites add at
// most per_run * n_frag <= 2^32 - 1 to a bin.  The per-lane site counts see a candidate once: below n_frag < 2^31.
#include <algorithm>

#include "ftk_sitescan.h"
#include "ftk_siteends.h"

namespace ftk {

namespace {

template <bool WEIGHTED, bool SITES>
__global__ __launch_bounds__(kSiteThreads) void site_ends_kernel(ContigView cv, const uint32_t* __restrict__ weights,
                                                                 const uint32_t* __restrict__ site,
                                                                 const int32_t* __restrict__ order,
                                                                 const int32_t* __restrict__ run_off,
                                                                 const int32_t* __restrict__ run_group, SiteEndsParams p,
                                                                 unsigned long long* __restrict__ sum_out,
                                                                 unsigned long long* __restrict__ cnt_out,
                                                                 unsigned long long* __restrict__ site_sum,
                                                                 unsigned long long* __restrict__ site_cnt) {
    extern __shared__ unsigned long long ends_s[];  // WEIGHTED: cells sums, then as many counts; else the counts alone
    const int cells = (p.split ? 1 : 2) * p.n_bins;  // what the launch gave the block: track 0's bins, then track 1's
    unsigned int* cnt_s = reinterpret_cast<unsigned int*>(WEIGHTED ? ends_s + cells : ends_s);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int only = p.split ? (int)blockIdx.y : -1;  // the one track this workgroup holds (gridDim.y == 2), or both
    site_cells_clear<WEIGHTED>(ends_s, cnt_s, cells);
    const int s0 = run_off[blockIdx.x], s1 = run_off[blockIdx.x + 1];
    const int H = p.half_width, b = p.bin_size;
    const float rinv = 1.0f / (float)b;
    const int near = p.peak - p.flank;              // >= 1
    const unsigned span = 2u * (unsigned)p.flank;   // |d -+ peak| <= flank  <=>  (unsigned)(+-d - near) <= span
    for (int si = s0 + wv; si < s1; si += kSiteThreads / 64) {
        const uint32_t word = site[si];
        const int c = (int)(word & ~kSiteFlipBit);
        const int flip = (word & kSiteFlipBit) ? 1 : 0;
        // the tracks of the two ends at this site, and which of them this workgroup takes
        const int tr_u = flip, tr_d = flip ^ 1;
        const bool do_u = only < 0 || only == tr_u, do_d = only < 0 || only == tr_d;
        const int off_u = only < 0 ? tr_u * p.n_bins : 0, off_d = only < 0 ? tr_d * p.n_bins : 0;
        unsigned int wc[4] = {0u, 0u, 0u, 0u};             // left_up, left_down, right_up, right_down of this lane
        unsigned long long ws[4] = {0ull, 0ull, 0ull, 0ull};
        site_scan<WEIGHTED>(cv, weights, c, H, p.lmax, lane, [&](bool valid, int fs, int fe, int q, uint32_t wt) {
            const int len = fe - fs;
            const bool pass = valid & (q >= p.mapq_min) & (len >= p.min_len) & (len <= p.max_len) & (len >= 1);
            const int du = fs - c, dd = fe - 1 - c;  // coordinates < 2^30: no overflow
            const bool ok_u = pass & (du >= -H) & (du < H) & do_u;
            const bool ok_d = pass & (dd >= -H) & (dd < H) & do_d;
            int ku = quot(ok_u ? du + H : 0, b, rinv);  // 0 <= x < 2 H <= 2^21
            int kd = quot(ok_d ? dd + H : 0, b, rinv);
            if (flip) {
                ku = p.n_bins - 1 - ku;
                kd = p.n_bins - 1 - kd;
            }
            ku += off_u;  // 0 <= ku, kd < n_bins where the end counts: its cell of the workgroup's tracks
            kd += off_d;
            if (ok_u) {
                atomicAdd(&cnt_s[ku], 1u);
                if (WEIGHTED) atomicAdd(&ends_s[ku], (unsigned long long)wt);
            }
            if (ok_d) {
                atomicAdd(&cnt_s[kd], 1u);
                if (WEIGHTED) atomicAdd(&ends_s[kd], (unsigned long long)wt);
            }
            if (SITES) {  // (peak + flank < H: an end inside a window is inside [-H, H))
                const unsigned lu = (unsigned)(-du - near) <= span, ld = (unsigned)(-dd - near) <= span;
                const unsigned ru = (unsigned)(du - near) <= span, rd = (unsigned)(dd - near) <= span;
                const unsigned in[4] = {lu & (unsigned)ok_u, ld & (unsigned)ok_d, ru & (unsigned)ok_u, rd & (unsigned)ok_d};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    wc[j] += in[j];
                    if (WEIGHTED) ws[j] += in[j] ? (unsigned long long)wt : 0ull;
                }
            }
        });
        if (SITES) {
            const size_t row = (size_t)order[si] * 4;  // the site's place in the caller's list
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned long long n = wave_sum_u32(wc[j]);
                const unsigned long long w = WEIGHTED ? wave_sum_u64(ws[j]) : n * FTK_WEIGHT_ONE;
                if (lane == 0 && ((j & 1) ? do_d : do_u)) {
                    site_sum[row + j] = w;
                    if (site_cnt) site_cnt[row + j] = n;
                }
            }
        }
    }
    // the group's two tracks lie behind one another: cell t * n_bins + k of a whole run, k of track `only` of a split one
    const size_t first = ((size_t)run_group[blockIdx.x] * 2 + (size_t)(only < 0 ? 0 : only)) * (size_t)p.n_bins;
    site_cells_flush<WEIGHTED>(ends_s, cnt_s, cells, first, sum_out, cnt_out);
}

}  // namespace

hipError_t siteends_lds_most(int device, int* most_out) {  // (the unweighted kernels take 32 KiB at most)
    return site_lds_limit(device, kSiteEndsLdsMost,
                          {reinterpret_cast<const void*>(&site_ends_kernel<true, false>),
                           reinterpret_cast<const void*>(&site_ends_kernel<true, true>)},
                          most_out);
}

long long siteends_run_sites(int n_cu, long long n_sites, long long n_frag, int max_end, const SiteEndsParams& p) {
    return site_run_sites_of(n_cu, n_sites, n_frag, max_end, p.half_width, p.lmax, kSiteRunCandidates, p.split ? 2 : 1);
}

void launch_site_ends(hipStream_t s, const ContigView& cv, const uint32_t* weights, const uint32_t* site, const int32_t* order,
                      const int32_t* run_off, const int32_t* run_group, int n_runs, const SiteEndsParams& p, unsigned long long* sum,
                      unsigned long long* cnt, unsigned long long* site_sum, unsigned long long* site_cnt) {
    if (n_runs <= 0 || cv.n <= 0) return;
    const dim3 grid((unsigned)n_runs, p.split ? 2u : 1u);
    const size_t lds = siteends_lds(p);
#define FTK_ENDS_LAUNCH(W, S)                                                                                                       \
    hipLaunchKernelGGL((site_ends_kernel<W, S>), grid, dim3(kSiteThreads), lds, s, cv, weights, site, order, run_off, run_group, p, \
                       sum, cnt, site_sum, site_cnt)
    if (p.weighted) {
        if (site_sum) FTK_ENDS_LAUNCH(true, true); else FTK_ENDS_LAUNCH(true, false);
    } else {
        if (site_sum) FTK_ENDS_LAUNCH(false, true); else FTK_ENDS_LAUNCH(false, false);
    }
#undef FTK_ENDS_LAUNCH
}

}  // namespace ftk
