// Fragment length x midpoint offset maps around sites (ftk_site_vplot): the rule of ftk_site_profile with a second
// axis.  A fragment that passes the MAPQ rule with a length L in [len_lo, len_hi], and whose midpoint m = (start + end)
// >> 1 lies in [c - H, c + H) of a site, counts in row (L - len_lo) / len_bin and column (m - c + H) / b of the site's
// group - column n_bins - 1 - k for a flipped site; the flip never touches the row.  Sums and counts are integers, so no
// result depends on the order of arrival.
//
// site_vplot_kernel  one workgroup per (RUN of sites, TILE of rows).  The runs are those of site_profile_kernel (sites
//                    sorted by (group, centre), cut inside a group); the tile is tile_rows x n_bins cells in LDS: a
//                    32-bit count per cell, and with weights a 64-bit sum in front of it (4 or 12 bytes per cell), as
//                    many rows as the LDS budget holds (ftk_vplot.h).  blockIdx.y is the tile; the last one may hold
//                    fewer rows.  A tile takes only the lengths of its own rows, so its candidate range reaches back by
//                    its own longest passing length - min(contig's longest, the tile's last length) - and the tiles of
//                    short rows read less.  Inside, the scan is the shared one of ftk_sitescan.h: a wave takes one
//                    site at a time and its lanes stride over the site's candidates.  The predicate is branch-free, and
//                    both the row and the column are integer quotients (quot: L - len_lo < 2^16 and d + H < 2^21).  A
//                    passing candidate adds to its cell with LDS atomics.  At the end of the run the non-zero cells go
//                    to the zeroed outputs.
#include <algorithm>

#include "ftk_sitescan.h"
#include "ftk_vplot.h"

namespace ftk {

namespace {

template <bool WEIGHTED>
__global__ __launch_bounds__(kSiteThreads) void site_vplot_kernel(ContigView cv, const uint32_t* __restrict__ weights,
                                                                  const uint32_t* __restrict__ site,
                                                                  const int32_t* __restrict__ run_off,
                                                                  const int32_t* __restrict__ run_group, VplotParams p,
                                                                  unsigned long long* __restrict__ sum_out,
                                                                  unsigned long long* __restrict__ cnt_out) {
    extern __shared__ unsigned long long vp_s[];  // WEIGHTED: tile_rows * n_bins sums, then as many counts; else the counts alone
    unsigned int* cnt_s = reinterpret_cast<unsigned int*>(WEIGHTED ? vp_s + p.tile_rows * p.n_bins : vp_s);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int row0 = (int)blockIdx.y * p.tile_rows;              // < n_rows: the grid holds ceil(n_rows / tile_rows) tiles
    const int rows = min(p.tile_rows, p.n_rows - row0);
    const int cells = rows * p.n_bins;                           // <= tile_rows * n_bins: what the launch gave the block
    const int tlo = p.len_lo + row0 * p.len_bin, thi = tlo + rows * p.len_bin - 1;  // the tile's lengths: len_lo <= tlo <= thi <= len_hi
    const int lmax = min(p.contig_lmax, thi);                    // the longest fragment that can pass in this tile
    if (lmax < tlo) return;                                      // (the whole block: the contig has no fragment this long)
    site_cells_clear<WEIGHTED>(vp_s, cnt_s, cells);
    const int s0 = run_off[blockIdx.x], s1 = run_off[blockIdx.x + 1];
    const int H = p.half_width, b = p.bin_size, lb = p.len_bin;
    const float rinv = 1.0f / (float)b, linv = 1.0f / (float)lb;
    for (int si = s0 + wv; si < s1; si += kSiteThreads / 64) {
        const uint32_t word = site[si];
        const int c = (int)(word & ~kSiteFlipBit);
        const bool flip = (word & kSiteFlipBit) != 0;
        site_scan<WEIGHTED>(cv, weights, c, H, lmax, lane, [&](bool valid, int fs, int fe, int q, uint32_t wt) {
            const int len = fe - fs;
            const int mid = (int)(((unsigned)fs + (unsigned)fe) >> 1);  // coordinates < 2^30
            const int d = mid - c;
            const bool ok = valid & (q >= p.mapq_min) & (len >= tlo) & (len <= thi) & (d >= -H) & (d < H);
            int k = quot(ok ? d + H : 0, b, rinv);           // 0 <= x < 2 H <= 2^21
            if (flip) k = p.n_bins - 1 - k;
            const int r = quot(ok ? len - tlo : 0, lb, linv);  // 0 <= y < rows * lb <= 2^16
            if (ok) {  // 0 <= r < rows, 0 <= k < n_bins
                const int cell = r * p.n_bins + k;
                atomicAdd(&cnt_s[cell], 1u);
                if (WEIGHTED) atomicAdd(&vp_s[cell], (unsigned long long)wt);
            }
        });
    }
    // the tile's rows lie behind one another in the group's matrix: cell (r, k) is output cell (row0 + r) * n_bins + k
    const size_t first = ((size_t)run_group[blockIdx.x] * (size_t)p.n_rows + (size_t)row0) * (size_t)p.n_bins;
    site_cells_flush<WEIGHTED>(vp_s, cnt_s, cells, first, sum_out, cnt_out);
}

}  // namespace

hipError_t vplot_lds_budget(int device, int* budget_out) {
    return site_lds_limit(device, kVplotLdsBytes,
                          {reinterpret_cast<const void*>(&site_vplot_kernel<true>), reinterpret_cast<const void*>(&site_vplot_kernel<false>)},
                          budget_out);
}

long long vplot_run_sites(int n_cu, long long n_sites, long long n_frag, int max_end, const VplotParams& p) {
    return site_run_sites_of(n_cu, n_sites, n_frag, max_end, p.half_width, std::min(p.contig_lmax, p.len_hi), kVplotRunCandidates,
                             vplot_tiles(p));
}

void launch_site_vplot(hipStream_t s, const ContigView& cv, const uint32_t* weights, const uint32_t* site, const int32_t* run_off,
                       const int32_t* run_group, int n_runs, const VplotParams& p, unsigned long long* sum, unsigned long long* cnt) {
    if (n_runs <= 0 || cv.n <= 0) return;
    const dim3 grid((unsigned)n_runs, (unsigned)vplot_tiles(p));
    if (p.weighted)
        hipLaunchKernelGGL(site_vplot_kernel<true>, grid, dim3(kSiteThreads), vplot_lds(p), s, cv, weights, site, run_off, run_group, p,
                           sum, cnt);
    else
        hipLaunchKernelGGL(site_vplot_kernel<false>, grid, dim3(kSiteThreads), vplot_lds(p), s, cv, weights, site, run_off, run_group,
                           p, sum, cnt);
}

}  // namespace ftk
