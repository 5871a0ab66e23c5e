// Launcher of the V-plot kernel in ftk_vplot.hip (internal).
#pragma once

#include "ftk_siteprofile.h"

namespace ftk {

// The LDS a workgroup's tile of the matrix may take (the device's per-workgroup limit where that is smaller) - a larger
// tile reads the candidates fewer times, a smaller one lets a compute unit hold more workgroups - and the candidates a
// run of sites should hold before its tile is flushed: a V-plot run flushes up to tile_rows * n_bins cells where a
// profile run flushes n_bins, so it has a constant of its own.  Both chosen on the MI355X (32 KiB beat 64 KiB and the
// device's 160 KiB; 16 x 4096 candidates beat 4 x 4096 and equalled 64 x 4096): docs/experiments.md, "V-plot".
#ifndef FTK_VPLOT_LDS_BYTES
#define FTK_VPLOT_LDS_BYTES (32 << 10)
#endif
#ifndef FTK_VPLOT_RUN_CANDIDATES
#define FTK_VPLOT_RUN_CANDIDATES (16 * 4096)
#endif
constexpr int kVplotLdsBytes = FTK_VPLOT_LDS_BYTES;
constexpr long long kVplotRunCandidates = FTK_VPLOT_RUN_CANDIDATES;
constexpr int kVplotMaxRows = 4096;
constexpr int kVplotMaxLen = (1 << 16) - 1;  // L - len_lo < 2^16: exact in the float the row's quotient is estimated in
static_assert(kVplotLdsBytes >= 4 * kSiteMaxBins, "an unweighted row of the widest matrix has to fit the budget");

struct VplotParams {
    int half_width, bin_size, n_bins;  // n_bins = 2 * half_width / bin_size <= kSiteMaxBins
    int len_lo, len_hi, len_bin;       // closed bounds; n_rows = (len_hi - len_lo + 1) / len_bin <= kVplotMaxRows
    int n_rows, tile_rows;             // rows of the matrix, and of one workgroup's tile of it (the last may hold fewer)
    int mapq_min;
    int contig_lmax;                   // longest fragment of the contig
    int weighted;                      // 1: sum the weight column; 0: every fragment weighs FTK_WEIGHT_ONE
};

// Bytes of LDS per cell, rows per tile under a budget of `lds_bytes` (one row at least: the widest weighted row, 4096 bins
// x 12 B = 48 KiB, is within any device's limit and may exceed a smaller budget), tiles per run, LDS of one workgroup.
inline int vplot_cell_bytes(bool weighted) { return weighted ? 12 : 4; }
inline int vplot_tile_rows(int lds_bytes, int n_rows, int n_bins, bool weighted) {
    const int fit = lds_bytes / (vplot_cell_bytes(weighted) * n_bins);
    return fit < 1 ? 1 : (fit < n_rows ? fit : n_rows);
}
inline int vplot_tiles(const VplotParams& p) { return (p.n_rows + p.tile_rows - 1) / p.tile_rows; }
inline size_t vplot_lds(const VplotParams& p) { return (size_t)p.tile_rows * p.n_bins * vplot_cell_bytes(p.weighted != 0); }

// The budget of this device: min(kVplotLdsBytes, the device's LDS per workgroup); above 64 KiB the kernels' dynamic-LDS
// limit is raised to it.  Once per context (the caller keeps the result).
hipError_t vplot_lds_budget(int device, int* budget_out);

// Sites the runs of one call may hold each (site_run_sites_of with the V-plot's constant; a run is vplot_tiles(p) workgroups).
long long vplot_run_sites(int n_cu, long long n_sites, long long n_frag, int max_end, const VplotParams& p);

// Runs as for launch_site_profile; gridDim.y runs over the tiles of rows.  sum[(run_group[r] * n_rows + row) * n_bins +
// k] and cnt[...] (may be NULL) += the run's matrix; both zeroed by the caller.  n_runs * vplot_tiles(p) <=
// kSiteMaxRunsPerLaunch, n_runs >= 1, cv.n >= 1; vplot_lds(p) within the budget.
void launch_site_vplot(hipStream_t s, const ContigView& cv, const uint32_t* weights, const uint32_t* site, const int32_t* run_off,
                       const int32_t* run_group, int n_runs, const VplotParams& p, unsigned long long* sum, unsigned long long* cnt);

}  // namespace ftk
