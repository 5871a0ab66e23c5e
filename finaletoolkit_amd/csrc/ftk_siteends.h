// Launcher of the site-ends kernel in ftk_siteends.hip (internal).
#pragma once

#include "ftk_siteprofile.h"

namespace ftk {

// The LDS above which a run's two tracks no longer share one workgroup.  Both tracks of the widest weighted profile take
// 2 x 4096 bins x 12 B = 96 KiB, above the 64 KiB a kernel gets without asking.  At or below this threshold a run is ONE
// workgroup; above it a run is TWO workgroups, one per track (48 KiB each at most), and the candidates are read twice.
// Chosen on the MI355X: 96 KiB in one workgroup leaves a compute unit one workgroup of four waves, and the two passes
// beat it (docs/experiments.md, "site ends").  Every unweighted shape (32 KiB at most) and the weighted ones up to 2730
// bins stay whole.  The launcher still raises the weighted kernels' dynamic-LDS limit where the device has the room, so
// that a larger threshold - or FTK_SITE_ENDS_SPLIT=0 at run time - gets the one-workgroup arrangement.
#ifndef FTK_SITEENDS_LDS_BYTES
#define FTK_SITEENDS_LDS_BYTES (64 << 10)
#endif
constexpr int kSiteEndsLdsBytes = FTK_SITEENDS_LDS_BYTES;
constexpr int kSiteEndsLdsMost = 2 * 12 * kSiteMaxBins;  // both weighted tracks of the widest profile
static_assert(kSiteEndsLdsBytes >= 12 * kSiteMaxBins, "one weighted track of the widest profile has to fit the threshold");

struct SiteEndsParams {
    int half_width, bin_size, n_bins;  // n_bins = 2 * half_width / bin_size <= kSiteMaxBins
    int mapq_min, min_len, max_len;    // closed bounds (open ones: INT32_MIN / INT32_MAX)
    int lmax;                          // longest fragment that can pass
    int weighted;                      // 1: sum the weight column; 0: every fragment weighs FTK_WEIGHT_ONE
    int split;                         // 1: a run is two workgroups, one per track (blockIdx.y); 0: one holds both
    int peak, flank;                   // the per-site windows |d -+ peak| <= flank (read only with per-site outputs)
};

// Bytes of LDS per bin of one track, LDS of both tracks in one workgroup, LDS of one workgroup of the launch.
inline int siteends_bin_bytes(bool weighted) { return weighted ? 12 : 4; }
inline int siteends_whole_bytes(int n_bins, bool weighted) { return 2 * n_bins * siteends_bin_bytes(weighted); }
inline size_t siteends_lds(const SiteEndsParams& p) {
    return (size_t)(p.split ? 1 : 2) * p.n_bins * siteends_bin_bytes(p.weighted != 0);
}

// The most LDS one workgroup of the kernels may take on this device: min(kSiteEndsLdsMost, the device's LDS per
// workgroup); above 64 KiB the weighted kernels' dynamic-LDS limit is raised to it.  Once per context (the caller keeps
// the result).  A run whose two tracks need more is split whatever the threshold says.
hipError_t siteends_lds_most(int device, int* most_out);

// Sites the runs of one call may hold each: site_run_sites_of with the profile's constant, a run being one or two
// workgroups.  Its bound on a 32-bit LDS count holds here as it stands: see ftk_siteends.hip.
long long siteends_run_sites(int n_cu, long long n_sites, long long n_frag, int max_end, const SiteEndsParams& p);

// Runs as for launch_site_profile, with order[si] = the caller's index of sorted site si (read only when site_sum is
// given).  sum[(run_group[r] * 2 + track) * n_bins + k] and cnt[...] (may be NULL) += the run's two tracks; both zeroed
// by the caller.  site_sum (may be NULL) and site_cnt (may be NULL): [n_sites][4] = left_up, left_down, right_up,
// right_down of every site of the runs, at row order[si], written with plain stores - each cell by one workgroup.
// n_runs * (p.split ? 2 : 1) <= kSiteMaxRunsPerLaunch, n_runs >= 1, cv.n >= 1; siteends_lds(p) within siteends_lds_most.
void launch_site_ends(hipStream_t s, const ContigView& cv, const uint32_t* weights, const uint32_t* site, const int32_t* order,
                      const int32_t* run_off, const int32_t* run_group, int n_runs, const SiteEndsParams& p, unsigned long long* sum,
                      unsigned long long* cnt, unsigned long long* site_sum, unsigned long long* site_cnt);

}  // namespace ftk
