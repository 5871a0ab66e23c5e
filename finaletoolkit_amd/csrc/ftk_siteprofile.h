// Launcher of the site-profile kernel in ftk_siteprofile.hip (internal).
#pragma once

#include <initializer_list>

#include "ftk_internal.h"

namespace ftk {

// Threads of a workgroup (a multiple of 64: one wave takes one site at a time), the candidates a run of sites should
// hold before its LDS profile is flushed, and the runs per compute unit a call keeps when it has the sites for them.
// Chosen on the MI355X: docs/experiments.md, "site profile".
#ifndef FTK_SITE_THREADS
#define FTK_SITE_THREADS 256
#endif
#ifndef FTK_SITE_RUN_CANDIDATES
#define FTK_SITE_RUN_CANDIDATES (4 * 4096)
#endif
#ifndef FTK_SITE_RUNS_PER_CU
#define FTK_SITE_RUNS_PER_CU 4
#endif
constexpr int kSiteThreads = FTK_SITE_THREADS;
constexpr long long kSiteRunsPerCu = FTK_SITE_RUNS_PER_CU;
constexpr long long kSiteRunCandidates = FTK_SITE_RUN_CANDIDATES;
constexpr int kSiteMaxRunsPerLaunch = 1 << 20;  // workgroups of one launch (1 024 threads at most each: < 2^32 threads)
constexpr int kSiteMaxBins = 4096;          // 48 KiB of LDS: 8 bytes of sum and 4 of count per bin
constexpr int kSiteMaxHalfWidth = 1 << 20;  // d + H < 2^21: exact in the float the bin's quotient is estimated in
constexpr uint32_t kSiteFlipBit = 1u << 31; // a site word: the centre (< 2^30) with the flip flag on top

struct SiteProfileParams {
    int half_width, bin_size, n_bins;  // n_bins = 2 * half_width / bin_size <= kSiteMaxBins
    int mapq_min, min_len, max_len;    // closed bounds (open ones: INT32_MIN / INT32_MAX)
    int lmax;                          // longest fragment that can pass
    int weighted;                      // 1: sum the weight column; 0: every fragment weighs FTK_WEIGHT_ONE
};

// Sites the runs of one call may hold each, for n_sites sites of a contig of n_frag fragments that ends at max_end:
// about kSiteRunCandidates candidates at the contig's mean density, no more than leaves kSiteRunsPerCu runs per compute unit, and
// few enough that a bin's 32-bit LDS count cannot wrap (a site adds at most n_frag to a bin).
long long site_run_sites(int n_cu, long long n_sites, long long n_frag, int max_end, const SiteProfileParams& p);
// The same rule with the caller's own numbers: `run_candidates` candidates per run, and runs of `groups_per_run`
// workgroups each (kSiteRunsPerCu workgroups per compute unit are kept, not runs).
long long site_run_sites_of(int n_cu, long long n_sites, long long n_frag, int max_end, int half_width, int lmax,
                            long long run_candidates, long long groups_per_run);

// The most dynamic LDS a workgroup of `kernels` may take on this device: min(cap, the device's LDS per workgroup); above
// the 64 KiB a kernel gets without asking, the kernels' limit is raised to it.  hipErrorInvalidValue: the device cannot
// hold the 12 * kSiteMaxBins bytes of the widest weighted row or track.  Once per context (the caller keeps the result).
hipError_t site_lds_limit(int device, int cap, std::initializer_list<const void*> kernels, int* limit_out);

// Run r = sites [run_off[r], run_off[r + 1]) of `site` (sorted by group, then centre), all of group run_group[r]:
// sum[run_group[r] * n_bins + k] and cnt[...] (may be NULL) += the run's profile; both zeroed by the caller.  `weights`
// is read only when p.weighted.  Device arrays; n_runs >= 1, cv.n >= 1.
void launch_site_profile(hipStream_t s, const ContigView& cv, const uint32_t* weights, const uint32_t* site, const int32_t* run_off,
                         const int32_t* run_group, int n_runs, const SiteProfileParams& p, unsigned long long* sum,
                         unsigned long long* cnt);

}  // namespace ftk
