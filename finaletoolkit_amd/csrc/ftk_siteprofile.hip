// Site-aggregated midpoint profiles (ftk_site_profile): for every site (centre c, flip flag, group) the fragments that
// pass the MAPQ / length rule and whose midpoint m = (start + end) >> 1 lies in [c - H, c + H) are counted, and their
// weights summed, in bin (m - c + H) / b of the site's group - bin n_bins - 1 - k for a flipped site.  Sums and counts
// are integers, so no result depends on the order of arrival.
//
// site_profile_kernel  one workgroup per RUN of sites; the host sorted the sites by (group, centre) and cut the list
//                      into runs that stay inside one group (site_run_sites).  The run's profile lives in LDS: n_bins
//                      64-bit sums and n_bins 32-bit counts (12 bytes per bin, 48 KiB at most).  The scan is the shared
//                      one of ftk_sitescan.h: a wave takes one site at a time and its lanes stride over the site's
//                      candidates.  The predicate is branch-free and the bin is the integer quotient (quot).  A passing
//                      candidate adds to its bin with LDS atomics; at the end of the run the non-zero bins go to the
//                      zeroed outputs of the run's group.
#include <algorithm>

#include "ftk_sitescan.h"

namespace ftk {

namespace {

template <bool WEIGHTED>
__global__ __launch_bounds__(kSiteThreads) void site_profile_kernel(ContigView cv, const uint32_t* __restrict__ weights,
                                                                    const uint32_t* __restrict__ site,
                                                                    const int32_t* __restrict__ run_off,
                                                                    const int32_t* __restrict__ run_group, SiteProfileParams p,
                                                                    unsigned long long* __restrict__ sum_out,
                                                                    unsigned long long* __restrict__ cnt_out) {
    extern __shared__ unsigned long long sum_s[];  // n_bins sums (WEIGHTED only), then n_bins counts
    unsigned int* cnt_s = reinterpret_cast<unsigned int*>(sum_s + p.n_bins);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    site_cells_clear<WEIGHTED>(sum_s, cnt_s, p.n_bins);
    const int s0 = run_off[blockIdx.x], s1 = run_off[blockIdx.x + 1];
    const int H = p.half_width, b = p.bin_size;
    const float rinv = 1.0f / (float)b;
    for (int si = s0 + wv; si < s1; si += kSiteThreads / 64) {
        const uint32_t word = site[si];
        const int c = (int)(word & ~kSiteFlipBit);
        const bool flip = (word & kSiteFlipBit) != 0;
        site_scan<WEIGHTED>(cv, weights, c, H, p.lmax, lane, [&](bool valid, int fs, int fe, int q, uint32_t wt) {
            const int len = fe - fs;
            const int mid = (int)(((unsigned)fs + (unsigned)fe) >> 1);  // coordinates < 2^30
            const int d = mid - c;
            const bool ok = valid & (q >= p.mapq_min) & (len >= p.min_len) & (len <= p.max_len) & (d >= -H) & (d < H);
            int k = quot(ok ? d + H : 0, b, rinv);  // 0 <= x < 2 H <= 2^21
            if (flip) k = p.n_bins - 1 - k;
            if (ok) {  // 0 <= k < n_bins
                atomicAdd(&cnt_s[k], 1u);
                if (WEIGHTED) atomicAdd(&sum_s[k], (unsigned long long)wt);
            }
        });
    }
    site_cells_flush<WEIGHTED>(sum_s, cnt_s, p.n_bins, (size_t)run_group[blockIdx.x] * (size_t)p.n_bins, sum_out, cnt_out);
}

}  // namespace

hipError_t site_lds_limit(int device, int cap, std::initializer_list<const void*> kernels, int* limit_out) {
    int limit = 0;
    hipError_t e = hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device);
    if (e != hipSuccess) return e;
    if (limit < 12 * kSiteMaxBins) return hipErrorInvalidValue;  // (no gfx9 device: 64 KiB is the least any has)
    limit = std::min(cap, limit);
    if (limit > (64 << 10))
        for (const void* k : kernels)
            if ((e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, limit)) != hipSuccess) return e;
    *limit_out = limit;
    return hipSuccess;
}

long long site_run_sites_of(int n_cu, long long n_sites, long long n_frag, int max_end, int half_width, int lmax,
                            long long run_candidates, long long groups_per_run) {
    const double reach = 2.0 * half_width + lmax + 2.0 * (1 << kBinShift);  // what the index hands one site
    const double est = std::max(1.0, std::min((double)n_frag, (double)n_frag / std::max(max_end, 1) * reach));
    long long per_run = (long long)((double)run_candidates / est) + 1;
    const long long runs = std::max((kSiteRunsPerCu * n_cu + groups_per_run - 1) / groups_per_run, 1LL);
    per_run = std::min(per_run, (n_sites + runs - 1) / runs);
    per_run = std::min(per_run, (long long)(0xffffffffLL / std::max(n_frag, 1LL)));
    return std::max(per_run, 1LL);
}

long long site_run_sites(int n_cu, long long n_sites, long long n_frag, int max_end, const SiteProfileParams& p) {
    return site_run_sites_of(n_cu, n_sites, n_frag, max_end, p.half_width, p.lmax, kSiteRunCandidates, 1);
}

void launch_site_profile(hipStream_t s, const ContigView& cv, const uint32_t* weights, const uint32_t* site, const int32_t* run_off,
                         const int32_t* run_group, int n_runs, const SiteProfileParams& p, unsigned long long* sum,
                         unsigned long long* cnt) {
    if (n_runs <= 0 || cv.n <= 0) return;
    const size_t lds = (size_t)p.n_bins * 12;
    if (p.weighted)
        hipLaunchKernelGGL(site_profile_kernel<true>, dim3((unsigned)n_runs), dim3(kSiteThreads), lds, s, cv, weights, site, run_off,
                           run_group, p, sum, cnt);
    else
        hipLaunchKernelGGL(site_profile_kernel<false>, dim3((unsigned)n_runs), dim3(kSiteThreads), lds, s, cv, weights, site, run_off,
                           run_group, p, sum, cnt);
}

}  // namespace ftk
