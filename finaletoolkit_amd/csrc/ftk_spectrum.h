// Launchers of the periodogram kernels in ftk_spectrum.hip (internal).  The rule: include/ftk.h, "spectrum".
#pragma once

#include "ftk_internal.h"

namespace ftk {

constexpr int kSpectrumMaxPeriods = 1024;
constexpr int kSpectrumMinPeriod = 2, kSpectrumMaxPeriod = 4096;
constexpr long long kSpectrumMaxRun = 1LL << 22;  // sum |v| < 2^53: exact in the float64 the mean is divided in
// Runs (workgroups of the first pass) and (run, four periods) workgroups of the second per launch.
constexpr long long kSpectrumMaxBlocks = 1LL << 30;
constexpr int kSpectrumWaves = 4;  // periods per workgroup of the second pass on a run read from memory, one wave each
// Runs of at most this many samples (128 KiB of float64; the device's LDS per workgroup where that is less) are folded out
// of LDS: workgroups of kSpectrumStagedThreads threads, each taking kSpectrumStagedPeriods periods of its run.
#ifndef FTK_SPECTRUM_LDS_SAMPLES
#define FTK_SPECTRUM_LDS_SAMPLES (16 << 10)
#endif
constexpr int kSpectrumLdsSamples = FTK_SPECTRUM_LDS_SAMPLES;
constexpr int kSpectrumStagedThreads = 512, kSpectrumStagedPeriods = 32;
inline int spectrum_chunks(int n_per, int per_block) { return (n_per + per_block - 1) / per_block; }

// One (cos, sin) pair per residue of a period.
struct Twiddle { double c, s; };

// table[tab_off[k] + j] = (cos, sin)(2 pi j / periods[k]) for j < periods[k]; all device arrays.
void launch_spectrum_twiddles(hipStream_t s, const int32_t* periods, const int32_t* tab_off, int n_per, Twiddle* table);

// Run r is v[beg[r], end[r]) (0 <= end - beg <= kSpectrumMaxRun; device arrays of n_runs entries each, 1 <= n_runs <=
// kSpectrumMaxBlocks).  x[beg[r] + n] = (v - mean) * taper, ssw[r] = sum of the squared taper (ssw may be NULL), *bad |= 1
// when some |v| >= 2^31.
void launch_spectrum_prep(hipStream_t s, const int64_t* v, const int64_t* beg, const int64_t* end, long long n_runs, double taper,
                          int detrend, double* x, double* ssw, int* bad);

// The samples a staged run may hold on this device: min(kSpectrumLdsSamples, LDS per workgroup / 8); above 64 KiB the
// kernel's dynamic-LDS limit is raised to it.  Once per context (the caller keeps the result).
hipError_t spectrum_lds_samples(int device, int* samples_out);

// out[(r * n_per + k) * 2 + {0, 1}] = (re, im) of run r of x at periods[k]; n_runs * ceil(n_per / kSpectrumWaves) <=
// kSpectrumMaxBlocks, n_per >= 1.  limit: runs of at most that many samples are staged in LDS (-1: none);
// longest_staged: the longest of them among these runs (-1: there is none); any_longer: some run is longer than limit.
void launch_spectrum_fold(hipStream_t s, const double* x, const int64_t* beg, const int64_t* end, long long n_runs,
                          const int32_t* periods, const int32_t* tab_off, const Twiddle* table, int n_per, int limit, int longest_staged,
                          bool any_longer, double* out);

}  // namespace ftk
