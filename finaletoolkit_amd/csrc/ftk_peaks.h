// Launchers of the nucleosome-call kernels in ftk_peaks.hip (internal).  The rule: include/ftk.h, "peaks".
#pragma once

#include "ftk_internal.h"

namespace ftk {

constexpr int kPeaksMaxRegion = 1024;  // FTK_PEAKS_MAX_REGION: the values of one region, held in LDS by one wave
constexpr int kPeaksMaxGap = 63;       // FTK_PEAKS_MAX_GAP: a position sees max_gap + 1 <= 64 neighbours, one mask word
constexpr int kPeaksTile = 1024;       // positions per workgroup of the mark pass
constexpr int kPeaksHalo = 64;         // positions a tile reads on either side of its own (>= kPeaksMaxGap + 1)

struct PeaksParams {
    int32_t skip, max_gap, min_region, short_max, max_region;
};

// The device arrays of one call.  Regions and calls are counted in 32 bits: reg_cap and out_cap are at most INT32_MAX.
struct PeaksBufs {
    const int32_t *tile_run, *tile_k;  // per tile of the mark pass: its run and its number within that
    uint64_t* tile_cnt;                // n_tiles + 1: region starts (low half) and ends (high half) per tile, then scanned
    int64_t *reg_start, *reg_end;      // reg_cap: [start, end) of every region as indices into the track, in position order
    int32_t* reg_run;                  // reg_cap: the run every region lies in
    double* reg_med;                   // reg_cap: the median of every region that is called
    uint64_t* reg_cnt;                 // reg_cap + 1: calls per region, then scanned (behind *n_calls)
    int64_t reg_cap;
    int64_t* stats;                    // six counters per run (FTK_PEAKS_*), zeroed by the caller
    uint64_t* n_calls;                 // calls written so far, zeroed by the caller: launch_peaks appends
    int* bad;                          // set when a score is not finite, zeroed by the caller
    int32_t* o_run;                    // out_cap each: the calls
    int64_t *o_start, *o_stop, *o_summit;
    double *o_height, *o_area;
    int64_t out_cap;
};

// Calls of the runs a[off[r], off[r + 1]) (r < n_runs; device arrays), tiled by tile_run / tile_k (n_tiles >= 1 tiles of
// kPeaksTile positions, every run's own, in run order), appended behind *n_calls in (run, start) order.  A call's run is
// run_base + r, its positions count from the run's start; stats rows are indexed by run_base + r too.
void launch_peaks(hipStream_t s, const double* a, const int64_t* off, int n_runs, int64_t n_tiles, const PeaksParams& p,
                  int run_base, const PeaksBufs& b);

// v[i] = (double)v[i] in place (the WPS is scored as int64, the adjust chain reads float64).
void launch_i64_to_f64(hipStream_t s, void* v, int64_t n);

}  // namespace ftk
