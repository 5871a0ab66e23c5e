// Launchers of the per-base depth kernels in ftk_depth.hip (internal).
#pragma once

#include "ftk_internal.h"

namespace ftk {

// tiles one pass of the single workgroup of depth_scan_kernel takes (its width)
constexpr int kDepthScanWidth = 1024;

struct DepthParams {
    long long start, stop;  // the region; tile k holds the bases [start + k * kWpsTile, ...)
    int min_len, max_len, mapq_min;
    int lmax;          // longest admissible fragment
    int include_zero;  // runs of depth 0 are kept (the runs then tile the region)
};

// What the two run passes hand each other, one entry per tile.
struct DepthRunPlan {
    int32_t* cnt;    // runs the tile opens (pass 1)
    int32_t* first;  // its first base whose depth differs from the base in front, INT32_MAX: none (pass 1)
    int32_t* off;    // exclusive prefix sum of cnt (scan)
    int32_t* next;   // first such base behind the tile, p.stop: none (scan)
    int64_t* total;  // one word: runs in the region (scan)
};

// depth[stop - start]
void launch_depth(hipStream_t s, const ContigView& cv, const DepthParams& p, int64_t n_tiles, int32_t* depth);
// pass 1 and the scan of its counts
void launch_depth_count(hipStream_t s, const ContigView& cv, const DepthParams& p, int64_t n_tiles, const DepthRunPlan& rp);
// pass 2: run r of the region at run_start[r], run_end[r], run_depth[r]
void launch_depth_write(hipStream_t s, const ContigView& cv, const DepthParams& p, int64_t n_tiles, const DepthRunPlan& rp,
                        int32_t* run_start, int32_t* run_end, int32_t* run_depth);

}  // namespace ftk
