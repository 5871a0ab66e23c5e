// Launchers of the preferred-end kernels in ftk_prefends.hip (internal).  The rule: include/ftk.h, "preferred ends".
#pragma once

#include "ftk_internal.h"

namespace ftk {

// positions per workgroup (PREFENDS_TILE of _lib.py)
constexpr int kPrefTile = 4096;
// the two halo instantiations: the literature's 1 kb window and FTK_PREFENDS_MAX_HALF
constexpr int kPrefHaloSmall = 512, kPrefHaloLarge = 2048;
// tiles of one batch: what the single workgroup of the scan walks, and the bound of a batch's plan in the scratch
constexpr int kPrefBatchTiles = 4096;
constexpr int kPrefScanWidth = 1024;
// per-tile counters of the count pass, in the order of the call's per-interval counters
constexpr int kPrefStats = 6;

struct PrefParams {
    int chrom;      // chrom_size
    int half;       // h
    int split;      // mode
    unsigned min_count;
    int n_thr;
    const unsigned long long* thr;  // device copy of the caller's table
    int min_len, max_len, mapq_min;
    int lmax;    // longest admissible fragment
    int packed;  // read lq instead of end and mapq (packed_call_ok said so)
};

// One batch of tiles: what the passes hand each other, one entry per tile.
struct PrefPlan {
    const int32_t* tile_t0;   // first position
    const int32_t* tile_len;  // positions (1 .. kPrefTile)
    const int32_t* tile_run;  // its interval's number
    uint32_t* stats;          // [n_tiles][kPrefStats] (count pass)
    int32_t* off;             // exclusive prefix sum of the tiles' calls (scan)
    int64_t* total;           // one word: calls of the batch (scan)
};

struct PrefOut {
    int32_t* run;
    int64_t* pos;
    int32_t* kind;
    int32_t* count;
    int64_t* total;
    int32_t* n_w;
};

// the count pass and the scan of its counts
void launch_prefends_count(hipStream_t s, const ContigView& cv, const PrefParams& p, int n_tiles, const PrefPlan& pl);
// the write pass: call r of the batch at out.*[r]
void launch_prefends_write(hipStream_t s, const ContigView& cv, const PrefParams& p, int n_tiles, const PrefPlan& pl,
                           const PrefOut& out);

}  // namespace ftk
