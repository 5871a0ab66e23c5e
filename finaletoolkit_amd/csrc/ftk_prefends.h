// Launchers of the preferred-end kernels in ftk_prefends.hip (internal).  The rule: include/ftk.h, "preferred ends".
#pragma once

#include "ftk_tilecall.h"

namespace ftk {

// the two halo instantiations: the literature's 1 kb window and FTK_PREFENDS_MAX_HALF
constexpr int kPrefHaloSmall = 512, kPrefHaloLarge = 2048;
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

struct PrefOut {
    int32_t* run;
    int64_t* pos;
    int32_t* kind;
    int32_t* count;
    int64_t* total;
    int32_t* n_w;
};

// the count pass and the scan of its counts
void launch_prefends_count(hipStream_t s, const ContigView& cv, const PrefParams& p, int n_tiles, const TileCallPlan& pl);
// the write pass: call r of the batch at out.*[r]
void launch_prefends_write(hipStream_t s, const ContigView& cv, const PrefParams& p, int n_tiles, const TileCallPlan& pl,
                           const PrefOut& out);

}  // namespace ftk
