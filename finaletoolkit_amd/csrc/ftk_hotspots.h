// Launchers of the IFS hotspot kernels in ftk_hotspots.hip (internal).  The rule: include/ftk.h, "IFS hotspots".
#pragma once

#include "ftk_tilecall.h"

namespace ftk {

// the two halo instantiations, in bins: the 5 kb / 10 kb backgrounds at a 20-base step (h2 + m = 260) and
// FTK_IFS_MAX_REACH
constexpr int kIfsHaloSmall = 512, kIfsHaloLarge = 1024;
// per-tile counters of the count pass: tested windows, called windows
constexpr int kIfsStats = 2;
// workgroups of the totals kernel, one (count, length sum) pair each
constexpr int kIfsTotalsBlocks = 1024;

enum IfsPass { kIfsCount = 0, kIfsWrite = 1, kIfsTrack = 2 };

struct IfsParams {
    int chrom;    // chrom_size
    int step;     // s
    int m;        // bins per window
    int n_bins;   // ceil(chrom / s)
    unsigned L;   // mean_len
    int h1, h2;   // half-widths in bins (h2 == 0: off)
    int reach;    // max(h1, h2); 0 for the track pass, which reads no background
    unsigned min_count;
    int n_thr;
    const unsigned* thr;  // device copy of the caller's table (every entry < 2^32)
    unsigned long long global_mean;
    int min_len, max_len, mapq_min;
    int lmax;    // longest admissible fragment
    int packed;  // read lq instead of end and mapq (packed_call_ok said so)
};

struct IfsOut {
    // called windows (write pass)
    int32_t* run;
    int64_t* pos;
    int32_t* count;
    int64_t* ifs;
    int64_t* bg1;
    int32_t* nb1;
    int64_t* bg2;
    int32_t* nb2;
    // every window (track pass)
    int32_t* n_out;
    int64_t* ifs_out;
};

// the count pass and the scan of its counts
void launch_ifs_count(hipStream_t s, const ContigView& cv, const IfsParams& p, int n_tiles, const TileCallPlan& pl);
// the write pass: called window r of the batch at out.*[r]
void launch_ifs_write(hipStream_t s, const ContigView& cv, const IfsParams& p, int n_tiles, const TileCallPlan& pl, const IfsOut& out);
// the track pass: n and I of every window of every tile
void launch_ifs_track(hipStream_t s, const ContigView& cv, const IfsParams& p, long long n_tiles, const TileCallPlan& pl, const IfsOut& out);
// passing fragments with a midpoint on the contig: kIfsTotalsBlocks pairs (count, length sum) at partial[2 b], [2 b + 1]
void launch_ifs_totals(hipStream_t s, const ContigView& cv, const IfsParams& p, unsigned long long* partial);

}  // namespace ftk
