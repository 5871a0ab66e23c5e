// Launchers of the fragment-weight kernels in ftk_weights.hip (internal).
#pragma once

#include "ftk_gcbias.h"
#include "ftk_internal.h"

namespace ftk {

constexpr int kGcWeightThreads = 1024;
// The weight table is packed like the observed table (ftk_gcbias.h: row L holds g = 0 .. L) and is staged in LDS whole
// while it has at most this many cells - lengths (1, 254) fit, (1, 255) do not - else it is read from global memory.
constexpr int kGcWeightLdsCells = kGcFragLdsCells;
constexpr int kWwThreads = 256;  // weighted_window_kernel: a chunk of kChunk candidates is 16 per thread

inline long long gc_weight_cells(int len_lo, int len_hi) { return gc_tri((long long)len_hi + 1) - gc_tri(len_lo); }

struct GcWeightParams {
    int len_lo, len_hi, mapq_min;  // 1 <= len_lo <= len_hi <= FTK_GC_MAX_LEN
    int n_cells;                   // gc_weight_cells(len_lo, len_hi)
    int in_lds;                    // the table is staged in LDS (n_cells <= kGcWeightLdsCells)
};

// The window predicate of ftk_window_counts (WinPred, ftk_kernels.hip) and the reach of its candidate range.
struct WeightedWinParams {
    int mapq_min, min_len, max_len;  // closed bounds (open ones: INT32_MIN / INT32_MAX)
    int policy, bam;                 // FTK_POLICY_*; 1: the read1 fetch rule (the contig has read1 columns)
    int lmax;                        // longest fragment that can pass
};

// w_out[i] = packed[tri(L) - tri(len_lo) + gc] for every fragment that passes the MAPQ / length rule and has a gc, else
// 0; *n_zero += the fragments that pass the rule and got 0 (zeroed by the caller).  `packed`: n_cells device words.
void launch_frag_gc_weights(hipStream_t s, int n_cu, const ContigView& cv, const RefView& im, GcWeightParams p,
                            const uint32_t* packed, uint32_t* w_out, unsigned long long* n_zero);

// Blocks per window (gridDim.y) for n_win windows of a contig of n_frag fragments on n_cu compute units.
int weighted_window_slices(int n_cu, long long n_win, long long n_frag);
// sum[w] += the weights of the fragments window w counts, cnt[w] (may be NULL) += those with a weight above 0; both
// zeroed by the caller.  ws / we: device arrays of n_win >= 1 entries.
void launch_weighted_windows(hipStream_t s, const ContigView& cv, const uint32_t* weights, const int32_t* ws, const int32_t* we,
                             int n_win, int slices, const WeightedWinParams& p, unsigned long long* sum, unsigned long long* cnt);

}  // namespace ftk
