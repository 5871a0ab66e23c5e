// Launcher of the motif x length kernels in ftk_motiflen.hip (internal).
#pragma once

#include "ftk_internal.h"

namespace ftk {

constexpr int kMotifLenThreads = 512;
// a workgroup's band of rows: 63 KiB of u32 - with the kernel's few static words still within the 64 KiB a launch gets
// without raising the dynamic-LDS limit, and two workgroups to a CU's 160 KiB
constexpr int kMotifLenLdsCells = 16128;
constexpr int kMotifLenUnroll = 4;       // fragments a thread takes per step of either pass: their column loads are independent
constexpr int kMotifLenBandMax = 512;     // rows a band holds at most (k = 1, 2 would fit more: the flush stays short)

// columns of one (kind, row): the 4^k motifs and "undefined"
inline int motiflen_cols(int k) { return (1 << (2 * k)) + 1; }
// rows one workgroup keeps in LDS, [row][kind][4^k + 1]; the further rows of a call go to further rows of the grid
inline int motiflen_lds_rows(int k) {
    const int fit = kMotifLenLdsCells / (2 * motiflen_cols(k));
    return fit < kMotifLenBandMax ? fit : kMotifLenBandMax;
}

struct MotifLenParams {
    int k, shift;                  // 1 <= k <= FTK_MOTIFLEN_MAX_K, |shift| <= 4
    int len_lo, len_hi, len_bin;   // 1 <= len_lo <= len_hi <= 2^30, len_bin >= 1
    int n_rows;                    // (len_hi - len_lo) / len_bin + 1 <= FTK_MOTIFLEN_MAX_ROWS
    int mapq_min;
    int band;                      // rows per row of the grid (motiflen_lds_rows(k))
};

// out: [2][n_rows][4^k + 1] int64 cells the launch ADDS to, n_kept[n_rows] likewise (both zeroed by the caller, on `s`).
void launch_motif_length(hipStream_t s, int n_cu, const ContigView& cv, const RefView& im, MotifLenParams p, unsigned long long* out,
                         unsigned long long* n_kept);

}  // namespace ftk
