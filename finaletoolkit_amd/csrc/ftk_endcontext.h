// Launchers of the end-context kernels in ftk_endcontext.hip (internal).
#pragma once

#include "ftk_internal.h"

namespace ftk {

constexpr int kCtxThreads = 512;
constexpr int kCtxCellsPerRow = 25;     // 5 x 5 (first base, second base), N = 4
constexpr int kCtxLdsCells = 32768;     // a workgroup's block of classes: 128 KiB of u32
constexpr int kCtxRefThreads = 256;
constexpr int kCtxRefRun = 64;          // reference positions a thread of the background kernel walks at a time

// the two LDS arrangements of end_context (docs/experiments.md has both times)
constexpr int kCtxLanesAreOffsets = 0;    // a wave takes one fragment end per 2W lanes, a lane one offset
constexpr int kCtxLanesAreFragments = 1;  // a thread takes one fragment and walks its offsets

// cells of one class: [2 kinds][2W offsets][25]
inline int ctx_class_cells(int half) { return 2 * 2 * half * kCtxCellsPerRow; }
// classes one workgroup keeps in LDS at that width; the rest go to further rows of the grid
inline int ctx_lds_classes(int half) {
    const int fit = kCtxLdsCells / ctx_class_cells(half);
    return fit < FTK_CONTEXT_MAX_CLASSES ? fit : FTK_CONTEXT_MAX_CLASSES;
}

struct EndContextParams {
    int edges[FTK_CONTEXT_MAX_CLASSES + 1];  // strictly ascending, 1 <= edges[0], edges[n_classes] <= 2^30
    int n_classes, half, mapq_min, anchor;
    int lds_classes;                         // classes per row of the grid
};

// out: [n_classes][2][2 half][25] int64 cells the launch ADDS to, n_kept[n_classes] likewise (both zeroed by the caller).
void launch_end_context(hipStream_t s, int n_cu, const ContigView& cv, const RefView& im, EndContextParams p, int arrangement,
                        unsigned long long* out, unsigned long long* n_kept);
// out25: zeroed by the caller; 0 <= pos_lo < pos_hi <= im.chrom_len.
void launch_ref_context(hipStream_t s, int n_cu, const RefView& im, int pos_lo, int pos_hi, unsigned long long* out25);

}  // namespace ftk
