// Launchers of the fragment length x GC kernels in ftk_gcbias.hip (internal).
#pragma once

#include "ftk_internal.h"

namespace ftk {

// Both tables are kept in LDS "packed": row L holds only its L + 1 possible counts g = 0 .. L, so the row of length L
// starts tri(L) - tri(first row) cells into the block, tri(L) = L (L + 1) / 2.
constexpr int kGcFragThreads = 1024;
constexpr int kGcFragLdsCells = 32768;  // observed table: 128 KiB of u32 per workgroup
constexpr int kGcRefThreads = 1024;
constexpr int kGcRefTile = 4096;        // positions per tile of the expected table
constexpr int kGcRefLdsCells = 28672;   // expected table: 112 KiB of u32 beside the tile's 20 KiB of prefix sums
constexpr int kGcRefMaxChunks = 64;

inline long long gc_tri(long long L) { return L * (L + 1) / 2; }

struct FragGcParams {
    int min_len, max_len, mapq_min;  // the kept fragments (closed bounds, 1 <= min_len, max_len <= FTK_GC_MAX_LEN)
    int len_lo, len_hi;              // table rows (table != nullptr: equal to min_len, max_len)
    int lds_hi;                      // rows len_lo .. lds_hi are counted in LDS, the rows above with global atomics
};

// gc_out (may be NULL): gc per fragment or -1.  table (may be NULL): (len_hi - len_lo + 1) x (len_hi + 1) int64 cells
// the launch ADDS to, *n_skipped likewise (both zeroed by the caller).
void launch_frag_gc(hipStream_t s, int n_cu, const ContigView& cv, const RefView& im, FragGcParams p, int16_t* gc_out,
                    unsigned long long* table, unsigned long long* n_skipped);
// table: as above, zeroed by the caller; positions p of [pos_lo, pos_hi) with p % stride == 0.
// 0 <= pos_lo < pos_hi <= im.chrom_len.
void launch_ref_gc_table(hipStream_t s, int n_cu, const RefView& im, int pos_lo, int pos_hi, int len_lo, int len_hi,
                         long long stride, unsigned long long* table);

}  // namespace ftk
