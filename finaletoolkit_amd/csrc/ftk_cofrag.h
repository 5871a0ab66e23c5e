// Launchers of the co-fragmentation kernels in ftk_cofrag.hip (internal).
#pragma once

#include "ftk_internal.h"

namespace ftk {

constexpr int kKsTile = 64;      // T: edge of the pair tile one workgroup computes (ftk_hist_ks_shape)
constexpr int kKsChunk = 32;     // lengths one LDS chunk holds (ftk_hist_ks_shape)
constexpr int kKsThreads = 256;  // of a tile workgroup: 16 x 16 threads, each with a 4 x 4 block of pairs
constexpr int kKsBlock = 4;      // edge of a thread's register block
constexpr int kKsRowThreads = 256;
constexpr int kKsNoRow = 0x7f7f7f7f;  // the flag's rest value (what a byte fill of 0x7f leaves)

// the two arrangements of the pair kernel (docs/experiments.md has both times)
constexpr int kKsPairThreads = 0;  // one thread per pair i <= j, both prefix columns straight from memory
constexpr int kKsTiles = 1;        // one workgroup per T x T tile of the upper triangle, prefixes staged in LDS

// row pitch of the prefix image: rows rounded up to whole tiles, so a tile's staging needs no bound on the row
inline int ks_pitch(int n_rows) { return (n_rows + kKsTile - 1) / kKsTile * kKsTile; }

// hist: [n_rows][n_bins] cells.  prefix: [n_bins][pitch] - C(i, l) at prefix[l * pitch + i], LENGTH-major, so that the
// rows of a tile lie side by side at every length; the columns i >= n_rows are not written (and what a tile reads there
// never reaches an output).  n32[i] = n(i) mod 2^32.  *bad_row = min(*bad_row, i) for every row with n(i) >= 2^31
// (the caller sets it to kKsNoRow); the prefixes of such a row are meaningless.
void launch_ks_rows(hipStream_t s, const uint32_t* hist, int n_rows, int n_bins, uint32_t* prefix, uint32_t* n32, int32_t* bad_row);
// every cell of k_out [n_rows][n_rows], at_out (or nullptr) and n_out [n_rows]; every n(i) < 2^31.
void launch_ks_pairs(hipStream_t s, int arrangement, const uint32_t* prefix, const uint32_t* n32, int n_rows, int n_bins,
                     long long* k_out, int32_t* at_out, long long* n_out);

}  // namespace ftk
