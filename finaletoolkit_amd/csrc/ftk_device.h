// Device-only primitives that more than one kernel file uses (included by .hip files only): the wave scan and sums, the
// position-index bound of the per-base tiles, and the reads of a reference image through
// its RefView (the G + C count of a span included).  A new kernel file takes these from here.
#pragma once

#include "ftk_internal.h"

namespace ftk {

// inclusive prefix sum over the 64 lanes of a wave on DPP (row_shr 1/2/4/8 inside rows of 16, then row_bcast:15 /
// row_bcast:31 across rows): no LDS traffic, where six dependent `__shfl_up` are six LDS permutes
__device__ __forceinline__ int wave_incl_scan_dpp(int x) {
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);
    return x;
}

// the sum over the 64 lanes of a wave, in every lane
__device__ __forceinline__ unsigned int wave_sum_u32(unsigned int v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64x(unsigned long long v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// first fragment of the position-index bin of q (which = 0) or of the bin behind it (which = 1): the conservative
// candidate bounds of a tile, "start >= q" below and "start < q" above
__device__ __forceinline__ int index_bound(const ContigView& cv, long long q, int which) {
    if (q <= 0) return 0;
    const long long kb = q >> kBinShift;
    return kb >= cv.n_bins ? cv.n : cv.bin_idx[kb + which];
}

// ---- a reference image through its RefView ----------------------------------------------------------------------
// does [a, b) touch one of the N blocks [lo, hi) of n_nblk?  (sorted, disjoint: the first block that ends behind a)
__device__ __forceinline__ bool n_block_search(const int32_t* nblk_start, const int32_t* nblk_end, int n_nblk, int a, int b,
                                               int lo, int hi) {
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (nblk_end[m] <= a) lo = m + 1; else hi = m;
    }
    return lo < n_nblk && nblk_start[lo] < b;
}
__device__ __forceinline__ bool ref_has_n(const RefView& rv, int a, int b) {
    return n_block_search(rv.nblk_start, rv.nblk_end, rv.n_nblk, a, b, 0, rv.n_nblk);
}

// FASTA text: the byte offset of base p and its column in the line; ref_text_next steps both to base p + 1
__device__ __forceinline__ long long ref_text_offset(const RefView& rv, int p, int& col) {
    const int row = p / rv.line_bases;
    col = p - row * rv.line_bases;
    return (long long)row * rv.line_width + col;
}
__device__ __forceinline__ void ref_text_next(const RefView& rv, long long& off, int& col) {
    ++off;
    if (++col == rv.line_bases) { col = 0; off += rv.line_width - rv.line_bases; }
}

// 2bit: the code of base p (T=0 C=1 A=2 G=3; G and C have the low bit set) out of the byte that holds it, img[p >> 2]
__device__ __forceinline__ uint32_t twobit_code(uint32_t byte, int p) { return (byte >> (6 - 2 * (p & 3))) & 3u; }

// first cell of row L of a packed length x GC table (ftk_gcbias.h), relative to row 0
__device__ __forceinline__ int tri(int L) { return L * (L + 1) / 2; }

// ---- G + C bases of a span [a, b) of the image (frag_gc_kernel, frag_gc_weight_kernel) --------------------------------
// 0 <= a < b <= chrom_len, b - a <= FTK_GC_MAX_LEN.  -1: the span holds an N.
__device__ __forceinline__ int span_gc_2bit(const RefView& im, int a, int b) {
    if (im.n_nblk && ref_has_n(im, a, b)) return -1;
    const uint32_t* w32 = reinterpret_cast<const uint32_t*>(im.img);  // (the block is 256-byte aligned and 32 bytes longer than the image)
    const int w0 = a >> 4, w1 = (b - 1) >> 4;
    int g = 0;
    for (int w = w0; w <= w1; ++w) {
        const uint32_t v = __builtin_bswap32(w32[w]) & 0x55555555u;  // base j of the word: bit 30 - 2 j
        const int j0 = max(a - 16 * w, 0), j1 = min(b - 16 * w, 16);
        uint32_t m = 0xffffffffu >> (2 * j0);
        if (j1 < 16) m &= ~(0xffffffffu >> (2 * j1));
        g += __popc(v & m);
    }
    return g;
}

__device__ __forceinline__ int span_gc_text(const RefView& im, int a, int b) {
    int col;
    long long off = ref_text_offset(im, a, col);
    int g = 0;
    bool bad = false;
    for (int j = a; j < b; ++j) {
        const int ch = im.img[off] & 0xDF;  // fold case
        const bool gc = (ch == 'G') | (ch == 'C');
        g += gc;
        bad |= !(gc | (ch == 'A') | (ch == 'T'));
        ref_text_next(im, off, col);
    }
    return bad ? -1 : g;
}

}  // namespace ftk
