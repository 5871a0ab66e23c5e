// Primitives that more than one kernel file uses (included by .hip files only).  A new kernel file takes from here: the
// wave scan and sums (wave_incl_scan_dpp, wave_sum_u32 / _u64); index_bound of the per-base tiles; the reads of a reference
// image through its RefView - one base (ref_base; its pieces text_base, acgt_of_2bit[_word], twobit_code, ref_has_n,
// ref_text_offset / _next) and the G + C of a span (span_gc); a packed length x GC block in LDS and its way to the 64-bit
// table (tri, flush_packed_rows); and, on the host, the grid of a grid-stride pass over a contig's fragments (frag_pass_grid).
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

// inclusive prefix sum inside each row of 16 lanes (the first four steps above).  A lane only takes from lower lanes of
// its row, so a row whose upper lanes are switched off still gives the lower ones their sums.
__device__ __forceinline__ int row_incl_scan_dpp(int x) {
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);
    return x;
}

// Four consecutive starts from the delta columns (ContigView::ds / gbase, ftk_packed.h): the lane holds the deltas of
// fragments i .. i + 3 in one dword (i a multiple of 4), the 16 lanes of its row hold one group of 64 in order, gb is the
// group's base.  An in-lane prefix, a scan over the row, the base.  Not for a group whose base carries kGbaseWide.
__device__ __forceinline__ int4 starts_from_deltas(unsigned dsw, int gb) {
    const int p0 = (int)(dsw & 255u), p1 = p0 + (int)((dsw >> 8) & 255u), p2 = p1 + (int)((dsw >> 16) & 255u),
              p3 = p2 + (int)(dsw >> 24);
    const int before = gb + row_incl_scan_dpp(p3) - p3;  // the start of the fragment in front of the lane's four
    return make_int4(before + p0, before + p1, before + p2, before + p3);
}

// the sum over the 64 lanes of a wave, in every lane
__device__ __forceinline__ unsigned int wave_sum_u32(unsigned int v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
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

// A 0, C 1, G 2, T 3 of a 2bit code (T 0, C 1, A 2, G 3); of every 2-bit digit of a word at once
__device__ __forceinline__ int acgt_of_2bit(uint32_t c) { return (int)((0x87u >> (2 * c)) & 3u); }
__device__ __forceinline__ uint32_t acgt_of_2bit_word(uint32_t w) {
    const uint32_t v1 = (w >> 1) & 0x55555555u, v0 = w & 0x55555555u;  // T=00 C=01 A=10 G=11
    return ((~(v1 ^ v0) & 0x55555555u) << 1) | (~v1 & 0x55555555u);    // -> A=00 C=01 G=10 T=11
}

// A 0, C 1, G 2, T 3 of a byte of FASTA text in either case; 4 for every other byte
__device__ __forceinline__ int text_base(uint32_t byte) {
    const uint32_t ch = byte & 0xDFu;  // fold case
    return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4;
}

// base q of the image, any q: A 0, C 1, G 2, T 3; 4 for an N (2bit: in an N block; text: not ACGTacgt) or outside the contig
__device__ __forceinline__ int ref_base(const RefView& im, int q) {
    if (q < 0 || q >= im.chrom_len) return 4;
    if (im.kind == FTK_REF_2BIT) {
        if (im.n_nblk && ref_has_n(im, q, q + 1)) return 4;
        return acgt_of_2bit(twobit_code(im.img[q >> 2], q));
    }
    int col;
    return text_base(im.img[ref_text_offset(im, q, col)]);
}

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
        const int ch = im.img[off] & 0xDF;  // (not text_base: its ladder made both fragment kernels ~50 instructions longer)
        const bool gc = (ch == 'G') | (ch == 'C');
        g += gc;
        bad |= !(gc | (ch == 'A') | (ch == 'T'));
        ref_text_next(im, off, col);
    }
    return bad ? -1 : g;
}
// either kind, any a < b with b - a <= FTK_GC_MAX_LEN; -1 also when the span leaves the contig
__device__ __forceinline__ int span_gc(const RefView& im, int a, int b) {
    if (a < 0 || b > im.chrom_len) return -1;
    return im.kind == FTK_REF_2BIT ? span_gc_2bit(im, a, b) : span_gc_text(im, a, b);
}

// ---- a packed length x GC table in LDS (ftk_gcbias.h): the row of length L holds g = 0 .. L only -----------------------
// first cell of row L, relative to row 0
__device__ __forceinline__ int tri(int L) { return L * (L + 1) / 2; }

// rows L0 .. L1 of `cells` (row L0 first) added to the table (row len_lo first, `pitch` cells a row) by a workgroup of THREADS:
// wave = row, lane = g, one global atomic per non-zero cell
template <int THREADS>
__device__ __forceinline__ void flush_packed_rows(const uint32_t* cells, int L0, int L1, int len_lo, int pitch,
                                                  unsigned long long* __restrict__ table) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int L = L0 + wv; L <= L1; L += THREADS / 64) {
        const int base = tri(L) - tri(L0);
        for (int g = lane; g <= L; g += 64) {
            const uint32_t v = cells[base + g];
            if (v) atomicAdd(&table[(long long)(L - len_lo) * pitch + g], (unsigned long long)v);
        }
    }
}

// host: the grid of a grid-stride pass, one thread per fragment, `lds` bytes of LDS per workgroup
inline unsigned frag_pass_grid(int n_cu, long long n_frag, int threads, size_t lds) {
    const long long blocks = (n_frag + threads - 1) / threads;
    const long long resident = (long long)n_cu * (2 * lds <= (size_t)(152 << 10) ? 2 : 1);  // workgroups a CU's LDS and 32 wave slots hold
    return (unsigned)(blocks < resident ? blocks : resident);
}

}  // namespace ftk
