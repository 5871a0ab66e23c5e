// End-motif x fragment-length tables (ftk_motif_length_table): the rule is in include/ftk.h under "motif x length".  Every
// kept fragment [s, e) of length L adds one to out[kind][r][code] for its two readings of k bases - kind 0: base(s + shift
// + i), kind 1: comp(base(e - 1 - shift - i)), i = 0 .. k-1, first base most significant, column 4^k when a base is N -
// in its length row r = (L - len_lo) / len_bin.
//
// The table of k = 4 over 1000 lengths is 2 x 1000 x 257 cells, far more than a workgroup's LDS, and the fragments come
// sorted by start, not by length.  Two passes:
//
// motiflen_rows_kernel    pass A: one stream over the (start, end, mapq) columns counts the kept fragments per row in a
//                         workgroup's LDS and adds the non-zero rows to n_kept.  Part of the result - and what tells pass B,
//                         on the device, which rows hold anything.
// motiflen_table_kernel   pass B, the arrangement of end_context_frag_kernel: lanes are fragments, grid.y walks BANDS of
//                         p.band rows.  A workgroup first sums n_kept over its band and returns when that is 0, before it
//                         touches a column (on plasma data most bands are empty).  Otherwise it keeps the band as 32-bit cells
//                         in LDS, [row][kind][4^k + 1] - it sees fewer than 2^31 fragments and a fragment adds one per kind, so
//                         no cell can wrap - reads start and end of every fragment, mapq and the image only for the fragments
//                         of its own band, and flushes once, one 64-bit global atomic per non-zero cell.
//
// A reading is CLEAN when the image is 2bit and its k bases lie inside the contig and outside every N block: they then come
// out of two adjacent bytes at once (k <= 4 bases from any alignment span at most 7 digits of the 8).  Every other reading -
// FASTA text, the contig's edges, N blocks - goes base by base through ref_base.  Counts are integers: the table does not
// depend on the order of arrival.
#include <algorithm>

#include "ftk_device.h"
#include "ftk_motiflen.h"

namespace ftk {

namespace {

// the code of the k bases [lo, lo + k) of a clean window, read as kind 0 (ascending) or kind 1 (descending, complemented)
__device__ __forceinline__ int motiflen_clean_code(const RefView& im, int lo, int k, int kind) {
    const uint32_t v = ((uint32_t)im.img[lo >> 2] << 8) | im.img[(lo >> 2) + 1];  // (the block is 32 bytes longer than the image)
    const uint32_t mask = (1u << (2 * k)) - 1u;
    uint32_t a = acgt_of_2bit_word(v >> (16 - 2 * ((lo & 3) + k))) & mask;  // base lo is the top digit
    if (!kind) return (int)a;
    a = ((a & 0x33u) << 2) | ((a >> 2) & 0x33u);  // the four digits of a byte in reverse order ...
    a = ((a & 0x0fu) << 4) | (a >> 4);
    return (int)(~(a >> (2 * (4 - k))) & mask);   // ... the k of them at the bottom, complemented (3 - x)
}

// the column of the reading of `kind` whose first base stands at position q (kind 0 walks up from q, kind 1 down)
__device__ __forceinline__ int motiflen_code(const RefView& im, int q, int k, int kind) {
    const int lo = kind ? q - k + 1 : q;
    if (im.kind == FTK_REF_2BIT && lo >= 0 && lo + k <= im.chrom_len && !(im.n_nblk && ref_has_n(im, lo, lo + k)))
        return motiflen_clean_code(im, lo, k, kind);
    int code = 0;
    bool undefined = false;
    for (int i = 0; i < k; ++i) {
        const int x = ref_base(im, kind ? q - i : q + i);
        undefined |= x == 4;
        code = 4 * code + (kind ? 3 - x : x);
    }
    return undefined ? 1 << (2 * k) : code;
}

__global__ __launch_bounds__(kMotifLenThreads) void motiflen_rows_kernel(ContigView cv, MotifLenParams p,
                                                                         unsigned long long* __restrict__ n_kept) {
    __shared__ unsigned int rows_s[FTK_MOTIFLEN_MAX_ROWS];  // a workgroup sees fewer than 2^31 fragments
    const int tid = threadIdx.x;
    for (int i = tid; i < p.n_rows; i += kMotifLenThreads) rows_s[i] = 0;
    __syncthreads();
    // kMotifLenUnroll fragments a step, their loads issued together (a fragment behind the last one: L = 0, never kept)
    const long long stride = (long long)gridDim.x * kMotifLenThreads;
    for (long long i0 = (long long)blockIdx.x * kMotifLenThreads + tid; i0 < cv.n; i0 += kMotifLenUnroll * stride) {
        int L[kMotifLenUnroll], mq[kMotifLenUnroll];
#pragma unroll
        for (int j = 0; j < kMotifLenUnroll; ++j) {
            const long long i = i0 + j * stride;
            L[j] = i < cv.n ? cv.end[i] - cv.start[i] : 0;
            mq[j] = i < cv.n ? (int)cv.mapq[i] : 0;
        }
#pragma unroll
        for (int j = 0; j < kMotifLenUnroll; ++j) {
            if (mq[j] < p.mapq_min || L[j] < p.len_lo || L[j] > p.len_hi) continue;
            atomicAdd(&rows_s[(unsigned)(L[j] - p.len_lo) / (unsigned)p.len_bin], 1u);  // < n_rows: L <= len_hi
        }
    }
    __syncthreads();
    for (int i = tid; i < p.n_rows; i += kMotifLenThreads) {
        const unsigned int v = rows_s[i];
        if (v) atomicAdd(&n_kept[i], (unsigned long long)v);
    }
}

__global__ __launch_bounds__(kMotifLenThreads) void motiflen_table_kernel(ContigView cv, RefView im, MotifLenParams p,
                                                                          const unsigned long long* __restrict__ n_kept,
                                                                          unsigned long long* __restrict__ out) {
    extern __shared__ uint32_t band_cells[];  // [row][kind][4^k + 1]
    const int tid = threadIdx.x;
    const int r0 = blockIdx.y * p.band, nr = min(p.band, p.n_rows - r0);
    // pass A's counts of the band (complete: the launch before this one on the stream); the same answer in every thread
    bool any = false;
    for (int i = tid; i < nr; i += kMotifLenThreads) any |= n_kept[r0 + i] != 0;
    if (!__syncthreads_or(any)) return;
    const int cols = (1 << (2 * p.k)) + 1, n_cells = nr * 2 * cols;
    for (int i = tid; i < n_cells; i += kMotifLenThreads) band_cells[i] = 0;
    __syncthreads();
    // the lengths of the band: [band_lo, band_hi], inside [len_lo, len_hi] (r0 * len_bin <= len_hi - len_lo)
    const int band_lo = p.len_lo + r0 * p.len_bin;
    const int band_hi = (int)min((long long)band_lo + (long long)nr * p.len_bin - 1, (long long)p.len_hi);
    // kMotifLenUnroll fragments a step, their loads issued together (a fragment behind the last one: L = 0, in no band)
    const long long stride = (long long)gridDim.x * kMotifLenThreads;
    for (long long i0 = (long long)blockIdx.x * kMotifLenThreads + tid; i0 < cv.n; i0 += kMotifLenUnroll * stride) {
        int fs[kMotifLenUnroll], fe[kMotifLenUnroll];
#pragma unroll
        for (int j = 0; j < kMotifLenUnroll; ++j) {
            const long long i = i0 + j * stride;
            fs[j] = i < cv.n ? cv.start[i] : 0;
            fe[j] = i < cv.n ? cv.end[i] : 0;
        }
#pragma unroll
        for (int j = 0; j < kMotifLenUnroll; ++j) {
            const int s = fs[j], e = fe[j], L = e - s;
            if (L < band_lo || L > band_hi || (int)cv.mapq[i0 + j * stride] < p.mapq_min) continue;
            const int r = p.len_bin == 1 ? L - band_lo : (int)((unsigned)(L - band_lo) / (unsigned)p.len_bin);  // < nr
            uint32_t* row_cells = band_cells + r * 2 * cols;
            atomicAdd(&row_cells[motiflen_code(im, s + p.shift, p.k, 0)], 1u);
            atomicAdd(&row_cells[cols + motiflen_code(im, e - 1 - p.shift, p.k, 1)], 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i < n_cells; i += kMotifLenThreads) {
        const uint32_t v = band_cells[i];
        if (!v) continue;
        const int rk = i / cols, c = i - rk * cols;  // rk = row * 2 + kind
        atomicAdd(&out[((long long)(rk & 1) * p.n_rows + r0 + (rk >> 1)) * cols + c], (unsigned long long)v);
    }
}

}  // namespace

void launch_motif_length(hipStream_t s, int n_cu, const ContigView& cv, const RefView& im, MotifLenParams p, unsigned long long* out,
                         unsigned long long* n_kept) {
    if (cv.n <= 0) return;
    p.band = motiflen_lds_rows(p.k);
    const int n_bands = (p.n_rows + p.band - 1) / p.band;
    const size_t lds = (size_t)std::min(p.band, p.n_rows) * 2 * motiflen_cols(p.k) * 4;  // <= 63 KiB: two workgroups a CU
    const long long blocks = ((long long)cv.n + kMotifLenThreads - 1) / kMotifLenThreads;
    const long long resident = (long long)n_cu * 2;
    hipLaunchKernelGGL(motiflen_rows_kernel, dim3((unsigned)std::min(blocks, resident)), dim3(kMotifLenThreads), 0, s, cv, p, n_kept);
    // Workgroups per band.  The workgroups of an empty band return at once, so the grid may hold more than the CUs do: up to
    // four times, shared among the bands; never more per band than are resident at once (each flushes up to a whole band).
    const long long per_band = std::max<long long>(1, std::min(resident, 4 * resident / n_bands));
    hipLaunchKernelGGL(motiflen_table_kernel, dim3((unsigned)std::min(blocks, per_band), (unsigned)n_bands), dim3(kMotifLenThreads), lds,
                       s, cv, im, p, n_kept, out);
}

}  // namespace ftk
