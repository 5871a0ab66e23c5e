// Fragment length x GC tables (ftk_frag_gc, ftk_frag_gc_table, ftk_ref_gc_table): what deepTools computeGCBias, Griffin
// and GCparagon measure.  gc(a, b) = G + C bases of seq[a:b] of a reference image resident in HBM, undefined when the
// span leaves the contig, is longer than FTK_GC_MAX_LEN or holds an N base (2bit: a base of an N block; FASTA text: any
// byte but ACGTacgt).
//
// frag_gc_kernel       one thread per fragment, grid-stride over the contig's start-sorted columns.  2bit: the span's
//                      32-bit words (first base in the high bits once byte-swapped; G and C are the codes with the low
//                      bit set, twobit_code), the first and the last one masked, __popc of the rest - 11-12 words
//                      for 167 bases, which neighbouring fragments share through the caches - and a binary search of
//                      the N blocks; FASTA text: the bytes through the line geometry, case folded.  The same body
//                      writes the int16 per fragment and / or counts the table: rows len_lo .. lds_hi in a workgroup's
//                      own LDS block of 32-bit cells (a workgroup sees fewer than 2^31 fragments: no cell can wrap),
//                      the rows above with 64-bit global atomics, the LDS block flushed with one global atomic per
//                      non-zero cell.
// ref_gc_table_kernel  one workgroup per (tiles, chunk of rows).  Per tile of kGcRefTile positions it builds, in LDS, the
//                      prefix sums x[i] over the tile and a halo of the chunk's longest length of one packed word per
//                      base: is-GC in the low half, is-N (or behind the contig's end) in the high half.  A window
//                      [p, p + L) is then ONE subtraction, x[p + L] - x[p]: high half 0 = defined, low half = g.  A
//                      thread owns one length and walks the sampled positions of its group (threads of a wave: adjacent
//                      lengths, so x[p] is a broadcast, x[p + L] consecutive words and the LDS atomics go to different
//                      rows).  The chunk's rows stay in LDS over all tiles of the workgroup and are flushed once.
//
// Both tables are packed in LDS: the row of length L holds g = 0 .. L only (ftk_gcbias.h).  Counts are integers, so
// neither table depends on the order of arrival.
#include <algorithm>

#include "ftk_device.h"
#include "ftk_gcbias.h"

namespace ftk {

namespace {

// rows [lo[c], lo[c + 1]) of the expected table belong to chunk c
struct GcRefChunks {
    int n;
    short lo[kGcRefMaxChunks + 1];
};

constexpr int kGcRefPer = (kGcRefTile + FTK_GC_MAX_LEN + kGcRefThreads) / kGcRefThreads;  // bases per thread and tile
constexpr int kGcRefXLen = kGcRefPer * kGcRefThreads + 8;                                 // words of x[] (>= tile + halo + 1)
static_assert(kGcRefPer * kGcRefThreads >= kGcRefTile + FTK_GC_MAX_LEN, "a tile and its halo fit the threads' shares");

__global__ __launch_bounds__(kGcFragThreads) void frag_gc_kernel(ContigView cv, RefView im, FragGcParams p, int n_lds_cells,
                                                                 int16_t* __restrict__ gc_out,
                                                                 unsigned long long* __restrict__ table,
                                                                 unsigned long long* __restrict__ n_skipped) {
    extern __shared__ uint32_t gc_cells[];  // table != nullptr: rows len_lo .. lds_hi, packed
    __shared__ unsigned int skipped_s;
    const int tid = threadIdx.x;
    const int tri0 = tri(p.len_lo), pitch = p.len_hi + 1;
    if (table) {
        for (int i = tid; i < n_lds_cells; i += kGcFragThreads) gc_cells[i] = 0;
        if (tid == 0) skipped_s = 0;
        __syncthreads();
    }
    for (long long i = (long long)blockIdx.x * kGcFragThreads + tid; i < cv.n; i += (long long)gridDim.x * kGcFragThreads) {
        const int a = cv.start[i], b = cv.end[i], L = b - a;
        int g = -1;
        if ((int)cv.mapq[i] >= p.mapq_min && L >= p.min_len && L <= p.max_len) {
            g = span_gc(im, a, b);
            if (table) {
                if (g < 0) atomicAdd(&skipped_s, 1u);
                else if (L <= p.lds_hi) atomicAdd(&gc_cells[tri(L) - tri0 + g], 1u);
                else atomicAdd(&table[(long long)(L - p.len_lo) * pitch + g], 1ull);
            }
        }
        if (gc_out) gc_out[i] = (int16_t)g;
    }
    if (!table) return;
    __syncthreads();
    flush_packed_rows<kGcFragThreads>(gc_cells, p.len_lo, p.lds_hi, p.len_lo, pitch, table);
    if (tid == 0 && skipped_s) atomicAdd(n_skipped, (unsigned long long)skipped_s);
}

// is-GC (bit 0) / is-N or outside the contig (bit 16) of position q >= 0
// (not stated over ref_base: once per base and tile, that made ref_gc_table_kernel 1103 -> 1364 instructions long)
__device__ __forceinline__ uint32_t base_flags(const RefView& im, int q) {
    if (q >= im.chrom_len) return 0x10000u;
    if (im.kind == FTK_REF_2BIT) {
        if (im.n_nblk && ref_has_n(im, q, q + 1)) return 0x10000u;
        return twobit_code(im.img[q >> 2], q) & 1u;
    }
    int col;
    const int ch = im.img[ref_text_offset(im, q, col)] & 0xDF;
    if ((ch == 'G') | (ch == 'C')) return 1u;
    return ((ch == 'A') | (ch == 'T')) ? 0u : 0x10000u;
}

__global__ __launch_bounds__(kGcRefThreads) void ref_gc_table_kernel(RefView im, int pos_lo, int pos_hi, int len_lo, int len_hi,
                                                                     long long stride, GcRefChunks ch, int n_tiles,
                                                                     unsigned long long* __restrict__ table) {
    extern __shared__ uint32_t gc_lds[];
    __shared__ uint32_t wsum[kGcRefThreads / 64];
    uint32_t* x = gc_lds;                  // x[i] = flags of the tile's first i bases, summed
    uint32_t* cells = gc_lds + kGcRefXLen;  // the chunk's rows, packed
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int L0 = ch.lo[blockIdx.y], L1 = ch.lo[blockIdx.y + 1] - 1, R = L1 - L0 + 1;
    const int tri0 = tri(L0), n_cells = tri(L1 + 1) - tri0;
    for (int i = tid; i < n_cells; i += kGcRefThreads) cells[i] = 0;
    const int groups = kGcRefThreads / R, pg = tid / R;  // thread = (group of positions, length)
    const int L = L0 + (tid - pg * R), row = tri(L) - tri0;
    const int nx = kGcRefTile + L1;  // bases a window of the tile can reach
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int tile_lo = pos_lo + tile * kGcRefTile, tile_hi = min(tile_lo + kGcRefTile, pos_hi);
        __syncthreads();  // the tile before: every reader of x[] and wsum[] has finished (first tile: cells[] is zero)
        uint32_t f[kGcRefPer], sum = 0;
#pragma unroll
        for (int k = 0; k < kGcRefPer; ++k) {
            const int i = tid * kGcRefPer + k;
            if (i < nx) sum += base_flags(im, tile_lo + i);
            f[k] = sum;
        }
        const uint32_t incl = (uint32_t)wave_incl_scan_dpp((int)sum);  // (the packed sums stay far below 2^31)
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        uint32_t excl = incl - sum;
        for (int w = 0; w < wv; ++w) excl += wsum[w];
        if (tid == 0) x[0] = 0;
#pragma unroll
        for (int k = 0; k < kGcRefPer; ++k) {
            const int i = tid * kGcRefPer + k;
            if (i < nx) x[i + 1] = excl + f[k];
        }
        __syncthreads();
        if (pg < groups) {
            const long long first = ((long long)tile_lo + stride - 1) / stride * stride;  // the tile's first sampled position
            for (long long q = first + pg * stride; q < tile_hi; q += groups * stride) {
                const int i = (int)(q - tile_lo);
                const uint32_t d = x[i + L] - x[i];  // (the low half never borrows: both halves only grow)
                if (!(d >> 16)) atomicAdd(&cells[row + d], 1u);
            }
        }
    }
    __syncthreads();
    flush_packed_rows<kGcRefThreads>(cells, L0, L1, len_lo, len_hi + 1, table);
}

}  // namespace

void launch_frag_gc(hipStream_t s, int n_cu, const ContigView& cv, const RefView& im, FragGcParams p, int16_t* gc_out,
                    unsigned long long* table, unsigned long long* n_skipped) {
    if (cv.n <= 0) return;
    int n_cells = 0;
    if (table) {
        p.lds_hi = p.len_lo;
        while (p.lds_hi < p.len_hi && gc_tri(p.lds_hi + 2) - gc_tri(p.len_lo) <= kGcFragLdsCells) ++p.lds_hi;
        n_cells = (int)(gc_tri(p.lds_hi + 1) - gc_tri(p.len_lo));
    }
    const size_t lds = (size_t)n_cells * 4;
    hipLaunchKernelGGL(frag_gc_kernel, dim3(frag_pass_grid(n_cu, cv.n, kGcFragThreads, lds)), dim3(kGcFragThreads), lds, s, cv, im, p,
                       n_cells, gc_out, table, n_skipped);
}

void launch_ref_gc_table(hipStream_t s, int n_cu, const RefView& im, int pos_lo, int pos_hi, int len_lo, int len_hi,
                         long long stride, unsigned long long* table) {
    if (pos_hi <= pos_lo) return;
    GcRefChunks ch{};
    long long most = 0;
    for (int lo = len_lo; lo <= len_hi;) {  // rows are taken while the chunk fits its LDS block
        int hi = lo;
        while (hi < len_hi && gc_tri(hi + 2) - gc_tri(lo) <= kGcRefLdsCells) ++hi;
        most = std::max(most, gc_tri(hi + 1) - gc_tri(lo));
        ch.lo[ch.n++] = (short)lo;
        lo = hi + 1;
    }
    ch.lo[ch.n] = (short)(len_hi + 1);
    const int n_tiles = (int)(((long long)pos_hi - pos_lo + kGcRefTile - 1) / kGcRefTile);
    const int gx = std::max(1, std::min(n_tiles, n_cu / ch.n));
    const size_t lds = ((size_t)kGcRefXLen + (size_t)most) * 4;
    hipLaunchKernelGGL(ref_gc_table_kernel, dim3((unsigned)gx, (unsigned)ch.n), dim3(kGcRefThreads), lds, s, im, pos_lo, pos_hi,
                       len_lo, len_hi, stride, ch, n_tiles, table);
}

}  // namespace ftk
