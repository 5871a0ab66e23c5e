// Nucleotide and dinucleotide profiles around fragment ends (ftk_end_context) and their background (ftk_ref_context):
// the rule is in include/ftk.h under "end context".  base(q) = A 0, C 1, G 2, T 3 or N 4 of a reference image resident in
// HBM (ref_base, ftk_device.h); every kept fragment gives two oriented readings r0(o) = base(a0 + o), r1(o) = comp(base(a1 - o)) and adds one to
// out[class][kind][o + W][5 r(o) + r(o + 1)] for every o of [-W, W).
//
// Both kernels keep the classes of one row of the grid in a workgroup's LDS block of 32-bit cells (a workgroup sees fewer
// than 2^31 fragments and a fragment adds at most one to a cell - its (class, kind, offset) row gets exactly one - so no
// cell can wrap) and flush it once, one 64-bit global atomic per non-zero cell.  Counts are integers: the table does not
// depend on the order of arrival.
//
// end_context_frag_kernel   lanes are FRAGMENTS: a thread takes one fragment and walks its 2 x 2W offsets, as
//                           frag_gc_kernel walks a span; the 64 lanes of a step stand at one offset of 64 fragments and
//                           meet in the 25 cells of that row.  The arrangement ftk_end_context launches: measured the
//                           faster of the two (docs/experiments.md, "End context") - its loads do not depend on one
//                           another, so a thread keeps several in flight.
// end_context_kernel        lanes are OFFSETS.  A wave takes 64 fragments at a time: lane i classifies fragment i and, when
//                           it is kept, stages its two ends (anchor, class, kind, is the window clean) in the wave's
//                           LDS list, compacted by the ballot.  Then a wave step takes as many whole ends as 2W lanes fit
//                           into 64 (one at W = 32; an end wider than 64 offsets takes several steps): a lane reads its
//                           end's entry (a broadcast), extracts ITS pair of bases and issues one returnless LDS add at
//                           row * 25 + cell.  The rows of a step are 25 words apart - an odd stride - so they spread over
//                           the banks.  Every step waits for its own list entry and then its own bytes of the image, a
//                           chain the step before cannot hide: the slower one as it stands.  FTK_CONTEXT_ARRANGE=0.
// ref_context_kernel        a thread walks runs of kCtxRefRun positions and counts in 25 cells of its own (LDS,
//                           cell-major: no atomics, no conflicts); the cells are summed per wave and added to the result.
//
// A window is CLEAN when the image is 2bit and its 2W + 1 bases lie inside the contig and outside every N block (one binary
// search per end): both bases of a pair then come out of two adjacent bytes.  Every other window - FASTA text included -
// reads base by base through ref_base.
#include <algorithm>
#include <cstdlib>

#include "ftk_device.h"
#include "ftk_endcontext.h"

namespace ftk {

namespace {

constexpr int kCtxWaves = kCtxThreads / 64;

__device__ __forceinline__ int ctx_comp(int x) { return x < 4 ? 3 - x : 4; }

// is [a - half, a + half + 1), what both kinds read around an anchor, a clean window?
__device__ __forceinline__ bool ctx_clean(const RefView& im, int a, int half) {
    if (im.kind != FTK_REF_2BIT || a - half < 0 || a + half + 1 > im.chrom_len) return false;
    return !(im.n_nblk && ref_has_n(im, a - half, a + half + 1));
}

// 5 r(o) + r(o + 1) of the reading of `kind` whose offset o stands at position q (kind 0: a0 + o, kind 1: a1 - o)
__device__ __forceinline__ int ctx_cell(const RefView& im, int q, int kind, bool clean) {
    if (clean) {
        const int lo = q - kind;  // bases lo and lo + 1 (the block is 32 bytes longer than the image)
        const uint32_t v = ((uint32_t)im.img[lo >> 2] << 8) | im.img[(lo >> 2) + 1];
        const uint32_t pr = (v >> (12 - 2 * (lo & 3))) & 15u;
        const int x = acgt_of_2bit(pr >> 2), y = acgt_of_2bit(pr & 3u);
        return kind ? 5 * (3 - y) + (3 - x) : 5 * x + y;
    }
    if (!kind) return 5 * ref_base(im, q) + ref_base(im, q + 1);
    return 5 * ctx_comp(ref_base(im, q)) + ctx_comp(ref_base(im, q - 1));
}

// the class of fragment i among the row's classes [c0, c0 + nc), or -1; its anchors
__device__ __forceinline__ int ctx_classify(const ContigView& cv, const EndContextParams& p, long long i, int c0, int nc, int& a0,
                                            int& a1) {
    const int s = cv.start[i], e = cv.end[i], L = e - s;
    if ((int)cv.mapq[i] < p.mapq_min || L < p.edges[0] || L >= p.edges[p.n_classes]) return -1;
    int c = 0;
#pragma unroll
    for (int k = 1; k < FTK_CONTEXT_MAX_CLASSES; ++k) c += (k < p.n_classes && L >= p.edges[k]) ? 1 : 0;
    const int half_len = p.anchor == FTK_CONTEXT_CENTRE ? (L >> 1) : 0;
    a0 = s + half_len;
    a1 = e - 1 - half_len;
    c -= c0;
    return c >= 0 && c < nc ? c : -1;
}

// the LDS block to the result; kept_s likewise
__device__ __forceinline__ void ctx_flush(const uint32_t* cells, const unsigned int* kept_s, int n_cells, int c0, int nc, int class_cells,
                                          unsigned long long* __restrict__ out, unsigned long long* __restrict__ n_kept) {
    const int tid = threadIdx.x;
    for (int i = tid; i < n_cells; i += kCtxThreads) {
        const uint32_t v = cells[i];
        if (v) atomicAdd(&out[(long long)c0 * class_cells + i], (unsigned long long)v);
    }
    if (tid < nc && kept_s[tid]) atomicAdd(&n_kept[c0 + tid], (unsigned long long)kept_s[tid]);
}

__global__ __launch_bounds__(kCtxThreads) void end_context_kernel(ContigView cv, RefView im, EndContextParams p,
                                                                  unsigned long long* __restrict__ out,
                                                                  unsigned long long* __restrict__ n_kept) {
    extern __shared__ uint32_t ctx_cells[];        // the row's classes: [class][kind][offset][25]
    __shared__ int2 ends_s[kCtxWaves][128];        // per wave: the kept ends of its 64 fragments, (anchor, (class * 2 + kind) * 2 + clean)
    __shared__ unsigned int kept_s[FTK_CONTEXT_MAX_CLASSES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c0 = blockIdx.y * p.lds_classes, nc = min(p.lds_classes, p.n_classes - c0);
    const int rows = 2 * p.half, class_cells = 2 * rows * kCtxCellsPerRow, n_cells = nc * class_cells;
    for (int i = tid; i < n_cells; i += kCtxThreads) ctx_cells[i] = 0;
    if (tid < FTK_CONTEXT_MAX_CLASSES) kept_s[tid] = 0;
    __syncthreads();
    // a lane's place in a step: `per_step` whole ends side by side, or one end over `sub_steps` steps
    const int width = min(rows, 64), per_step = 64 / width, sub_steps = (rows + 63) >> 6;
    const int slot = lane / width, lrow = lane - slot * width;
    int2* ends = ends_s[wv];
    const long long n_batches = ((long long)cv.n + 63) >> 6;
    for (long long b = (long long)blockIdx.x * kCtxWaves + wv; b < n_batches; b += (long long)gridDim.x * kCtxWaves) {
        const long long i = b * 64 + lane;
        int a0 = 0, a1 = 0;
        const int cls = i < cv.n ? ctx_classify(cv, p, i, c0, nc, a0, a1) : -1;
        const unsigned long long mask = __ballot(cls >= 0);
        if (!mask) continue;  // (the same in every lane)
        if (cls >= 0) {
            const int r = __popcll(mask & ((1ull << lane) - 1ull));
            atomicAdd(&kept_s[cls], 1u);
            ends[2 * r] = make_int2(a0, (cls * 2 + 0) * 2 + (ctx_clean(im, a0, p.half) ? 1 : 0));
            ends[2 * r + 1] = make_int2(a1, (cls * 2 + 1) * 2 + (ctx_clean(im, a1, p.half) ? 1 : 0));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int n_ends = 2 * __popcll(mask);
        for (int first = 0; first < n_ends; first += per_step) {
            const int u = first + slot;
            if (slot < per_step && u < n_ends) {
                const int2 d = ends[u];
                const int kind = (d.y >> 1) & 1, ck = d.y >> 1;
                for (int sub = 0; sub < sub_steps; ++sub) {
                    const int row = sub * 64 + lrow;
                    if (row < rows) {
                        const int o = row - p.half;
                        const int cell = ctx_cell(im, kind ? d.x - o : d.x + o, kind, d.y & 1);
                        atomicAdd(&ctx_cells[(ck * rows + row) * kCtxCellsPerRow + cell], 1u);
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the list is read before the next batch overwrites it
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    ctx_flush(ctx_cells, kept_s, n_cells, c0, nc, class_cells, out, n_kept);
}

__global__ __launch_bounds__(kCtxThreads) void end_context_frag_kernel(ContigView cv, RefView im, EndContextParams p,
                                                                       unsigned long long* __restrict__ out,
                                                                       unsigned long long* __restrict__ n_kept) {
    extern __shared__ uint32_t ctx_cells[];
    __shared__ unsigned int kept_s[FTK_CONTEXT_MAX_CLASSES];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.y * p.lds_classes, nc = min(p.lds_classes, p.n_classes - c0);
    const int rows = 2 * p.half, class_cells = 2 * rows * kCtxCellsPerRow, n_cells = nc * class_cells;
    for (int i = tid; i < n_cells; i += kCtxThreads) ctx_cells[i] = 0;
    if (tid < FTK_CONTEXT_MAX_CLASSES) kept_s[tid] = 0;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * kCtxThreads + tid; i < cv.n; i += (long long)gridDim.x * kCtxThreads) {
        int a[2] = {0, 0};
        const int cls = ctx_classify(cv, p, i, c0, nc, a[0], a[1]);
        if (cls < 0) continue;
        atomicAdd(&kept_s[cls], 1u);
#pragma unroll
        for (int kind = 0; kind < 2; ++kind) {
            const bool clean = ctx_clean(im, a[kind], p.half);
            uint32_t* row_cells = ctx_cells + (cls * 2 + kind) * rows * kCtxCellsPerRow;
            for (int row = 0; row < rows; ++row) {
                const int o = row - p.half;
                atomicAdd(&row_cells[row * kCtxCellsPerRow + ctx_cell(im, kind ? a[kind] - o : a[kind] + o, kind, clean)], 1u);
            }
        }
    }
    __syncthreads();
    ctx_flush(ctx_cells, kept_s, n_cells, c0, nc, class_cells, out, n_kept);
}

__global__ __launch_bounds__(kCtxRefThreads) void ref_context_kernel(RefView im, int pos_lo, int pos_hi, long long n_runs,
                                                                     unsigned long long* __restrict__ out25) {
    __shared__ uint32_t cnt[kCtxCellsPerRow * kCtxRefThreads];  // cell-major; a thread sees fewer than 2^30 positions
    const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll
    for (int c = 0; c < kCtxCellsPerRow; ++c) cnt[c * kCtxRefThreads + tid] = 0;
    for (long long r = (long long)blockIdx.x * kCtxRefThreads + tid; r < n_runs; r += (long long)gridDim.x * kCtxRefThreads) {
        const int lo = (int)(pos_lo + r * kCtxRefRun), hi = min(lo + kCtxRefRun, pos_hi);
        // bases lo .. hi are read (hi <= chrom_len: base(chrom_len) is N)
        const bool clean = im.kind == FTK_REF_2BIT && hi + 1 <= im.chrom_len && !(im.n_nblk && ref_has_n(im, lo, hi + 1));
        int cur = clean ? acgt_of_2bit(twobit_code(im.img[lo >> 2], lo)) : ref_base(im, lo);
        for (int q = lo; q < hi; ++q) {
            const int nxt = clean ? acgt_of_2bit(twobit_code(im.img[(q + 1) >> 2], q + 1)) : ref_base(im, q + 1);
            ++cnt[(5 * cur + nxt) * kCtxRefThreads + tid];
            cur = nxt;
        }
    }
#pragma unroll
    for (int c = 0; c < kCtxCellsPerRow; ++c) {
        const unsigned int v = wave_sum_u32(cnt[c * kCtxRefThreads + tid]);  // (a wave's share of fewer than 2^30 positions)
        if (lane == 0 && v) atomicAdd(&out25[c], (unsigned long long)v);
    }
}

}  // namespace

void launch_end_context(hipStream_t s, int n_cu, const ContigView& cv, const RefView& im, EndContextParams p, int arrangement,
                        unsigned long long* out, unsigned long long* n_kept) {
    if (cv.n <= 0) return;
    p.lds_classes = ctx_lds_classes(p.half);
    const int n_rows = (p.n_classes + p.lds_classes - 1) / p.lds_classes;
    const size_t lds = (size_t)std::min(p.lds_classes, p.n_classes) * ctx_class_cells(p.half) * 4;
    const long long blocks = ((long long)cv.n + kCtxThreads - 1) / kCtxThreads;  // either arrangement: kCtxThreads fragments a pass
    // workgroups a CU's 160 KiB of LDS hold (beside the 8 KiB of the waves' lists), at most 4: 32 wave slots
    const long long per_cu = std::max<long long>(1, std::min<long long>(4, (160 << 10) / (lds + (9 << 10))));
    const long long resident = std::max<long long>(1, (long long)n_cu * per_cu / n_rows);
    const dim3 grid((unsigned)std::min(blocks, resident), (unsigned)n_rows);
    if (arrangement == kCtxLanesAreFragments)
        hipLaunchKernelGGL(end_context_frag_kernel, grid, dim3(kCtxThreads), lds, s, cv, im, p, out, n_kept);
    else
        hipLaunchKernelGGL(end_context_kernel, grid, dim3(kCtxThreads), lds, s, cv, im, p, out, n_kept);
}

void launch_ref_context(hipStream_t s, int n_cu, const RefView& im, int pos_lo, int pos_hi, unsigned long long* out25) {
    if (pos_hi <= pos_lo) return;
    const long long n_runs = ((long long)pos_hi - pos_lo + kCtxRefRun - 1) / kCtxRefRun;
    const long long blocks = (n_runs + kCtxRefThreads - 1) / kCtxRefThreads;
    hipLaunchKernelGGL(ref_context_kernel, dim3((unsigned)std::min<long long>(blocks, (long long)n_cu * 4)), dim3(kCtxRefThreads), 0, s,
                       im, pos_lo, pos_hi, n_runs, out25);
}

}  // namespace ftk
