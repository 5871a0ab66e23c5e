// Per-fragment weights (ftk_frags_set_gc_weights, ftk_weighted_window_sums): a uint32 column beside a resident contig's
// columns, in units of 2^-16 (FTK_WEIGHT_ONE), and its sums per window.  Sums are integers, so no result depends on the
// order of arrival.
//
// frag_gc_weight_kernel   one thread per fragment, grid-stride: gc(start, end) through the span-GC code frag_gc_kernel
//                         uses (ftk_device.h), the weight looked up in the length x GC table, one coalesced 4-byte
//                         store per fragment.  The table is packed (row L holds g = 0 .. L, ftk_gcbias.h) and staged
//                         in the workgroup's LDS while it has at most kGcWeightLdsCells cells; a larger one is read
//                         from global memory, where its 2 MB at most stay in the caches.  Fragments that pass the rule
//                         and get weight 0 are counted per thread, then in one LDS counter per workgroup, then with one
//                         global atomic.
// weighted_window_kernel  grid (n_win, S): block (w, y) takes chunks y, y + S, ... of kChunk candidates of window w.
//                         The candidate range comes from the 512-bp index exactly as the window-feature kernels take
//                         it (window_candidates, ftk_kernels.hip): [index_bound(ws - lmax) & ~3, index_bound(we, 1)).
//                         The predicate is WinPred's, branch-free.  Sum and count are kept per lane in 64 bits,
//                         reduced across the wave by shuffles and across the block through LDS, and added to the
//                         zeroed outputs with one 64-bit atomic per block and non-zero result.  It reads the wide
//                         columns (start, end, mapq, weight: 13 bytes per candidate; the read1 columns on top for a
//                         BAM contig).
#include <algorithm>

#include "ftk_device.h"
#include "ftk_weights.h"

namespace ftk {

namespace {

__global__ __launch_bounds__(kGcWeightThreads) void frag_gc_weight_kernel(ContigView cv, RefView im, GcWeightParams p,
                                                                          const uint32_t* __restrict__ packed,
                                                                          uint32_t* __restrict__ w_out,
                                                                          unsigned long long* __restrict__ n_zero) {
    extern __shared__ uint32_t w_cells[];  // p.in_lds: the packed table
    __shared__ unsigned int zero_s;
    const int tid = threadIdx.x;
    if (tid == 0) zero_s = 0;
    if (p.in_lds)
        for (int i = tid; i < p.n_cells; i += kGcWeightThreads) w_cells[i] = packed[i];
    __syncthreads();
    const int tri0 = tri(p.len_lo);
    unsigned int zeros = 0;
    for (long long i = (long long)blockIdx.x * kGcWeightThreads + tid; i < cv.n; i += (long long)gridDim.x * kGcWeightThreads) {
        const int a = cv.start[i], b = cv.end[i], L = b - a;
        uint32_t w = 0;
        if ((int)cv.mapq[i] >= p.mapq_min && L >= p.len_lo && L <= p.len_hi) {
            const int g = span_gc(im, a, b);
            if (g >= 0) {  // (g <= L: the cell lies inside row L)
                const int cell = tri(L) - tri0 + g;
                w = p.in_lds ? w_cells[cell] : packed[cell];
            }
            zeros += w == 0;
        }
        w_out[i] = w;
    }
    if (zeros) atomicAdd(&zero_s, zeros);  // (a workgroup sees fewer than 2^31 fragments)
    __syncthreads();
    if (tid == 0 && zero_s) atomicAdd(n_zero, (unsigned long long)zero_s);
}

// (not ftk_device.h's wave_sum_u64: on __shfl_xor the kernel below came out 12 instructions longer and slower at times)
__device__ __forceinline__ unsigned long long wave_sum_down_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
    return v;  // lane 0 holds the sum
}

template <bool BAM>
__global__ __launch_bounds__(kWwThreads) void weighted_window_kernel(ContigView cv, const uint32_t* __restrict__ weights,
                                                                     const int32_t* __restrict__ ws_, const int32_t* __restrict__ we_,
                                                                     WeightedWinParams p, unsigned long long* __restrict__ sum_out,
                                                                     unsigned long long* __restrict__ cnt_out) {
    __shared__ unsigned long long red[2][kWwThreads / 64];
    const int w = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ws = ws_[w], we = we_[w];  // FTK_OPEN_LO / FTK_OPEN_HI compare like any other bound
    int lo = index_bound(cv, (long long)ws - p.lmax, 0) & ~3;
    int hi = index_bound(cv, we, 1);
    if (hi < lo || we < ws) hi = lo;
    const bool want_mid = p.policy == FTK_POLICY_MIDPOINT, want_any = p.policy == FTK_POLICY_ANY;
    unsigned long long sum = 0, cnt = 0;
    for (long long base = (long long)lo + (long long)blockIdx.y * kChunk; base < hi; base += (long long)gridDim.y * kChunk) {
#pragma unroll
        for (int k = 0; k < kChunk / kWwThreads; ++k) {
            const long long j = base + k * kWwThreads + tid;
            const bool valid = j < hi;
            const int i = (int)(valid ? j : base);  // (base < hi <= n: a fragment of the contig)
            const int fs = cv.start[i], fe = cv.end[i], q = cv.mapq[i];
            const uint32_t wt = weights[i];
            const int len = fe - fs;
            bool ok = valid & (q >= p.mapq_min) & (len >= p.min_len) & (len <= p.max_len);
            const bool overlap = (fs < we) & (fe > ws);
            if (BAM) {
                const int rs = cv.r1_start[i], re = cv.r1_end[i];
                ok &= (rs < we) & (re > ws);
            } else {
                ok &= overlap;
            }
            const int mid = (int)(((unsigned)fs + (unsigned)fe) >> 1);  // coordinates < 2^30
            const bool mid_in = (mid >= ws) & (mid < we);
            ok &= (!want_mid | mid_in) & (!want_any | overlap);  // FTK_POLICY_FETCH: the query alone
            sum += ok ? (unsigned long long)wt : 0ull;
            cnt += (unsigned long long)(ok & (wt != 0));
        }
    }
    sum = wave_sum_down_u64(sum);
    cnt = wave_sum_down_u64(cnt);
    if (lane == 0) { red[0][wv] = sum; red[1][wv] = cnt; }
    __syncthreads();
    if (tid < 2) {
        unsigned long long t = 0;
#pragma unroll
        for (int k = 0; k < kWwThreads / 64; ++k) t += red[tid][k];
        unsigned long long* dst = tid == 0 ? sum_out : cnt_out;
        if (dst && t) atomicAdd(&dst[w], t);
    }
}

}  // namespace

void launch_frag_gc_weights(hipStream_t s, int n_cu, const ContigView& cv, const RefView& im, GcWeightParams p,
                            const uint32_t* packed, uint32_t* w_out, unsigned long long* n_zero) {
    if (cv.n <= 0) return;
    p.n_cells = (int)gc_weight_cells(p.len_lo, p.len_hi);
    p.in_lds = p.n_cells <= kGcWeightLdsCells;
    const size_t lds = p.in_lds ? (size_t)p.n_cells * 4 : 0;
    hipLaunchKernelGGL(frag_gc_weight_kernel, dim3(frag_pass_grid(n_cu, cv.n, kGcWeightThreads, lds)), dim3(kGcWeightThreads), lds, s,
                       cv, im, p, packed, w_out, n_zero);
}

int weighted_window_slices(int n_cu, long long n_win, long long n_frag) {
    // about four blocks per compute unit in all: 1 for 4 n_cu windows or more, 4 n_cu for one whole-contig window; never
    // more than the chunks the longest possible candidate range has
    const long long want = (4LL * n_cu + n_win - 1) / std::max(n_win, 1LL);
    const long long chunks = (n_frag + 3 + kChunk - 1) / kChunk;
    return (int)std::max(1LL, std::min({want, chunks, 65535LL}));
}

void launch_weighted_windows(hipStream_t s, const ContigView& cv, const uint32_t* weights, const int32_t* ws, const int32_t* we,
                             int n_win, int slices, const WeightedWinParams& p, unsigned long long* sum, unsigned long long* cnt) {
    if (n_win <= 0 || cv.n <= 0) return;
    const dim3 grid((unsigned)n_win, (unsigned)slices);
    if (p.bam) hipLaunchKernelGGL(weighted_window_kernel<true>, grid, dim3(kWwThreads), 0, s, cv, weights, ws, we, p, sum, cnt);
    else hipLaunchKernelGGL(weighted_window_kernel<false>, grid, dim3(kWwThreads), 0, s, cv, weights, ws, we, p, sum, cnt);
}

}  // namespace ftk
