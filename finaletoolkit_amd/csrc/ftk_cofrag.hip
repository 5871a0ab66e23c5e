// Pairwise two-sample Kolmogorov-Smirnov numerators of histogram rows (ftk_hist_ks, ftk_cofrag): the rule is in
// include/ftk.h under "co-fragmentation".  With C(i, l) the prefix sums of row i and n(i) its total,
//     K(i, j) = max over l of |C(i, l) n(j) - C(j, l) n(i)|,   at(i, j) = the smallest l that attains it.
// Every n(i) is below 2^31 and so is every prefix: the two products are 32 x 32 -> 64 multiplies, each below 2^62, and
// their difference fits the signed 64-bit word it is taken in.
//
// ks_rows_kernel    a wave per row: the lanes take 64 lengths a step (one coalesced read, the wave scan on DPP, a carry)
//                   and write the prefixes LENGTH-major - prefix[l][i] - so that at one length the rows of a tile are
//                   adjacent words.  The row's total is summed in 64 bits beside the scan; a total of 2^31 or more
//                   lowers the call's flag to the row's number and the host stops there.
// ks_tile_kernel    arrangement 1, what ftk_hist_ks launches: a workgroup of 16 x 16 threads per T x T tile (T = 64) of
//                   the upper triangle.  Per chunk of kKsChunk lengths the T row-prefixes and the T column-prefixes
//                   are staged as [side][length][row] - 2 x 32 x 64 words, 16 KiB, a straight copy of 256-byte pieces
//                   of the image - while the chunk before is computed on (the next chunk's 4 x 16 bytes per thread
//                   wait in registers).  Thread (ty, tx) owns rows 4 ty .. + 3 and columns 4 tx .. + 3: per length ONE
//                   16-byte read of each side.  The 16 lanes of a read group that differ in tx take the 16 slots of one
//                   256-byte bank row, the lanes that share tx (or ty) read one address, which is a broadcast: no
//                   conflicts.  n(i), n(j), 16 running maxima and their lengths stay in registers; a pair step is two
//                   multiply-adds, the absolute value, one 64-bit compare and three selects.  The maximum moves on a
//                   strict > as l ascends - within a chunk and from chunk to chunk alike - so `at` is the leftmost.
//                   A diagonal tile leaves the threads below its diagonal idle and writes its cells i <= j; every
//                   tile writes (i, j) and (j, i).
// ks_pair_kernel    arrangement 0 (FTK_COFRAG_ARRANGE=0): a thread per pair i <= j - a row of the grid per i, lanes
//                   along j - reading both prefix columns from memory at every length: prefix[l][i] is one address
//                   per wave, prefix[l][j] coalesced.  The cross-check inside the library.
#include <algorithm>

#include "ftk_cofrag.h"
#include "ftk_device.h"

namespace ftk {

namespace {

constexpr int kKsQuads = kKsTile / kKsBlock;                                    // threads along a tile's edge
constexpr int kKsStageQuads = 2 * kKsChunk * kKsQuads;                          // 16-byte pieces of one chunk
constexpr int kKsStagePerThread = kKsStageQuads / kKsThreads;
static_assert(kKsQuads * kKsQuads == kKsThreads && kKsBlock == 4, "a thread reads its four rows as one uint4");
static_assert(kKsStageQuads % kKsThreads == 0, "every thread stages the same number of pieces");

// one length of one pair: the running maximum moves on a strictly larger |c_i n_j - c_j n_i|.  All four factors are
// below 2^31, so the products are the same taken unsigned - two v_mad_u64_u32 - and their difference is the signed value.
__device__ __forceinline__ void ks_step(uint32_t ci, uint32_t cj, uint32_t ni, uint32_t nj, int l, unsigned long long& best, int& at) {
    const long long v = (long long)((unsigned long long)ci * nj - (unsigned long long)cj * ni);
    const unsigned long long m = (unsigned long long)(v < 0 ? -v : v);
    if (m > best) {
        best = m;
        at = l;
    }
}

__global__ __launch_bounds__(kKsRowThreads) void ks_rows_kernel(const uint32_t* __restrict__ hist, int n_rows, int n_bins, int pitch,
                                                                uint32_t* __restrict__ prefix, uint32_t* __restrict__ n32,
                                                                int32_t* __restrict__ bad_row) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (kKsRowThreads / 64) + (threadIdx.x >> 6);
    if (row >= n_rows) return;  // (a whole wave)
    const uint32_t* h = hist + (size_t)row * n_bins;
    unsigned long long total = 0;
    uint32_t carry = 0;
    for (int l0 = 0; l0 < n_bins; l0 += 64) {
        const int l = l0 + lane;
        const uint32_t v = l < n_bins ? h[l] : 0u;
        const uint32_t incl = (uint32_t)wave_incl_scan_dpp((int)v) + carry;
        if (l < n_bins) prefix[(size_t)l * pitch + row] = incl;
        total += v;
        carry = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    total = wave_sum_u64(total);
    if (lane == 0) {
        n32[row] = (uint32_t)total;
        if (total >= (1ull << 31)) atomicMin(bad_row, row);
    }
}

__global__ __launch_bounds__(kKsThreads) void ks_pair_kernel(const uint32_t* __restrict__ prefix, const uint32_t* __restrict__ n32,
                                                             int n_rows, int n_bins, int pitch, long long* __restrict__ k_out,
                                                             int32_t* __restrict__ at_out, long long* __restrict__ n_out) {
    const int i = blockIdx.y, j = blockIdx.x * kKsThreads + threadIdx.x;
    if (j >= n_rows || j < i) return;
    const uint32_t ni = n32[i], nj = n32[j];
    unsigned long long best = 0;
    int at = 0;
    for (int l = 0; l < n_bins; ++l) {
        const uint32_t* p = prefix + (size_t)l * pitch;
        ks_step(p[i], p[j], ni, nj, l, best, at);
    }
    k_out[(size_t)i * n_rows + j] = (long long)best;
    k_out[(size_t)j * n_rows + i] = (long long)best;
    if (at_out) {
        at_out[(size_t)i * n_rows + j] = at;
        at_out[(size_t)j * n_rows + i] = at;
    }
    if (i == j) n_out[i] = (long long)ni;
}

// the pieces of chunk l0 this thread stages: piece u = side * (chunk * quads) + length * quads + quad
__device__ __forceinline__ void ks_stage_load(const uint32_t* __restrict__ prefix, int pitch, int n_bins, int l0, int i0, int j0, int tid,
                                              uint4 (&held)[kKsStagePerThread]) {
#pragma unroll
    for (int u = 0; u < kKsStagePerThread; ++u) {
        const int piece = tid + u * kKsThreads;
        const int side = piece / (kKsChunk * kKsQuads), rest = piece % (kKsChunk * kKsQuads);
        const int l = l0 + rest / kKsQuads, q = rest % kKsQuads;
        held[u] = make_uint4(0u, 0u, 0u, 0u);
        // (row0 + 4 q + 3 < pitch: the image holds whole tiles; its base and pitch are multiples of 16 bytes)
        if (l < n_bins) held[u] = *reinterpret_cast<const uint4*>(prefix + (size_t)l * pitch + (side ? j0 : i0) + kKsBlock * q);
    }
}

__global__ __launch_bounds__(kKsThreads) void ks_tile_kernel(const uint32_t* __restrict__ prefix, const uint32_t* __restrict__ n32,
                                                             int n_rows, int n_bins, int pitch, long long* __restrict__ k_out,
                                                             int32_t* __restrict__ at_out, long long* __restrict__ n_out) {
    __shared__ uint4 stage[kKsStageQuads];  // [side][length][quad of rows]
    const int tid = threadIdx.x, ty = tid / kKsQuads, tx = tid % kKsQuads;
    // tile (ti, tj), ti <= tj, of the upper triangle: row ti of the tiles holds nt - ti of them
    const int nt = pitch / kKsTile;
    int ti = 0, rest = (int)blockIdx.x;
    while (rest >= nt - ti) {
        rest -= nt - ti;
        ++ti;
    }
    const int tj = ti + rest, i0 = ti * kKsTile, j0 = tj * kKsTile;
    const bool diag = ti == tj, active = !diag || ty <= tx;
    uint32_t ni[kKsBlock], nj[kKsBlock];
    unsigned long long best[kKsBlock][kKsBlock];
    int at[kKsBlock][kKsBlock];
#pragma unroll
    for (int a = 0; a < kKsBlock; ++a) {
        // (n32 holds `pitch` entries; those behind n_rows are never written and belong to pairs that are never stored)
        ni[a] = n32[i0 + kKsBlock * ty + a];
        nj[a] = n32[j0 + kKsBlock * tx + a];
#pragma unroll
        for (int b = 0; b < kKsBlock; ++b) {
            best[a][b] = 0;
            at[a][b] = 0;
        }
    }
    uint4 held[kKsStagePerThread];
    ks_stage_load(prefix, pitch, n_bins, 0, i0, j0, tid, held);
    for (int l0 = 0; l0 < n_bins; l0 += kKsChunk) {
#pragma unroll
        for (int u = 0; u < kKsStagePerThread; ++u) stage[tid + u * kKsThreads] = held[u];
        __syncthreads();
        if (l0 + kKsChunk < n_bins) ks_stage_load(prefix, pitch, n_bins, l0 + kKsChunk, i0, j0, tid, held);
        if (active) {
            const int nl = min(kKsChunk, n_bins - l0);
#pragma unroll 2
            for (int l = 0; l < nl; ++l) {
                const uint4 ra = stage[l * kKsQuads + ty], rb = stage[(kKsChunk + l) * kKsQuads + tx];
                const uint32_t ci[kKsBlock] = {ra.x, ra.y, ra.z, ra.w}, cj[kKsBlock] = {rb.x, rb.y, rb.z, rb.w};
#pragma unroll
                for (int a = 0; a < kKsBlock; ++a)
#pragma unroll
                    for (int b = 0; b < kKsBlock; ++b) ks_step(ci[a], cj[b], ni[a], nj[b], l0 + l, best[a][b], at[a][b]);
            }
        }
        __syncthreads();  // the chunk is read before the next one overwrites it
    }
    if (diag && tid < kKsTile && i0 + tid < n_rows) n_out[i0 + tid] = (long long)n32[i0 + tid];
    if (!active) return;
#pragma unroll
    for (int a = 0; a < kKsBlock; ++a)
#pragma unroll
        for (int b = 0; b < kKsBlock; ++b) {
            const int i = i0 + kKsBlock * ty + a, j = j0 + kKsBlock * tx + b;
            if (i >= n_rows || j >= n_rows || i > j) continue;
            k_out[(size_t)i * n_rows + j] = (long long)best[a][b];
            k_out[(size_t)j * n_rows + i] = (long long)best[a][b];
            if (at_out) {
                at_out[(size_t)i * n_rows + j] = at[a][b];
                at_out[(size_t)j * n_rows + i] = at[a][b];
            }
        }
}

}  // namespace

void launch_ks_rows(hipStream_t s, const uint32_t* hist, int n_rows, int n_bins, uint32_t* prefix, uint32_t* n32, int32_t* bad_row) {
    constexpr int per_block = kKsRowThreads / 64;
    hipLaunchKernelGGL(ks_rows_kernel, dim3((unsigned)((n_rows + per_block - 1) / per_block)), dim3(kKsRowThreads), 0, s, hist, n_rows,
                       n_bins, ks_pitch(n_rows), prefix, n32, bad_row);
}

void launch_ks_pairs(hipStream_t s, int arrangement, const uint32_t* prefix, const uint32_t* n32, int n_rows, int n_bins,
                     long long* k_out, int32_t* at_out, long long* n_out) {
    const int pitch = ks_pitch(n_rows);
    if (arrangement == kKsTiles) {
        const int nt = pitch / kKsTile;
        hipLaunchKernelGGL(ks_tile_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(kKsThreads), 0, s, prefix, n32, n_rows, n_bins,
                           pitch, k_out, at_out, n_out);
    } else {
        hipLaunchKernelGGL(ks_pair_kernel, dim3((unsigned)((n_rows + kKsThreads - 1) / kKsThreads), (unsigned)n_rows), dim3(kKsThreads), 0,
                           s, prefix, n32, n_rows, n_bins, pitch, k_out, at_out, n_out);
    }
}

}  // namespace ftk
