// Per-base fragment depth and its run-length encoding (ftk_depth, ftk_depth_runs).
//
// depth(b) = kept fragments with start <= b < end.  One workgroup of 256 threads per tile of kWpsTile bases, the tile
// skeleton of the WPS and cleavage kernels: the tile's candidates come from the position index, +1 at start and -1 at
// end go into an LDS difference array, the fragments that started in front of the tile are the carry-in, a DPP wave
// scan turns the differences into depths.  The same body serves three kernels:
//   per base   the depths, 16 bytes per lane and store
//   pass 1     per tile, how many runs open in it and where its first change of depth is
//   pass 2     every run, written by the base that opens it at its rank in the region
// A base opens a run when its depth differs from the base in front of it, that is when its entry of the difference
// array is not zero - the tile's first base included, whose entry holds the fragments that start or end exactly
// there, so no tile reads its neighbour's result.  The region's first base always opens one.  A run ends where the
// next change of depth is, whatever depth follows: inside the tile that is the next entry of the tile's own list of
// changes (kept in the LDS array once the differences are in registers), behind it the first change of a later tile,
// which the scan between the passes hands down (a suffix minimum), or the region's stop.  No atomics on global memory
// and no merging between tiles: a run that crosses tiles is written where it opens and nowhere else.
//
// Counters are 32 bits wide throughout.  cleavage_kernel packs two 16-bit counters into a word below 32 768
// candidates because it keeps TWO arrays per tile; here there is one, so 32-bit counters take the 16 KB per workgroup
// that kernel takes with its narrow layout: the eight workgroups a CU's 32 wave slots hold need 128 of its 160 KB.
// A depth above 65 535 (70 000 copies of one fragment) needs no second path.
#include <climits>

#include "ftk_depth.h"
#include "ftk_device.h"

namespace ftk {

namespace {

enum { kPerBase = 0, kCount = 1, kWrite = 2 };

template <int MODE>
__global__ __launch_bounds__(256) void depth_kernel(ContigView cv, DepthParams p, DepthRunPlan rp, int32_t* __restrict__ out,
                                                    int32_t* __restrict__ run_end, int32_t* __restrict__ run_depth) {
    constexpr int T = kWpsTile, NP = T / 1024;
    __shared__ __attribute__((aligned(16))) int dd[T];  // the differences; pass 2: then the positions of the tile's changes
    __shared__ int pre_s;
    __shared__ int wtot[NP][4];
    __shared__ int wcnt[NP][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long k = blockIdx.x;
    const long long t0 = p.start + k * T;
    const int len_t = (int)(min(t0 + (long long)T, p.stop) - t0);
    // candidates: start < t0 + len_t, end >= t0 (a fragment that ends exactly at t0 lowers the depth there)
    const int lo = index_bound(cv, t0 - (long long)p.lmax, 0), hi = index_bound(cv, t0 + len_t, 1);
    int4* dd4 = reinterpret_cast<int4*>(dd);
#pragma unroll
    for (int j = 0; j < NP; ++j) dd4[j * 256 + tid] = make_int4(0, 0, 0, 0);
    if (tid == 0) pre_s = 0;
    __syncthreads();
    auto apply = [&](int fs, int fe, int q) {
        const int len = fe - fs;
        if (q < p.mapq_min || len < p.min_len || len > p.max_len || len <= 0) return;
        const long long a = (long long)fs - t0, b = (long long)fe - t0;
        if (b < 0 || a >= len_t) return;
        if (a < 0) atomicAdd(&pre_s, 1);  // covers t0 - 1: the carry-in
        else atomicAdd(&dd[(int)a], 1);
        if (b < len_t) atomicAdd(&dd[(int)b], -1);
    };
    // the three columns of the first candidates requested in one batch (see cleave_tile)
    constexpr int PF = 4;
    int ps[PF], pe[PF], pq[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const int i = lo + tid + 256 * u;
        const bool ok = i < hi;
        ps[u] = ok ? cv.start[i] : 0;
        pe[u] = ok ? cv.end[i] : 0;
        pq[u] = ok ? (int)cv.mapq[i] : -1;
    }
#pragma unroll
    for (int u = 0; u < PF; ++u)
        if (lo + tid + 256 * u < hi) apply(ps[u], pe[u], pq[u]);
    for (int i = lo + PF * 256 + tid; i < hi; i += 256) apply(cv.start[i], cv.end[i], cv.mapq[i]);
    __syncthreads();
    // thread tid holds the bases j * 1024 + 4 * tid .. + 3 of every quarter j: 16-byte LDS reads and global stores
    int4 v[NP];
    int ex[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        v[j] = dd4[j * 256 + tid];
        const int s = v[j].x + v[j].y + v[j].z + v[j].w;
        const int incl = wave_incl_scan_dpp(s);
        ex[j] = incl - s;
        if (lane == 63) wtot[j][wv] = incl;
    }
    __syncthreads();  // (dd is free from here on: every difference is in a register)
    int g[NP][4];
    int base = pre_s;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        int carry = base;
#pragma unroll
        for (int w2 = 0; w2 < 4; ++w2) {
            const int tt = wtot[j][w2];
            if (w2 < wv) carry += tt;
            base += tt;
        }
        g[j][0] = carry + ex[j] + v[j].x;
        g[j][1] = g[j][0] + v[j].y;
        g[j][2] = g[j][1] + v[j].z;
        g[j][3] = g[j][2] + v[j].w;
    }
    if (MODE == kPerBase) {
        int32_t* dst = out + k * T;
        const bool vec_ok = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int i0 = j * 1024 + 4 * tid;
            if (i0 + 3 < len_t && vec_ok) {
                typedef int i4 __attribute__((ext_vector_type(4)));
                const i4 v4 = {g[j][0], g[j][1], g[j][2], g[j][3]};
                __builtin_nontemporal_store(v4, reinterpret_cast<i4*>(dst + i0));
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (i0 + c < len_t) dst[i0 + c] = g[j][c];
            }
        }
        return;
    }
    // bit c of chg / emit: base i0 + c changes the depth / opens a run that is kept.  Both counts ride in one word
    // (changes in the low half, kept runs in the high half; neither passes 4 096) through one scan.
    unsigned chg[NP], emit[NP];
    int rank[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int i0 = j * 1024 + 4 * tid;
        const int d[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
        chg[j] = emit[j] = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const bool ch = i0 + c < len_t && (d[c] != 0 || (k == 0 && i0 + c == 0));
            chg[j] |= (unsigned)ch << c;
            emit[j] |= (unsigned)(ch && (p.include_zero || g[j][c] != 0)) << c;
        }
        const int pc = __popc(chg[j]) | (__popc(emit[j]) << 16);
        const int incl = wave_incl_scan_dpp(pc);
        rank[j] = incl - pc;
        if (lane == 63) wcnt[j][wv] = incl;
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        int carry = total;
#pragma unroll
        for (int w2 = 0; w2 < 4; ++w2) {
            const int tt = wcnt[j][w2];
            if (w2 < wv) carry += tt;
            total += tt;
        }
        rank[j] += carry;
    }
    const int n_chg = total & 0xffff, n_emit = total >> 16;
    if (MODE == kCount) {
        if (tid == 0) {
            rp.cnt[k] = n_emit;
            if (n_chg == 0) rp.first[k] = INT_MAX;
        }
#pragma unroll
        for (int j = 0; j < NP; ++j)
            if (chg[j] && (rank[j] & 0xffff) == 0)  // one thread of the tile: the owner of its first change
                rp.first[k] = (int)(t0 + j * 1024 + 4 * tid + (__ffs(chg[j]) - 1));
        return;
    }
    // pass 2: the tile's changes as a list in LDS, so that a run finds where the next one starts
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        int r = rank[j] & 0xffff;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (chg[j] >> c & 1) dd[r++] = (int)(t0 + j * 1024 + 4 * tid + c);
    }
    __syncthreads();
    if (n_emit == 0) return;
    const int off = rp.off[k], behind = rp.next[k];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        int ra = rank[j] & 0xffff, re = rank[j] >> 16;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!(chg[j] >> c & 1)) continue;
            if (emit[j] >> c & 1) {
                const int o = off + re++;
                out[o] = dd[ra];
                run_end[o] = ra + 1 < n_chg ? dd[ra + 1] : behind;
                run_depth[o] = g[j][c];
            }
            ++ra;
        }
    }
}

// One workgroup, kDepthScanWidth tiles per trip: forwards the exclusive prefix sum of the tiles' run counts, then
// backwards the position of the first change of depth behind every tile.
__global__ __launch_bounds__(kDepthScanWidth) void depth_scan_kernel(DepthRunPlan rp, int n_tiles, int stop) {
    constexpr int W = kDepthScanWidth, NW = W / 64;
    __shared__ int wt[NW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int carry = 0;
    for (int c0 = 0; c0 < n_tiles; c0 += W) {
        const int i = c0 + tid;
        const int x = i < n_tiles ? rp.cnt[i] : 0;
        const int incl = wave_incl_scan_dpp(x);
        if (lane == 63) wt[wv] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w2 = 0; w2 < NW; ++w2) {
            const int tt = wt[w2];
            if (w2 < wv) before += tt;
            all += tt;
        }
        if (i < n_tiles) rp.off[i] = carry + before + incl - x;
        carry += all;
        __syncthreads();
    }
    if (tid == 0) *rp.total = carry;
    // thread tid takes the trip's tile W - 1 - tid: a prefix minimum in thread order is a suffix minimum in tile order
    int behind = stop;
    for (int c0 = (n_tiles - 1) / W * W; c0 >= 0; c0 -= W) {
        const int i = c0 + W - 1 - tid;
        int m = i < n_tiles ? rp.first[i] : INT_MAX;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(m, d, 64);
            if (lane >= d) m = min(m, y);
        }
        if (lane == 63) wt[wv] = m;
        int in_front = __shfl_up(m, 1, 64);  // of the tiles behind tile i within the wave
        if (lane == 0) in_front = INT_MAX;
        __syncthreads();
        int all = INT_MAX;
#pragma unroll
        for (int w2 = 0; w2 < NW; ++w2) {
            const int tt = wt[w2];
            if (w2 < wv) in_front = min(in_front, tt);
            all = min(all, tt);
        }
        if (i < n_tiles) rp.next[i] = min(behind, in_front);
        behind = min(behind, all);
        __syncthreads();
    }
}

}  // namespace

void launch_depth(hipStream_t s, const ContigView& cv, const DepthParams& p, int64_t n_tiles, int32_t* depth) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL((depth_kernel<kPerBase>), dim3((unsigned)n_tiles), dim3(256), 0, s, cv, p, DepthRunPlan{}, depth, nullptr,
                       nullptr);
}

void launch_depth_count(hipStream_t s, const ContigView& cv, const DepthParams& p, int64_t n_tiles, const DepthRunPlan& rp) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL((depth_kernel<kCount>), dim3((unsigned)n_tiles), dim3(256), 0, s, cv, p, rp, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(depth_scan_kernel, dim3(1), dim3(kDepthScanWidth), 0, s, rp, (int)n_tiles, (int)p.stop);
}

void launch_depth_write(hipStream_t s, const ContigView& cv, const DepthParams& p, int64_t n_tiles, const DepthRunPlan& rp,
                        int32_t* run_start, int32_t* run_end, int32_t* run_depth) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL((depth_kernel<kWrite>), dim3((unsigned)n_tiles), dim3(256), 0, s, cv, p, rp, run_start, run_end, run_depth);
}

}  // namespace ftk
