// The tile-call skeleton prefends_kernel and ifs_kernel share (their .hip files include it through their launchers'
// headers; the host part of the same skeleton is run_tile_call of ftk_api.hip).  One workgroup of 256 threads per tile:
// it counts the tile's candidates into NT LDS tracks (tile_candidates), turns the tracks into inclusive prefix sums in
// place (tile_tracks_scan), decides its positions in rounds of 256, and either leaves the tile's counters
// (tile_stats_reduce; tile_offsets_scan then turns the tiles' calls into offsets) or ranks its calls in position order
// (tile_rank_count, tile_rank_scan, tile_lower_lanes) and writes them behind the tile's offset.  What a candidate adds
// and what a position is decided on is the kernel's own: it hands the helpers lambdas defined in the kernel, so
// everything inlines and what the lambdas capture by reference stays in registers.  The LDS arrays are the kernel's too.
#pragma once

#include "ftk_device.h"

namespace ftk {

// positions (windows) per workgroup (PREFENDS_TILE and HOTSPOTS_TILE of _lib.py)
constexpr int kCallTile = 4096;
// tiles of one batch: what the single workgroup of the scan walks, and the bound of a batch's plan in the scratch
constexpr int kCallBatchTiles = 4096;
constexpr int kCallScanWidth = 1024;

// One batch of tiles: what the passes hand each other, one entry per tile.
struct TileCallPlan {
    const int32_t* tile_t0;   // first position (window)
    const int32_t* tile_len;  // positions (1 .. kCallTile)
    const int32_t* tile_run;  // its interval's number
    const int64_t* tile_out;  // track pass only: where the tile's first window goes in the outputs
    uint32_t* stats;          // [n_tiles][counters of the rule] (count pass)
    int32_t* off;             // exclusive prefix sum of the tiles' calls (scan)
    int64_t* total;           // one word: calls of the batch (scan)
};

// the columns of fragment i, off the packed word or the wide columns
__device__ __forceinline__ void tile_fetch(const ContigView& cv, int packed, int i, int& fs, int& fe, int& q) {
    fs = cv.start[i];
    if (packed) {
        const int w = cv.lq[i];
        fe = fs + (w >> kLqBits);
        q = w & kLqMapqSat;
    } else {
        fe = cv.end[i];
        q = cv.mapq[i];
    }
}

// apply(start, end, mapq) for the candidates [lo, hi), thread tid taking lo + tid, lo + tid + 256, ...: the columns of
// its first four are requested in one batch (see depth_kernel), the rest one at a time.
template <class Apply>
__device__ __forceinline__ void tile_candidates(const ContigView& cv, int packed, int lo, int hi, int tid, Apply&& apply) {
    constexpr int PF = 4;
    int ps[PF], pe[PF], pq[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const int i = lo + tid + 256 * u;
        ps[u] = pe[u] = pq[u] = 0;
        if (i < hi) tile_fetch(cv, packed, i, ps[u], pe[u], pq[u]);
    }
#pragma unroll
    for (int u = 0; u < PF; ++u)
        if (lo + tid + 256 * u < hi) apply(ps[u], pe[u], pq[u]);
    for (int i = lo + PF * 256 + tid; i < hi; i += 256) {
        int fs, fe, q;
        tile_fetch(cv, packed, i, fs, fe, q);
        apply(fs, fe, q);
    }
}

// NT tracks of W entries each, in place: counts -> inclusive prefix sums.  Thread tid holds the entries
// j * 1024 + 4 * tid .. + 3 of every trip j; wtot carries the waves' totals.  The workgroup has synchronised behind the
// last count, and synchronises again before it reads a sum.
template <int NT, int W>
__device__ __forceinline__ void tile_tracks_scan(unsigned (&trk)[NT][W], unsigned (&wtot)[NT][W / 1024][4], int tid) {
    static_assert(W % 1024 == 0, "the scan takes 1024 entries a trip");
    constexpr int NP = W / 1024;
    const int lane = tid & 63, wv = tid >> 6;
    uint4* trk4 = reinterpret_cast<uint4*>(&trk[0][0]);
    uint4 v[NT][NP];
    unsigned ex[NT][NP];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            v[t][j] = trk4[t * (W / 4) + j * 256 + tid];
            const unsigned s = v[t][j].x + v[t][j].y + v[t][j].z + v[t][j].w;
            const unsigned incl = (unsigned)wave_incl_scan_dpp((int)s);
            ex[t][j] = incl - s;
            if (lane == 63) wtot[t][j][wv] = incl;
        }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        unsigned all = 0;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            unsigned carry = all;
#pragma unroll
            for (int w2 = 0; w2 < 4; ++w2) {
                const unsigned tt = wtot[t][j][w2];
                if (w2 < wv) carry += tt;
                all += tt;
            }
            uint4 q4;
            q4.x = carry + ex[t][j] + v[t][j].x;
            q4.y = q4.x + v[t][j].y;
            q4.z = q4.y + v[t][j].z;
            q4.w = q4.z + v[t][j].w;
            trk4[t * (W / 4) + j * 256 + tid] = q4;
        }
    }
}

// the workgroup's sums of N per-thread counters -> stats[k * N + c]
template <int N>
__device__ __forceinline__ void tile_stats_reduce(const unsigned (&mine)[N], unsigned (&red)[4][N], uint32_t* stats, long long k, int tid) {
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const unsigned s = wave_sum_u32(mine[c]);
        if ((tid & 63) == 0) red[tid >> 6][c] = s;
    }
    __syncthreads();
    if (tid < N) stats[k * N + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// The rank of a call: the calls of the (round, wave) pairs in front of its own - wcnt, one entry per pair, written
// round by round and scanned into wpre by wave 0 - plus the calls of the lower lanes of its own wave's ballot.
// (The arrays hold the 64 pairs one wave scans: 16 rounds of the workgroup's 4 waves.)
__device__ __forceinline__ void tile_rank_count(int (&wcnt)[64], int r, int calls, int tid) {
    if ((tid & 63) == 0) wcnt[r * 4 + (tid >> 6)] = calls;
}
__device__ __forceinline__ void tile_rank_scan(const int (&wcnt)[64], int (&wpre)[64], int tid) {
    __syncthreads();
    if (tid < 64) {
        const int x = wcnt[tid];
        wpre[tid] = wave_incl_scan_dpp(x) - x;
    }
    __syncthreads();
}
__device__ __forceinline__ unsigned long long tile_lower_lanes(int tid) { return (1ull << (tid & 63)) - 1; }

// One workgroup of kCallScanWidth threads, as many tiles a trip: the exclusive prefix sum of the tiles' calls into off
// and their sum into *total.  count(i): the calls of tile i.
template <class Count>
__device__ __forceinline__ void tile_offsets_scan(int n_tiles, int32_t* off, int64_t* total, Count&& count) {
    constexpr int NW = kCallScanWidth / 64;
    __shared__ int wt[NW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    long long carry = 0;
    for (int c0 = 0; c0 < n_tiles; c0 += kCallScanWidth) {
        const int i = c0 + tid;
        const int x = i < n_tiles ? (int)count((long long)i) : 0;
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
        if (i < n_tiles) off[i] = (int32_t)(carry + before + incl - x);
        carry += all;
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

}  // namespace ftk
