// IFS fragmentation hotspots (ftk_ifs_hotspots, ftk_ifs_track): the rule of include/ftk.h, "IFS hotspots".
//
// One workgroup of 256 threads per tile of kCallTile windows of one interval, on the tile-call skeleton of
// ftk_tilecall.h: the candidates come from the position index, the midpoints are binned with LDS atomics, a DPP wave scan
// with a cross-wave carry turns the bins into prefix sums.  The kernel's own: the arrays hold BINS of `step` bases, not
// bases - two 32-bit tracks, c (midpoints) and i = c * L + l (the bin's IFS in units of 1 / L) - over the tile's kCallTile
// bins and a halo of HALO >= max(h1, h2) + m bins on either side, so that a window's n and I (m bins) and both
// backgrounds B (m + 2 h bins) are prefix differences inside the tile's own LDS.  Entry a of a track is bin
// k0 - HALO + a (k0: the tile's first window); window k0 + i is entries HALO + i .. HALO + i + m - 1.  Bins outside the
// contig hold no midpoint, so a background needs no clipping here - only n_b is clipped.
//
// Candidates: a midpoint lies in the bins the tile reads, [first, last), only when first - lmax < start < last (lmax: the
// longest fragment the filter admits - a midpoint may belong to a fragment that starts far in front of the tile).
//
// The same body serves the three passes.  Count and write decide window r * 256 + tid in thread tid: neighbouring lanes
// read neighbouring LDS words.  A wave's calls of round r are counted with a ballot; the 64 (round, wave) counts are
// scanned by wave 0 and a call's rank is its (round, wave) offset plus the calls of lower lanes - window order.  The count
// pass leaves two counters per tile (tested, called), a single workgroup scans the tiles' calls, the write pass places
// every call at offset + rank: no atomics on global memory anywhere, and both passes compute the same integers from the
// same columns.  The track pass stops behind the scan and writes n and I of every window.
//
// Counters are 32 bits wide: a background total below 2^32 is exact, because prefix sums are only ever subtracted
// (unsigned arithmetic wraps; the scan's additions are plain 32-bit adds).  LDS per workgroup and occupancy of the two
// instantiations: DESIGN.md, "IFS hotspots".
#include "ftk_hotspots.h"

namespace ftk {

namespace {

template <int HALO>
__global__ __launch_bounds__(256) void ifs_kernel(ContigView cv, IfsParams p, TileCallPlan pl, IfsOut o, int pass) {
    constexpr int T = kCallTile, W = T + 2 * HALO, NP = W / 1024, NT = 2, R = T / 256;
    static_assert(W % 1024 == 0 && R * 4 == 64, "the scan takes 1024 entries a trip; wave 0 scans the 64 (round, wave) counts");
    __shared__ __attribute__((aligned(16))) unsigned trk[NT][W];  // c and i per bin, then their inclusive prefix sums
    __shared__ unsigned wtot[NT][NP][4];
    __shared__ unsigned red[4][kIfsStats];
    __shared__ int wcnt[R * 4], wpre[R * 4];
    const int tid = threadIdx.x, wv = tid >> 6;
    const long long k = blockIdx.x;
    const int k0 = pl.tile_t0[k], len_t = pl.tile_len[k], m = p.m;
    const int base = k0 - HALO;  // bin of entry 0 (may be negative)
    // the entries this tile reads: 1 <= a_lo, a_hi <= W - 1 (HALO >= reach + m)
    const int a_lo = HALO - p.reach, a_hi = HALO + len_t + m - 1 + p.reach;
    const long long first = ((long long)k0 - p.reach) * p.step, last = ((long long)k0 + len_t + m - 1 + p.reach) * p.step;
    const int lo = index_bound(cv, first - p.lmax, 0), hi = index_bound(cv, last, 1);
    uint4* trk4 = reinterpret_cast<uint4*>(&trk[0][0]);
    for (int j = tid; j < NT * W / 4; j += 256) trk4[j] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    auto apply = [&](int fs, int fe, int q) {
        const int len = fe - fs;
        if (q < p.mapq_min || len < p.min_len || len > p.max_len || len <= 0) return;
        const long long mid = ((long long)fs + fe) >> 1;
        if (mid < 0 || mid >= p.chrom) return;
        const int a = (int)mid / p.step - base;
        if (a >= a_lo && a < a_hi) {
            atomicAdd(&trk[0][a], 1u);
            atomicAdd(&trk[1][a], p.L + (unsigned)len);
        }
    };
    tile_candidates(cv, p.packed, lo, hi, tid, apply);
    __syncthreads();
    tile_tracks_scan(trk, wtot, tid);
    __syncthreads();
    if (pass == kIfsTrack) {
        const long long at = pl.tile_out[k];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = r * 256 + tid, a = HALO + i;
            if (i < len_t) {
                o.n_out[at + i] = (int32_t)(trk[0][a + m - 1] - trk[0][a - 1]);
                o.ifs_out[at + i] = (int64_t)(trk[1][a + m - 1] - trk[1][a - 1]);
            }
        }
        return;
    }
    // the background of half-width h around window kw (entries a .. a + m - 1): B and the clipped n_b
    auto background = [&](int a, int kw, int h, unsigned& B, int& nb) {
        B = trk[1][a + m - 1 + h] - trk[1][a - h - 1];  // (a - h - 1 >= HALO - reach - 1 >= 0)
        nb = min(kw + m - 1 + h, p.n_bins - 1) - max(kw - h, 0) + 1;
    };
    // window kw at entry a.  0: not tested, 1: tested, 2: called
    auto decide = [&](int a, int kw, unsigned& n, unsigned& I) -> int {
        n = trk[0][a + m - 1] - trk[0][a - 1];  // (a >= HALO >= 1)
        I = trk[1][a + m - 1] - trk[1][a - 1];
        if (n < p.min_count) return 0;
        const unsigned q = I / p.L;
        if (q >= (unsigned)p.n_thr) return 1;
        const unsigned long long t = p.thr[q];
        if (t == 0 || (p.global_mean != 0 && t > p.global_mean)) return 1;
        unsigned B;
        int nb;
        background(a, kw, p.h1, B, nb);
        if (((unsigned long long)B * (unsigned)m << 10) < t * (unsigned long long)nb * p.L) return 1;
        if (p.h2) {
            background(a, kw, p.h2, B, nb);
            if (((unsigned long long)B * (unsigned)m << 10) < t * (unsigned long long)nb * p.L) return 1;
        }
        return 2;
    };
    unsigned flags = 0;  // bit r: window r * 256 + tid is called
    unsigned st[kIfsStats] = {0, 0};
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = r * 256 + tid;
        int res = 0;
        if (i < len_t) {
            unsigned n, I;
            res = decide(HALO + i, k0 + i, n, I);
        }
        st[0] += res > 0;
        st[1] += res == 2;
        flags |= (unsigned)(res == 2) << r;
        const int c = __popcll(__ballot(res == 2));
        tile_rank_count(wcnt, r, c, tid);
    }
    if (pass == kIfsCount) {
        tile_stats_reduce(st, red, pl.stats, k, tid);
        return;
    }
    tile_rank_scan(wcnt, wpre, tid);
    const long long off = pl.off[k];
    const unsigned long long lower = tile_lower_lanes(tid);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const bool called = flags >> r & 1;
        const unsigned long long b = __ballot(called);
        if (!called) continue;
        const long long at = off + wpre[r * 4 + wv] + __popcll(b & lower);
        const int i = r * 256 + tid, a = HALO + i, kw = k0 + i;
        unsigned n, I, B;
        int nb;
        decide(a, kw, n, I);
        o.run[at] = pl.tile_run[k];
        o.pos[at] = (int64_t)kw * p.step;
        o.count[at] = (int32_t)n;
        o.ifs[at] = (int64_t)I;
        background(a, kw, p.h1, B, nb);
        o.bg1[at] = (int64_t)B;
        o.nb1[at] = nb;
        B = 0, nb = 0;
        if (p.h2) background(a, kw, p.h2, B, nb);
        o.bg2[at] = (int64_t)B;
        o.nb2[at] = nb;
    }
}

// the exclusive prefix sum of the tiles' called windows and their total
__global__ __launch_bounds__(kCallScanWidth) void ifs_scan_kernel(TileCallPlan pl, int n_tiles) {
    tile_offsets_scan(n_tiles, pl.off, pl.total, [&](long long i) { return pl.stats[i * kIfsStats + 1]; });
}

// Passing fragments with a midpoint on the contig, their number and their lengths' sum: every workgroup strides over the
// columns and leaves one pair; the host adds the pairs.
__global__ __launch_bounds__(256) void ifs_totals_kernel(ContigView cv, IfsParams p, unsigned long long* partial) {
    __shared__ unsigned long long red[4][2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned long long cnt = 0, sum = 0;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < cv.n; i += (long long)gridDim.x * 256) {
        int fs, fe, q;
        tile_fetch(cv, p.packed, (int)i, fs, fe, q);
        const int len = fe - fs;
        if (q < p.mapq_min || len < p.min_len || len > p.max_len || len <= 0) continue;
        const long long mid = ((long long)fs + fe) >> 1;
        if (mid < 0 || mid >= p.chrom) continue;
        ++cnt;
        sum += (unsigned)len;
    }
    cnt = wave_sum_u64(cnt);
    sum = wave_sum_u64(sum);
    if (lane == 0) red[wv][0] = cnt, red[wv][1] = sum;
    __syncthreads();
    if (tid < 2) partial[2 * blockIdx.x + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

void launch_any(hipStream_t s, const ContigView& cv, const IfsParams& p, long long n_tiles, const TileCallPlan& pl, const IfsOut& out,
                int pass) {
    if (p.reach + p.m <= kIfsHaloSmall)
        hipLaunchKernelGGL((ifs_kernel<kIfsHaloSmall>), dim3((unsigned)n_tiles), dim3(256), 0, s, cv, p, pl, out, pass);
    else
        hipLaunchKernelGGL((ifs_kernel<kIfsHaloLarge>), dim3((unsigned)n_tiles), dim3(256), 0, s, cv, p, pl, out, pass);
}

}  // namespace

void launch_ifs_count(hipStream_t s, const ContigView& cv, const IfsParams& p, int n_tiles, const TileCallPlan& pl) {
    if (n_tiles <= 0) return;
    launch_any(s, cv, p, n_tiles, pl, IfsOut{}, kIfsCount);
    hipLaunchKernelGGL(ifs_scan_kernel, dim3(1), dim3(kCallScanWidth), 0, s, pl, n_tiles);
}

void launch_ifs_write(hipStream_t s, const ContigView& cv, const IfsParams& p, int n_tiles, const TileCallPlan& pl, const IfsOut& out) {
    if (n_tiles <= 0) return;
    launch_any(s, cv, p, n_tiles, pl, out, kIfsWrite);
}

void launch_ifs_track(hipStream_t s, const ContigView& cv, const IfsParams& p, long long n_tiles, const TileCallPlan& pl, const IfsOut& out) {
    if (n_tiles <= 0) return;
    launch_any(s, cv, p, n_tiles, pl, out, kIfsTrack);
}

void launch_ifs_totals(hipStream_t s, const ContigView& cv, const IfsParams& p, unsigned long long* partial) {
    hipLaunchKernelGGL(ifs_totals_kernel, dim3(kIfsTotalsBlocks), dim3(256), 0, s, cv, p, partial);
}

}  // namespace ftk
