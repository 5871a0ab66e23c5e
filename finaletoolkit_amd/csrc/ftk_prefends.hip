// Preferred fragment ends (ftk_preferred_ends): the rule of include/ftk.h, "preferred ends".
//
// One workgroup of 256 threads per tile of kCallTile positions of one interval, on the tile-call skeleton of
// ftk_tilecall.h: the candidates come from the position index, the ends are counted with LDS atomics, a DPP wave scan with
// a cross-wave carry turns the counts into prefix sums.  The kernel's own: the arrays hold the tile AND a halo of
// HALO >= h positions on either side, so that T(b) = P[b + h] - P[b - h - 1] for every position of the tile comes out of
// the tile's own LDS (positions outside the contig hold no end, so the window needs no clipping here - only n_w is
// clipped); and there are two tracks in split mode.  Entry a of a track is contig position t0 - HALO + a.
//
// Candidates: a fragment's U end is `start`, its D end `end - 1`; either lies in [t0 - h, t0 + len + h) only when
// t0 - h - lmax < start < t0 + len + h (lmax: the longest fragment the filter admits, as in depth_kernel - a D end may
// belong to a fragment that starts far in front of the tile).
//
// The same body serves both passes (`write`).  Thread tid decides the positions r * 256 + tid: neighbouring lanes read
// neighbouring LDS words.  A wave's calls of round r are counted with two ballots; the 64 (round, wave) counts are scanned
// by wave 0 and a call's rank is its (round, wave) offset plus the calls of lower lanes - position order, kind 0 in front
// of kind 1 on one position.  The count pass leaves six counters per tile (U ends, D ends, tested a / b, calls a / b),
// a single workgroup scans the tiles' calls, the write pass places every call at offset + rank: no atomics on global
// memory anywhere, and both passes compute the same integers from the same columns.
//
// Counters are 32 bits wide: counts up to 2^31 - 1 per position are exact, and a window total below 2^32 is exact too,
// because prefix sums are only ever subtracted (unsigned arithmetic wraps; the scan's additions are plain 32-bit adds).
// LDS per workgroup and occupancy of the four instantiations: DESIGN.md, "preferred ends".
#include "ftk_prefends.h"

namespace ftk {

namespace {

template <int HALO, bool SPLIT>
__global__ __launch_bounds__(256) void prefends_kernel(ContigView cv, PrefParams p, TileCallPlan pl, PrefOut o, int write) {
    constexpr int T = kCallTile, W = T + 2 * HALO, NP = W / 1024, NT = SPLIT ? 2 : 1, R = T / 256;
    static_assert(W % 1024 == 0 && R * 4 == 64, "the scan takes 1024 entries a trip; wave 0 scans the 64 (round, wave) counts");
    __shared__ __attribute__((aligned(16))) unsigned trk[NT][W];  // the counts, then their inclusive prefix sums
    __shared__ unsigned wtot[NT][NP][4];
    __shared__ unsigned red[4][kPrefStats];
    __shared__ int wcnt[R * 4], wpre[R * 4];
    const int tid = threadIdx.x, wv = tid >> 6;
    const long long k = blockIdx.x;
    const int t0 = pl.tile_t0[k], len_t = pl.tile_len[k], h = p.half;
    const int base = t0 - HALO;                          // contig position of entry 0 (may be negative)
    const int a_lo = HALO - h, a_hi = HALO + len_t + h;  // the entries this tile reads: 0 <= a_lo, a_hi <= W
    const int lo = index_bound(cv, (long long)t0 - h - p.lmax, 0), hi = index_bound(cv, (long long)t0 + len_t + h, 1);
    uint4* trk4 = reinterpret_cast<uint4*>(&trk[0][0]);
    for (int j = tid; j < NT * W / 4; j += 256) trk4[j] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    unsigned nu = 0, nd = 0;  // ends on the tile's own positions
    auto apply = [&](int fs, int fe, int q) {
        const int len = fe - fs;
        if (q < p.mapq_min || len < p.min_len || len > p.max_len || len <= 0) return;
        const int fd = fe - 1;
        if (fs >= 0 && fs < p.chrom) {
            const int a = fs - base;
            if (a >= a_lo && a < a_hi) {
                atomicAdd(&trk[0][a], 1u);
                nu += a >= HALO && a < HALO + len_t;
            }
        }
        if (fd >= 0 && fd < p.chrom) {
            const int a = fd - base;
            if (a >= a_lo && a < a_hi) {
                atomicAdd(&trk[NT - 1][a], 1u);
                nd += a >= HALO && a < HALO + len_t;
            }
        }
    };
    tile_candidates(cv, p.packed, lo, hi, tid, apply);
    __syncthreads();
    tile_tracks_scan(trk, wtot, tid);
    __syncthreads();
    // e, T and n_w of entry a (position b) of track t.  0: not tested, 1: tested, 2: called
    auto decide = [&](int t, int a, int b, unsigned& e, unsigned& tot, int& nw) -> int {
        e = trk[t][a] - trk[t][a - 1];  // (a >= HALO >= 1)
        if (e < p.min_count) return 0;
        const int below = a - h - 1;  // >= -1
        tot = trk[t][a + h] - (below < 0 ? 0u : trk[t][below]);
        nw = min(b + h, p.chrom - 1) - max(b - h, 0) + 1;
        const unsigned long long th = p.thr[min(e, (unsigned)(p.n_thr - 1))];
        return ((unsigned long long)tot << 20) <= th * (unsigned long long)nw ? 2 : 1;
    };
    unsigned flags = 0;  // bit 2 r: position r * 256 + tid is called on track a, bit 2 r + 1: on track b
    unsigned st[4] = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = r * 256 + tid;
        int ra = 0, rb = 0;
        if (i < len_t) {
            unsigned e, tot;
            int nw;
            ra = decide(0, HALO + i, t0 + i, e, tot, nw);
            if (SPLIT) rb = decide(NT - 1, HALO + i, t0 + i, e, tot, nw);
        }
        st[0] += ra > 0;
        st[1] += rb > 0;
        st[2] += ra == 2;
        st[3] += rb == 2;
        flags |= (unsigned)(ra == 2) << (2 * r) | (unsigned)(rb == 2) << (2 * r + 1);
        const int c = __popcll(__ballot(ra == 2)) + __popcll(__ballot(rb == 2));
        tile_rank_count(wcnt, r, c, tid);
    }
    if (!write) {
        const unsigned mine[kPrefStats] = {nu, nd, st[0], st[1], st[2], st[3]};
        tile_stats_reduce(mine, red, pl.stats, k, tid);
        return;
    }
    tile_rank_scan(wcnt, wpre, tid);
    const long long off = pl.off[k];
    const unsigned long long lower = tile_lower_lanes(tid);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const bool ca = flags >> (2 * r) & 1, cb = flags >> (2 * r + 1) & 1;
        const unsigned long long ba = __ballot(ca), bb = __ballot(cb);
        if (!(ca || cb)) continue;
        long long at = off + wpre[r * 4 + wv] + __popcll(ba & lower) + __popcll(bb & lower);
        const int i = r * 256 + tid;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (!(t == 0 ? ca : cb)) continue;
            unsigned e, tot;
            int nw;
            decide(t, HALO + i, t0 + i, e, tot, nw);
            o.run[at] = pl.tile_run[k];
            o.pos[at] = t0 + i;
            o.kind[at] = SPLIT ? t : 2;
            o.count[at] = (int32_t)e;
            o.total[at] = (int64_t)tot;
            o.n_w[at] = nw;
            ++at;
        }
    }
}

// the exclusive prefix sum of the tiles' calls (both tracks) and their total
__global__ __launch_bounds__(kCallScanWidth) void prefends_scan_kernel(TileCallPlan pl, int n_tiles) {
    tile_offsets_scan(n_tiles, pl.off, pl.total, [&](long long i) { return pl.stats[i * kPrefStats + 4] + pl.stats[i * kPrefStats + 5]; });
}

template <int HALO, bool SPLIT>
void launch_pass(hipStream_t s, const ContigView& cv, const PrefParams& p, int n_tiles, const TileCallPlan& pl, const PrefOut& out,
                 int write) {
    hipLaunchKernelGGL((prefends_kernel<HALO, SPLIT>), dim3((unsigned)n_tiles), dim3(256), 0, s, cv, p, pl, out, write);
}

void launch_any(hipStream_t s, const ContigView& cv, const PrefParams& p, int n_tiles, const TileCallPlan& pl, const PrefOut& out,
                int write) {
    if (p.half <= kPrefHaloSmall) {
        if (p.split) launch_pass<kPrefHaloSmall, true>(s, cv, p, n_tiles, pl, out, write);
        else launch_pass<kPrefHaloSmall, false>(s, cv, p, n_tiles, pl, out, write);
    } else {
        if (p.split) launch_pass<kPrefHaloLarge, true>(s, cv, p, n_tiles, pl, out, write);
        else launch_pass<kPrefHaloLarge, false>(s, cv, p, n_tiles, pl, out, write);
    }
}

}  // namespace

void launch_prefends_count(hipStream_t s, const ContigView& cv, const PrefParams& p, int n_tiles, const TileCallPlan& pl) {
    if (n_tiles <= 0) return;
    launch_any(s, cv, p, n_tiles, pl, PrefOut{}, 0);
    hipLaunchKernelGGL(prefends_scan_kernel, dim3(1), dim3(kCallScanWidth), 0, s, pl, n_tiles);
}

void launch_prefends_write(hipStream_t s, const ContigView& cv, const PrefParams& p, int n_tiles, const TileCallPlan& pl,
                           const PrefOut& out) {
    if (n_tiles <= 0) return;
    launch_any(s, cv, p, n_tiles, pl, out, 1);
}

}  // namespace ftk
