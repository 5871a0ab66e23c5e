// One fragment's events in a WPS tile's difference array, as 32-bit tile-relative arithmetic (plain C++: the tile kernel
// in ftk_kernels.hip and tools/check_wps_events.cpp, which holds it against a naive 64-bit restatement without a GPU,
// read this one text).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define FTK_HD __host__ __device__ __forceinline__
#else
#define FTK_HD inline
#endif

namespace ftk {

// What a call fixes (wps_params validates and clamps it on the host):
//   0 <= hl, hr <= 2^19 (window_size <= 2^20), 0 <= min_len <= 2^30, 0 <= max_len <= 2^28, 0 <= mapq_min <= 256.
struct WpsEvCall {
    int hl, hr;
    int min_len, max_len, mapq_min;
};

// What a tile fixes.  t0: its first base, as int (see "ranges"); len_t: its bases, 1 .. T; [fmin, fmax): the fetch
// window of the owning interval, clamped to [-1, 2^30] (wps_clamp_coord: coordinates lie in [0, 2^30), so no comparison
// with one changes); edge: some candidate may fail a window test (wps_tile_is_edge) - an interior tile skips them.
struct WpsEvTile {
    int t0, len_t;
    int fmin, fmax;
    bool edge;
};

struct WpsEv {
    int a, b, c, e;  // tile-relative cells of the -1, +2, -2, +1 steps
};

FTK_HD int wps_clamp_coord(long long x) { return x < -1 ? -1 : x > (1LL << 30) ? (1 << 30) : (int)x; }

// Ranges, and why nothing below overflows an int.
//   Coordinates: 0 <= fs <= fe < 2^30 for every resident fragment (the load validates it), so 0 <= len < 2^30; the
//   packed word gives len <= 2046.  A fragment is a CANDIDATE of a tile only when the position index places it in
//   [t0 - 1 - hl - lmax - 512, t0 + len_t + hr + 512) (512: the index's bin), lmax <= max_len.  A tile with candidates
//   therefore has
//       -(T + 2^19 + 512) <= t0 < 2^30 + 2^28 + 2^19 + 513 < 2^31 - 2^29,
//   which (int)t0 holds exactly; a tile outside that range has no candidates and its t0 is never used.
//   r = fs - t0          in (-2^30 - 2^28 - 2^20, 2^30 + T + 2^20)
//   a = r - hr           > -2^30 - 2^28 - 2^21 > -2^31
//   b = r + hl + 1       < 2^30 + 2^21
//   c = a + len = fe - hr - t0, e = b + len = fe + hl + 1 - t0: fe < 2^30 bounds them like a and b.
//   The tests are differences of two such values with a true result inside the same bounds (mid - fmin is the
//   difference of two coordinates, whichever base both are written against), so no single operation leaves int.
//   q - mapq_min in [-256, 255]; len - min_len > -2^30; max_len - len > -2^30.

// x >= 0 <=> the fragment passes the filters and touches [t0 - 1, t0 + len_t).  The window tests
// (frag/_wps.py:156-157: midpoint in [fmin, fmax), the tabix overlap fs < fmax && fe > fmin) only in an edge tile.
// read1: the overlap is tested on the read1 columns instead (a BAM contig, by the caller), so only the midpoint here.
FTK_HD int wps_accept(const WpsEvCall& k, const WpsEvTile& t, int fs, int len, int q, const WpsEv& v, bool read1) {
    int x = (q - k.mapq_min) | (len - k.min_len) | (k.max_len - len) | v.e | (t.len_t - 1 - v.a);
    if (t.edge) {
        const int mid = fs + (len >> 1);  // == (fs + fe) >> 1
        x |= (mid - t.fmin) | (t.fmax - 1 - mid);
        if (!read1) x |= (t.fmax - 1 - fs) | (fs + len - 1 - t.fmin);
    }
    return x;
}

// BAM, an accepted fragment: do its read1 columns decide (overlap of read1 with [fmin, fmax), tested by the caller on
// the unclamped window)?  A fragment inside the fetch window holds its read1 there when the contig says so (r1_inside).
FTK_HD bool wps_read1_decides(const WpsEvTile& t, int fs, int len, bool r1_inside) {
    return t.edge && (!r1_inside || fs < t.fmin || fs + len > t.fmax);
}

FTK_HD WpsEv wps_events(const WpsEvCall& k, int t0, int fs, int len) {
    WpsEv v;
    const int r = fs - t0;
    v.a = r - k.hr;
    v.b = r + k.hl + 1;
    v.c = v.a + len;
    v.e = v.b + len;
    return v;
}

// The steps of an accepted fragment (x >= 0: e >= 0 and a < len_t <= T).  add(cell, value): cell < 0 is the carry
// into the tile (every step left of its first base), 0 <= cell < T a cell of the difference array; a step at T or
// beyond is dropped.  -1 on [a, b) and [c, e), +1 on [b, c): one interval [a, e) when the two ranges touch or overlap.
template <int T, class Add>
FTK_HD void wps_emit(const WpsEv& v, Add&& add) {
    add(v.a, -1);
    if (v.c >= v.b) {
        if (v.b < T) add(v.b, 2);
        if (v.c < T) add(v.c, -2);
    }
    if (v.e < T) add(v.e, 1);
}

// An INTERIOR tile: no candidate that passes the other tests can fail a window test.  Such a fragment has
// len <= lmax (lmax = min(max_len, the contig's longest fragment)), e >= 0 and a <= len_t - 1, i.e.
//   fe >= t0 - hl - 1, so fs >= lo := t0 - hl - 1 - lmax;   fs <= t0 + len_t - 1 + hr, so fe <= hi := t0 + len_t - 1 + hr + lmax.
// With lo > fmin and hi < fmax:  fmin < fs <= mid <= fe < fmax, hence mid in [fmin, fmax), fs < fmax, fe > fmin; and a
// BAM contig whose fragments hold their read1 (r1_inside) tests no read1 column for a fragment with fs >= fmin and
// fe <= fmax.  A BAM contig without that property tests read1 for every fragment: all its tiles are edge tiles.
// (64-bit, once per tile, on the unclamped window.)
FTK_HD bool wps_tile_is_edge(long long t0, int len_t, long long fmin, long long fmax, int hl, int hr, int lmax,
                             bool read1_everywhere) {
    const long long lo = t0 - hl - 1 - lmax, hi = t0 + len_t - 1 + hr + lmax;
    return read1_everywhere || !(lo > fmin && hi < fmax);
}

}  // namespace ftk
