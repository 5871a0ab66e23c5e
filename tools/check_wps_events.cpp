// Stand-alone check (plain C++, no GPU) of a fragment's events in a WPS tile as the tile kernel computes them
// (finaletoolkit_amd/csrc/ftk_wps_events.h: 32-bit tile-relative cells, one OR-ed sign test, the fetch-window tests only
// in edge tiles) against a deliberately naive 64-bit restatement of the form the kernel had before: a chain of compares
// on long long positions and a three-way ladder per event.  Exhaustive over the places where the two could part:
// every offset of a fragment against its tile, lengths around the window size and the packed column's limit, tiles at
// 0, 4096 and just below 2^30, partial tiles, edge and interior tiles, and the fetch window at every off-by-one around
// a fragment's start, midpoint and end.  Built with -fsanitize=undefined,address it also shows that no int overflows.
//   c++ -std=c++17 -I finaletoolkit_amd/csrc tools/check_wps_events.cpp -o check_wps_events && ./check_wps_events
#include <algorithm>
#include <cstdio>
#include <vector>

#include "ftk_wps_events.h"

using namespace ftk;

constexpr int T = 4096;
typedef long long ll;

static ll bad = 0, cases = 0, interior_cases = 0, accepted = 0;

struct Steps {  // what one fragment adds: to the carry cell, and up to four (cell, value) steps of the array, in order
    int carry = 0, n = 0, cell[4] = {0, 0, 0, 0}, val[4] = {0, 0, 0, 0};
    void add(ll c, int v) {
        if (c < 0) carry += v;
        else { cell[n] = (int)c; val[n] = v; ++n; }
    }
    bool operator==(const Steps& o) const {
        if (carry != o.carry || n != o.n) return false;
        for (int i = 0; i < n; ++i)
            if (cell[i] != o.cell[i] || val[i] != o.val[i]) return false;
        return true;
    }
};

struct Call {
    int hl, hr, min_len, max_len, mapq_min;
};
struct Tile {
    ll t0, fmin, fmax;
    int len_t;
};
struct Read1 {  // a BAM contig's read1 columns for this fragment (on = false: a tabix contig)
    bool on = false, inside = false;
    ll s = 0, e = 0;
};

// the old form, every position long long
static Steps naive(const Call& p, const Tile& ti, ll fs, ll fe, int q, const Read1& r1) {
    Steps out;
    const ll len = fe - fs;
    const ll mid = (fs + fe) >> 1;
    if (q < p.mapq_min || len < p.min_len || len > p.max_len || mid < ti.fmin || mid >= ti.fmax) return out;
    if (r1.on) {
        if (!r1.inside || fs < ti.fmin || fe > ti.fmax) {
            if (!(r1.s < ti.fmax && r1.e > ti.fmin)) return out;
        }
    } else if (!(fs < ti.fmax && fe > ti.fmin)) {
        return out;
    }
    const ll a = fs - p.hr - ti.t0;
    const ll b = fs + p.hl + 1 - ti.t0;
    const ll c = fe - p.hr - ti.t0;
    const ll e = fe + p.hl + 1 - ti.t0;
    if (e <= -1 || a >= ti.len_t) return out;
    if (a < 0) out.add(-1, -1); else if (a < T) out.add(a, -1);
    if (c >= b) {
        if (b < 0) out.add(-1, 2); else if (b < T) out.add(b, 2);
        if (c < 0) out.add(-1, -2); else if (c < T) out.add(c, -2);
    }
    if (e < 0) out.add(-1, 1); else if (e < T) out.add(e, 1);
    return out;
}

// the kernel's form: the header's text, driven the way wps_block drives it
static Steps lean(const Call& p, const Tile& ti, int lmax, int fs, int len, int q, const Read1& r1) {
    Steps out;
    const WpsEvCall K{p.hl, p.hr, p.min_len, p.max_len, p.mapq_min};
    WpsEvTile t;
    t.t0 = (int)ti.t0;
    t.len_t = ti.len_t;
    t.fmin = wps_clamp_coord(ti.fmin);
    t.fmax = wps_clamp_coord(ti.fmax);
    t.edge = wps_tile_is_edge(ti.t0, ti.len_t, ti.fmin, ti.fmax, p.hl, p.hr, lmax, r1.on && !r1.inside);
    interior_cases += !t.edge;
    const WpsEv v = wps_events(K, t.t0, fs, len);
    if (wps_accept(K, t, fs, len, q, v, r1.on) < 0) return out;
    if (r1.on && wps_read1_decides(t, fs, len, r1.inside)) {
        if (!(r1.s < ti.fmax && r1.e > ti.fmin)) return out;
    }
    wps_emit<T>(v, [&](int cell, int val) { out.add(cell, val); });
    return out;
}

static void one(const Call& p, const Tile& ti, int lmax, ll fs, int len, int q, const Read1& r1) {
    const Steps want = naive(p, ti, fs, fs + len, q, r1), got = lean(p, ti, lmax, (int)fs, len, q, r1);
    ++cases;
    accepted += want.n > 0 || want.carry != 0;
    if (!(got == want)) {
        if (bad < 20)
            printf("t0 %lld len_t %d window [%lld, %lld) hl %d hr %d fs %lld len %d q %d filters %d %d %d read1 %d %d [%lld, %lld): "
                   "carry %d / %d, steps %d / %d\n", ti.t0, ti.len_t, ti.fmin, ti.fmax, p.hl, p.hr, fs, len, q, p.min_len,
                   p.max_len, p.mapq_min, r1.on, r1.inside, r1.s, r1.e, got.carry, want.carry, got.n, want.n);
        ++bad;
    }
}

static Call call_for(int W, int min_len, int max_len, int mapq_min) {
    Call p;
    if (W & 1) p.hl = p.hr = (W - 1) / 2;
    else { p.hl = W / 2; p.hr = W / 2 - 1; }
    p.min_len = min_len; p.max_len = max_len; p.mapq_min = mapq_min;
    return p;
}

int main() {
    const ll TOP = 1LL << 30;
    const int LONGEST = 2046;  // the contig's longest fragment (the packed column's limit)
    for (int W : {1, 2, 119, 120, 121, 1000}) {
        std::vector<int> lens = {0, 1, W - 2, W - 1, W, W + 1, 119, 120, 121, 179, 180, 181, 2046};
        lens.erase(std::remove_if(lens.begin(), lens.end(), [](int l) { return l < 0; }), lens.end());
        std::sort(lens.begin(), lens.end());
        lens.erase(std::unique(lens.begin(), lens.end()), lens.end());
        for (ll t0 : {0LL, 4096LL, TOP - 4096}) {
            for (int len_t : {T, T - 1, 100, 1}) {
                // ---- every offset, three windows: the whole contig (interior tiles where the fragments allow), one
                //      that makes the tile just interior, one that makes it just an edge tile on both sides
                for (int wide_max : {0, 1}) {
                    const Call p = call_for(W, 0, wide_max ? (1 << 28) : 2046, 0);
                    const int lmax = std::min(p.max_len, LONGEST);
                    const ll lo = t0 - p.hl - 1 - lmax, hi = t0 + len_t - 1 + p.hr + lmax;
                    const Tile tiles[3] = {{t0, 0, TOP + 12345, len_t}, {t0, lo - 1, hi + 1, len_t}, {t0, lo, hi, len_t}};
                    for (const Tile& ti : tiles)
                        for (int r = -2300; r <= T + 200; ++r)
                            for (int len : lens) {
                                const ll fs = t0 + r;
                                if (fs < 0 || fs + len >= TOP) continue;
                                one(p, ti, lmax, fs, len, 40, Read1{});
                            }
                }
                // ---- the fetch window at every off-by-one around start, midpoint and end; the filters at their
                //      thresholds; read1 columns that agree and disagree with the fragment's own span
                const Call p = call_for(W, 120, W == 1000 ? 1001 : 180, 30);
                const int lmax = std::min(p.max_len, LONGEST);
                std::vector<int> rs;
                for (int r = -2300; r <= T + 200; r += 61) rs.push_back(r);
                for (int c : {-2047 - p.hl, -p.hl - 1, -1, 0, p.hr, len_t - 1, len_t + p.hr, T, T + p.hr})
                    for (int k = -2; k <= 2; ++k) rs.push_back(c + k);
                for (int r : rs)
                    for (int len : lens) {
                        const ll fs = t0 + r, fe = fs + len, mid = (fs + fe) >> 1;
                        if (fs < 0 || fe >= TOP) continue;
                        const ll pts[3] = {fs, mid, fe};
                        for (ll pa : pts)
                            for (int da = -1; da <= 1; ++da)
                                for (ll pb : pts)
                                    for (int db = -1; db <= 1; ++db) {
                                        const Tile ti{t0, pa + da, pb + db, len_t};
                                        one(p, ti, lmax, fs, len, 30, Read1{});
                                        one(p, ti, lmax, fs, len, 29, Read1{});
                                        // read1 inside the fragment (the contig's promise holds), at either end
                                        one(p, ti, lmax, fs, len, 31, Read1{true, true, fs, std::min(fe, fs + 50)});
                                        one(p, ti, lmax, fs, len, 31, Read1{true, true, std::max(fs, fe - 50), fe});
                                        // a contig without the promise: read1 decides everywhere
                                        one(p, ti, lmax, fs, len, 31, Read1{true, false, fs - 70, fs - 20});
                                        one(p, ti, lmax, fs, len, 31, Read1{true, false, fe + 3, fe + 60});
                                    }
                        // interior / whole-contig windows with read1 columns
                        for (const Tile& ti : {Tile{t0, 0, TOP, len_t}, Tile{t0, t0 - p.hl - 2 - lmax, t0 + len_t + p.hr + lmax, len_t}}) {
                            one(p, ti, lmax, fs, len, 60, Read1{true, true, fs, std::min(fe, fs + 50)});
                            one(p, ti, lmax, fs, len, 60, Read1{true, false, fs - 70, fs - 20});
                            one(p, ti, lmax, fs, len, 60, Read1{true, false, -5, 0});
                        }
                    }
            }
        }
    }
    // the clamped filters (wps_params): thresholds at their ends, mapq 0 .. 255
    for (int mq : {0, 1, 31, 255, 256})
        for (int q : {0, 1, 30, 31, 32, 254, 255})
            for (int mn : {0, 1, 2046, 1 << 30})
                for (int mx : {0, 1, 2046, 1 << 28})
                    for (int len : {0, 1, 2, 2045, 2046}) {
                        const Call p = call_for(120, mn, mx, mq);
                        one(p, Tile{4096, 0, TOP, T}, std::min(mx, LONGEST), 5000, len, q, Read1{});
                    }
    printf("%lld cases, %lld accepted, %lld in interior tiles\n", cases, accepted, interior_cases);
    if (!accepted || !interior_cases) { printf("the sweep met no accepted fragment or no interior tile\n"); ++bad; }
    printf("%lld failures\n", bad);
    return bad ? 1 : 0;
}
