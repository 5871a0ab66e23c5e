// Stand-alone check (plain C++, no GPU) of the feature blocks' interior rule and of the counts taken from the length
// histogram (finaletoolkit_amd/csrc/ftk_feat_interior.h).  Small hand-made contigs, every window start of a range that
// crosses two multiples of 512 with a dozen window lengths each; per window
//   * the NAIVE statement: every fragment of the contig against the window in 64-bit - mapq cut, the tabix overlap
//     (fe > ws, fs < we), the midpoint in [ws, we) - gives the histogram, coverage, DELFI short (100 .. 150) and long
//     (151 .. 220);
//   * the BLOCK form: the candidate range of the position index as a packed feature block takes it, feat_interior, the
//     edge through the 32-bit sign test, the interior through feat_interior_bin (the packed word alone), the three counts
//     through feat_counts_add;
//   * the claim itself: every interior fragment passes the window test, the interior's bounds are multiples of kDsGroup
//     inside the range.
// The first line printed counts the cases met (below_cut / at_cut / above_cut: fragments that start at we - lmax - 1, we - lmax,
// we - lmax + 1; short_windows: shorter than lmax + 512), so that a test can see the ones it asks for were there.
//   c++ -std=c++17 -I finaletoolkit_amd/csrc tools/check_feat_interior.cpp -o check_feat_interior && ./check_feat_interior
#include <climits>
#include <cstdio>
#include <vector>

#include "ftk_feat_interior.h"

using namespace ftk;

static long long bad = 0;
static long long n_windows = 0, n_with_interior = 0, n_empty_interior = 0, n_interior_frags = 0, n_edge_frags = 0;
static long long n_zero_len_at_ws = 0, n_at_cut[3] = {0, 0, 0}, n_short_windows = 0, n_partial_last = 0, n_ws0 = 0, n_aligned = 0;
static long long n_empty_windows = 0, n_clamped = 0;

constexpr int kQ = 30, kLenLo = 0, kBins = 1001;

struct Contig {
    const char* name;
    std::vector<int32_t> start, len, mapq;
    std::vector<int32_t> bin_idx;
    int n_bins = 0, lmax = 0;
    void finish() {
        const int n = (int)start.size();
        lmax = 0;
        int max_start = 0;
        for (int i = 0; i < n; ++i) {
            if (len[i] > lmax) lmax = len[i];
            if (start[i] > max_start) max_start = start[i];
            if (i && start[i] < start[i - 1]) { printf("%s: unsorted\n", name); ++bad; }
        }
        n_bins = (max_start >> kFeatIndexShift) + 1;
        bin_idx.assign((size_t)n_bins + 1, n);
        int i = 0;
        for (int k = 0; k < n_bins; ++k) {
            while (i < n && start[i] < ((long long)k << kFeatIndexShift)) ++i;
            bin_idx[k] = i;
        }
    }
};

// the candidate range of a packed feature block (window_candidates and the group rounding of feat_fast_body)
static void candidates(const Contig& c, int ws, int we, int lmax, int& lo, int& hi) {
    const int n = (int)c.start.size();
    const long long ql = (long long)ws - lmax;
    if (ws == INT32_MIN || ql <= 0) lo = 0;
    else { const long long k = ql >> kFeatIndexShift; lo = k >= c.n_bins ? n : c.bin_idx[k]; }
    if (we == INT32_MAX) hi = n;
    else if (we <= 0) hi = 0;
    else { const long long k = (long long)we >> kFeatIndexShift; hi = k >= c.n_bins ? n : c.bin_idx[k + 1]; }
    lo &= ~3;
    if (hi < lo || we < ws) hi = lo;
    if (hi > lo) lo &= ~(kDsGroup - 1);
}

// the FAST tabix predicate as the kernel writes it (fast_group): sign clear = accepted.  Real fragments only.
static int fast_x(int ws_raw, int we_raw, int fs, int fe, int q) {
    const int top = 1 << 30;
    const int ws = ws_raw < -1 ? -1 : ws_raw > top ? top : ws_raw;
    const int we1 = (we_raw < 0 ? 0 : we_raw > top ? top : we_raw) - 1;
    const int ws2 = (int)(2u * (unsigned)(ws < 0 ? 0 : ws)), we2 = 2 * we1 + 1, wsm1 = -1 - ws;
    const int m2 = fs + fe;
    return (q - kQ) | (int)((unsigned)m2 - (unsigned)ws2) | (we2 - m2) | (fe + wsm1);
}

static void window(const Contig& c, int ws, int we) {
    const int n = (int)c.start.size();
    ++n_windows;
    // ---- naive ----
    std::vector<unsigned> want(kBins + 1, 0u);
    long long cov = 0, sh = 0, lg = 0;
    for (int i = 0; i < n; ++i) {
        const long long fs = c.start[i], fe = fs + c.len[i], mid = (fs + fe) >> 1;
        if (c.mapq[i] < kQ || !(fe > ws && fs < we) || !(mid >= ws && mid < we)) continue;
        ++cov;
        const long long L = c.len[i];
        ++want[L - kLenLo >= 0 && L - kLenLo < kBins ? L - kLenLo : kBins];
        if (L >= 100 && L <= 150) ++sh;
        if (L >= 151 && L <= 220) ++lg;
        if (L == 0 && fs == ws) { printf("%s [%d, %d): a zero-length fragment at ws passes\n", c.name, ws, we); ++bad; }
    }
    // ---- block form ----
    int lo, hi;
    candidates(c, ws, we, c.lmax, lo, hi);
    const FeatInterior in = feat_interior(c.bin_idx.data(), c.n_bins, n, ws, we, c.lmax, lo, hi);
    if (in.i0 > in.i1 || in.i0 < lo || in.i1 > hi || (in.i0 < in.i1 && ((in.i0 | in.i1) % kDsGroup)) ||
        (in.i0 == in.i1 && in.i0 != hi)) {
        printf("%s [%d, %d): interior [%d, %d) of [%d, %d)\n", c.name, ws, we, in.i0, in.i1, lo, hi);
        ++bad;
        return;
    }
    (in.i0 < in.i1 ? n_with_interior : n_empty_interior)++;
    std::vector<unsigned> got(kBins + 1, 0u);
    const int hi4 = lo + ((hi - lo + 3) & ~3);  // the block's groups of four reach past hi
    for (int i = lo; i < hi4 && i < n; ++i) {
        const long long at = (long long)c.start[i] - ((long long)we - c.lmax);
        if (at >= -1 && at <= 1) ++n_at_cut[at + 1];
        if (i >= in.i0 && i < in.i1) {
            const unsigned word = (unsigned)c.len[i] << kLqBits | (unsigned)(c.mapq[i] < kLqMapqSat ? c.mapq[i] : kLqMapqSat);
            unsigned add;
            const unsigned b = feat_interior_bin(word, kQ, kLenLo, kBins, add);
            got[b] += add;
            ++n_interior_frags;
            // the claim: but for the mapq, the window test cannot fail
            if (fast_x(ws, we, c.start[i], c.start[i] + c.len[i], 60) < 0) {
                printf("%s [%d, %d): interior fragment %d fails the window test\n", c.name, ws, we, i);
                ++bad;
            }
            const long long d = (long long)c.start[i] - ((long long)we - c.lmax);
            if (d >= 0) { printf("%s [%d, %d): interior fragment %d at we - lmax + %lld\n", c.name, ws, we, i, d); ++bad; }
        } else {
            const int fs = c.start[i], fe = fs + c.len[i];
            if (fast_x(ws, we, fs, fe, c.mapq[i]) >= 0) {
                const unsigned b = (unsigned)(c.len[i] - kLenLo);
                ++got[b < (unsigned)kBins ? b : (unsigned)kBins];
            }
            ++n_edge_frags;
            if (c.len[i] == 0 && fs == ws) ++n_zero_len_at_ws;
        }
    }
    unsigned gc = got[kBins], gs = 0, gl = 0;
    for (int b = 0; b < kBins; ++b) feat_counts_add(kLenLo, b, got[b], gc, gs, gl);
    if (got != want || gc != cov || gs != sh || gl != lg) {
        printf("%s [%d, %d): block form %u %u %u, naive %lld %lld %lld%s\n", c.name, ws, we, gc, gs, gl, cov, sh, lg,
               got != want ? ", histograms differ" : "");
        ++bad;
    }
    if ((long long)we - ws < (long long)c.lmax + 512) { ++n_short_windows; }
    if (ws == 0) ++n_ws0;
    if (ws >= 0 && ws % 512 == 0 && we % 512 == 0) ++n_aligned;
    if (n && we > c.start[n - 1] + c.len[n - 1]) ++n_partial_last;
    if (hi == lo) ++n_empty_windows;
    if (ws < -1 || we > (1 << 30)) ++n_clamped;
}

// fragments at `per` per position over [base, base + span), lengths cycling through `lens`, mapqs around the cut
static Contig dense(const char* name, int base, int span, int num, int den, const std::vector<int>& lens) {
    Contig c;
    c.name = name;
    int k = 0;
    static const int mq[] = {60, 30, 29, 31, 0, 42, 30, 60, 37};
    for (int p = 0; p < span; ++p)
        for (int r = (p * num) / den; r < ((p + 1) * num) / den; ++r, ++k) {
            c.start.push_back(base + p);
            c.len.push_back(lens[(size_t)k % lens.size()]);
            c.mapq.push_back(mq[k % 9]);
        }
    c.finish();
    return c;
}

static void sweep(const Contig& c, int base, int from, int to) {
    const int end = c.start.empty() ? base : c.start.back() + c.lmax;
    for (int ws = base + from; ws < base + to; ++ws) {
        for (int L : {1, 100, 511, 512, 513, 700, 1024, 1100, 1536, 2000})
            window(c, ws, ws + L);
        window(c, ws, end);        // up to the last fragment's end
        window(c, ws, end + 777);  // the last, partial window: it ends behind every fragment
    }
    for (int we : {-5, 0, 1, 511, 512, 513, 1024, 1536, INT32_MAX}) {
        const long long w = we == INT32_MAX ? we : (long long)base + we;
        window(c, 0, (int)w);
        window(c, -1, (int)w);
        window(c, -1000, (int)w);
        window(c, INT32_MIN, (int)w);
    }
    window(c, base + 900, base + 800);  // we < ws
    window(c, base + 512, base + 512);
}

int main() {
    static_assert(kDsGroup == 64 && kFeatIndexShift == 9, "groups of 64, bins of 512");
    const std::vector<int> mixed = {0, 167, 100, 150, 99, 151, 220, 221, 1, 145, 230, 166, 0, 180};
    {
        const Contig c = dense("dense, lmax 230", 0, 2600, 5, 4, mixed);
        sweep(c, 0, -2, 1100);
    }
    {
        const Contig c = dense("every length zero", 0, 2600, 1, 1, {0});
        if (c.lmax != 0) ++bad;
        sweep(c, 0, -2, 1100);
    }
    {
        const Contig c = dense("lmax 600", 0, 2600, 1, 1, {600, 120, 0, 167, 200, 333});
        sweep(c, 0, -2, 1100);
    }
    {
        const Contig c = dense("sparse", 0, 2600, 1, 9, mixed);
        sweep(c, 0, -2, 1100);
    }
    {
        const Contig c = dense("fifty fragments", 700, 50, 1, 1, mixed);
        sweep(c, 0, 0, 1100);
    }
    {
        Contig c;
        c.name = "no fragment";
        c.finish();
        sweep(c, 0, 0, 40);
    }
    {  // the same shapes just below 2^30: the clamps and the widest sums
        const int base = (1 << 30) - 3072;
        const Contig c = dense("top", base, 2600, 5, 4, mixed);
        sweep(c, base, -2, 600);
        for (int ws : {base, base + 100, base + 512})
            for (int we : {1 << 30, (1 << 30) + 1, INT32_MAX - 1, INT32_MAX}) window(c, ws, we);
    }
    printf("windows=%lld interior=%lld no_interior=%lld interior_fragments=%lld edge_fragments=%lld below_cut=%lld at_cut=%lld "
           "above_cut=%lld zero_length_at_ws=%lld short_windows=%lld ws_zero=%lld aligned=%lld partial_last=%lld empty_ranges=%lld "
           "clamped=%lld\n",
           n_windows, n_with_interior, n_empty_interior, n_interior_frags, n_edge_frags, n_at_cut[0], n_at_cut[1], n_at_cut[2],
           n_zero_len_at_ws, n_short_windows, n_ws0, n_aligned, n_partial_last, n_empty_windows, n_clamped);
    printf("%lld failures\n", bad);
    return bad ? 1 : 0;
}
