// Stand-alone check (plain C++, no GPU) of the rule that decides which calls may read the packed (length, mapq) column:
// packed_call_ok (finaletoolkit_amd/csrc/ftk_packed.h) against a brute-force statement of what it must guarantee - that
// no comparison the call makes can tell a word from the fragment it stands for, saturated words included.
//   c++ -std=c++17 -I finaletoolkit_amd/csrc tools/check_packed_rule.cpp -o check_packed_rule && ./check_packed_rule
#include <cstdio>
#include <vector>

#include "ftk_packed.h"

using namespace ftk;

// what the kernels see of a fragment (len, mapq) through its word
static int word_len(long long len) { return (int)(len < kLqLenSat ? len : kLqLenSat); }
static int word_q(int q) { return q < kLqMapqSat ? q : kLqMapqSat; }

// every comparison of the call, on the true values and on the word's: equal for every fragment?
static bool exact(const PackedCall& c, const std::vector<long long>& lens) {
    for (long long len : lens)
        for (int q : {0, 1, 19, 20, 21, 29, 30, 31, 32, 33, 34, 59, 60, 63, 64, 254, 255}) {
            const int wl = word_len(len), wq = word_q(q);
            if (c.feat) {
                if ((q < c.feat_q) != (wq < c.feat_q)) return false;
                if ((len < c.feat_min) != (wl < c.feat_min) || (len > c.feat_max) != (wl > c.feat_max)) return false;
                if (c.hist) {  // bin index, n_bins = overflow
                    auto bin = [&](long long l) { const long long b = l - c.len_lo; return b < 0 || b >= c.n_bins ? c.n_bins : b; };
                    if (bin(len) != bin(wl)) return false;
                }
                for (int k : {100, 150, 151, 220})
                    if ((len < k) != (wl < k)) return false;
            }
            if (c.wps) {
                if ((q < c.wps_q) != (wq < c.wps_q)) return false;
                if ((len < c.wps_min) != (wl < c.wps_min) || (len > c.wps_max) != (wl > c.wps_max)) return false;
            }
        }
    return true;
}

int main() {
    static_assert(kLqBits == 5 && kLqMapqSat == 31 && kLqLenSat == 2047 && kLqLenMax == 2046, "the 11 / 5 split");
    // lengths on both sides of every edge in play, up to the coordinate limit
    std::vector<long long> lens;
    for (long long e : {0LL, 100LL, 120LL, 150LL, 180LL, 220LL, 1000LL, 1047LL, 2047LL, 4096LL, 5000LL, 32768LL, 65536LL, (1LL << 28),
                        (1LL << 30) - 3})
        for (long long l = e > 3 ? e - 3 : 0; l <= e + 3; ++l) lens.push_back(l);
    const int qs[] = {-5, 0, 1, 20, 30, 31, 32, 33, 60, 255, 256};
    const long long los[] = {0, 1, 120, 2046, 2047, 2048, 5000};
    const long long his[] = {0, 180, 1000, 2045, 2046, 2047, 2048, 5000, (1LL << 28), (1LL << 30), 2147483647LL};
    const long long edges[][2] = {{0, 1001}, {0, 2047}, {0, 2048}, {1000, 1047}, {1000, 1048}, {-5, 100}, {2046, 1}, {2047, 1}, {0, 32768}};
    long long n = 0, n_ok = 0, bad = 0;
    PackedCall none;
    none.has_lq = true;
    if (packed_call_ok(none)) { printf("a call with no part must not be packed\n"); ++bad; }
    for (int part = 1; part < 4; ++part)
        for (int q : qs)
            for (long long lo : los)
                for (long long hi : his)
                    for (auto& e : edges)
                        for (int hist = 0; hist < 2; ++hist) {
                            PackedCall c;
                            c.has_lq = true;
                            c.feat = part & 1;
                            c.wps = (part & 2) != 0;
                            c.feat_q = q;
                            c.wps_q = q;
                            c.hist = hist != 0;
                            c.len_lo = e[0];
                            c.n_bins = e[1];
                            c.wps_min = lo;
                            c.wps_max = hi;
                            ++n;
                            const bool ok = packed_call_ok(c);
                            n_ok += ok;
                            if (ok && !exact(c, lens)) {
                                printf("admitted but not exact: part %d q %d lo %lld hi %lld hist %d (%lld, %lld)\n", part, q, lo,
                                       hi, hist, e[0], e[1]);
                                ++bad;
                            }
                            c.has_lq = false;
                            if (packed_call_ok(c)) { printf("packed without a column\n"); ++bad; }
                        }
    // the calls that must stay packed (the benchmark's, the tests') and the ones that must not
    auto call = [](int q, long long lo, long long nb, long long wmin, long long wmax, int wq) {
        PackedCall c;
        c.has_lq = c.feat = c.hist = c.wps = true;
        c.feat_q = q; c.len_lo = lo; c.n_bins = nb; c.wps_min = wmin; c.wps_max = wmax; c.wps_q = wq;
        return packed_call_ok(c);
    };
    struct { bool want, got; } pins[] = {
        {true, call(30, 0, 1001, 120, 180, 30)},    {true, call(31, 1000, 1047, 0, 2046, 31)},
        {false, call(32, 0, 1001, 120, 180, 30)},   {false, call(30, 0, 1001, 120, 180, 32)},
        {false, call(30, 1000, 1048, 120, 180, 30)}, {false, call(30, 0, 1001, 120, 2047, 30)},
        {true, call(30, 0, 1001, 120, 1 << 30, 30)}, {true, call(-1, 0, 1001, 0, 180, -1)},
    };
    for (auto& p : pins)
        if (p.want != p.got) { printf("pinned call: want %d got %d\n", p.want, p.got); ++bad; }
    printf("%lld calls, %lld admitted, %lld failures\n", n, n_ok, bad);
    return bad ? 1 : 0;
}
