// Stand-alone check (plain C++, no GPU) of the start column as 1-byte deltas (ds_encode / ds_decode,
// finaletoolkit_amd/csrc/ftk_packed.h): decode(encode(starts)) == starts, the bit on exactly the groups that hold a delta
// above 255 behind their first fragment, and the device's order of sums (a prefix over a lane's four deltas, a scan over
// the 16 lanes of a group, the base) against the rule.
//   c++ -std=c++17 -I finaletoolkit_amd/csrc tools/check_delta_columns.cpp -o check_delta_columns && ./check_delta_columns
#include <cstdio>
#include <vector>

#include "ftk_packed.h"

using namespace ftk;

static long long bad = 0;

// four starts of a lane the way the kernels rebuild them (starts_from_deltas, ftk_device.h)
static void lane_starts(const uint8_t* ds, int32_t gb, long long g, int lane, int32_t out[4]) {
    int32_t before = gb;
    for (int l = 0; l < lane; ++l)
        for (int j = 0; j < 4; ++j) before += ds[g * kDsGroup + 4 * l + j];
    int32_t p = 0;
    for (int j = 0; j < 4; ++j) {
        p += ds[g * kDsGroup + 4 * lane + j];
        out[j] = before + p;
    }
}

static void check(const char* what, const std::vector<int32_t>& start) {
    const long long n = (long long)start.size();
    const long long n_pad = (n + 3) / 4 * 4 + 4, n_groups = n_pad / kDsGroup + 1;  // the loader's padding
    std::vector<uint8_t> ds(n_groups * kDsGroup, 0xAB);
    std::vector<int32_t> gbase(n_groups, -7);
    ds_encode(start.data(), n, n_groups, ds.data(), gbase.data());
    for (long long g = 0; g < n_groups; ++g) {
        bool wide = false;
        for (long long i = g * kDsGroup + 1; i < (g + 1) * kDsGroup; ++i) {
            const long long a = i < n ? start[i] : kDsPadCoord, b = i - 1 < n ? start[i - 1] : kDsPadCoord;
            wide |= a - b > 255;
        }
        const bool flag = ((uint32_t)gbase[g] & kGbaseWide) != 0;
        const int32_t first = g * kDsGroup < n ? start[g * kDsGroup] : kDsPadCoord;
        if (flag != wide) { printf("%s: group %lld flag %d, want %d\n", what, g, flag, wide); ++bad; }
        if ((int32_t)((uint32_t)gbase[g] & ~kGbaseWide) != first) { printf("%s: group %lld base\n", what, g); ++bad; }
        if (ds[g * kDsGroup] != 0) { printf("%s: group %lld first delta %d\n", what, g, ds[g * kDsGroup]); ++bad; }
        if (!flag)
            for (int lane = 0; lane < 16; ++lane) {
                int32_t s[4];
                lane_starts(ds.data(), gbase[g], g, lane, s);
                for (int j = 0; j < 4; ++j) {
                    const long long i = g * kDsGroup + 4 * lane + j;
                    if (s[j] != (i < n ? start[i] : kDsPadCoord)) { printf("%s: lane form, fragment %lld\n", what, i); ++bad; }
                }
            }
    }
    for (long long i = 0; i < n; ++i)
        if (ds_decode(start.data(), ds.data(), gbase.data(), i) != start[i]) { printf("%s: fragment %lld\n", what, i); ++bad; }
    // the group that holds fragment n - 1 lies inside the columns (a block reads it whole)
    if (n > 0 && (n - 1) / kDsGroup >= n_groups) { printf("%s: last group outside\n", what); ++bad; }
}

int main() {
    static_assert(kDsGroup == 64 && kGbaseWide == 0x80000000u && kDsPadCoord == (1 << 30), "groups of 64, bit 31");
    const int32_t top = (1 << 30) - 1;
    for (int n : {0, 1, 63, 64, 65, 129}) {
        std::vector<int32_t> s(n);
        for (int i = 0; i < n; ++i) s[i] = 1000 + 10 * i;
        check("steps of 10", s);
        for (int i = 0; i < n; ++i) s[i] = 5;
        check("one start", s);
        for (int i = 0; i < n; ++i) s[i] = top - 255 * (n - 1 - i);
        check("steps of 255 up to 2^30 - 1", s);
        for (int i = 0; i < n; ++i) s[i] = top;
        check("all at 2^30 - 1", s);
    }
    {  // a run of equal starts longer than a group, across two boundaries
        std::vector<int32_t> s;
        for (int i = 0; i < 40; ++i) s.push_back(100 + i);
        for (int i = 0; i < 150; ++i) s.push_back(500);
        for (int i = 0; i < 30; ++i) s.push_back(501 + 3 * i);
        check("equal run", s);
    }
    // a delta of 255 / 256 at every place of a group, its first fragment included (there it never sets the bit)
    for (int gap : {255, 256, 100000})
        for (int at : {1, 2, 3, 4, 62, 63, 64, 65, 66, 127, 128, 129, 191, 192})
            for (int32_t base : {0, 12345, top - 100000 - 2 * 300}) {
                std::vector<int32_t> s(300);
                int32_t v = base;
                for (int i = 0; i < 300; ++i) {
                    v += i == at ? gap : (i ? 2 : 0);
                    s[i] = v;
                }
                check("one gap", s);
                const long long n_groups = (300 + 3) / 4 * 4 / kDsGroup + 1 + 1;
                std::vector<uint8_t> ds(n_groups * kDsGroup);
                std::vector<int32_t> gb(n_groups);
                ds_encode(s.data(), 300, n_groups, ds.data(), gb.data());
                for (int g = 0; g < 4; ++g) {
                    const bool want = gap > 255 && at / kDsGroup == g && at % kDsGroup != 0;
                    if ((((uint32_t)gb[g] & kGbaseWide) != 0) != want) { printf("gap %d at %d: group %d\n", gap, at, g); ++bad; }
                }
            }
    printf("%lld failures\n", bad);
    return bad ? 1 : 0;
}
