// The packed (length, mapq) word of a fragment, the start column as 1-byte deltas, and the rule that decides which calls
// may read them (host code, plain C++: tools/check_packed_rule.cpp and tools/check_delta_columns.cpp exercise it without
// a GPU).
#pragma once

#include <stdint.h>

namespace ftk {

// lq = len << kLqBits | min(mapq, kLqMapqSat), 16 bits; the split is 11 / 5.  MAPQ is only ever compared with a
// threshold, and the thresholds in use are 30 and below (the reference's default quality_threshold is 30; aligners stop
// at 42 or 60, so a cut above 31 is rare): five bits keep every comparison with a threshold <= 31 exact.  Eleven bits
// hold lengths up to 2046 (2047 is the saturation value, never met in a contig whose column is in use): paired-end
// inserts reach 1000-2000 bp with the usual aligner limits (bwa's proper-pair bound, bowtie2 -X), and under a 10 / 6
// split (1022) ONE such fragment would cost its contig the column; a 1001-bin length histogram fits either way.
constexpr int kLqBits = 5;
constexpr int kLqMapqSat = (1 << kLqBits) - 1;        // 31: saturated mapq
constexpr int kLqLenSat = (1 << (16 - kLqBits)) - 1;  // 2047: saturated length
constexpr int kLqLenMax = kLqLenSat - 1;              // 2046: longest fragment of a contig that keeps the column

// The start column as 1-byte deltas (ContigView::ds, ContigView::gbase), read by the same kernels INSTEAD of the 4-byte
// starts.  Fragments are sorted by start, so inside a group of kDsGroup = 64 consecutive fragments
//   ds[i]    = (uint8_t)(start[i] - start[i - 1]), and 0 for a group's first fragment (i % 64 == 0);
//   gbase[g] = start[64 g], with bit 31 (kGbaseWide; coordinates are below 2^30) set when a delta INSIDE the group
//              exceeds 255.  The gap in front of a group's first fragment is no delta of the group.
//   start[i] = gbase[g] + ds[64 g + 1] + ... + ds[i] in a group without the bit; a group with it is read from the
//              wide column, which stays resident.
// Both columns cover whole groups: the fragments behind the contig's last one sit at kDsPadCoord like the padding of the
// wide columns (so the group that holds fragment n, when n is no multiple of 64, carries the bit).
constexpr int kDsGroup = 64;
constexpr uint32_t kGbaseWide = 0x80000000u;
constexpr int32_t kDsPadCoord = 1 << 30;

// the two columns of start[0, n) over n_groups groups (n_groups * 64 >= n)
inline void ds_encode(const int32_t* start, long long n, long long n_groups, uint8_t* ds, int32_t* gbase) {
    for (long long g = 0; g < n_groups; ++g) {
        bool wide = false;
        for (long long i = g * kDsGroup; i < (g + 1) * kDsGroup; ++i) {
            const int32_t s = i < n ? start[i] : kDsPadCoord, prev = i == 0 ? s : i - 1 < n ? start[i - 1] : kDsPadCoord;
            const uint32_t d = i % kDsGroup ? (uint32_t)s - (uint32_t)prev : 0u;
            ds[i] = (uint8_t)d;
            wide |= d > 255u;
            if (i % kDsGroup == 0) gbase[g] = s;
        }
        if (wide) gbase[g] = (int32_t)((uint32_t)gbase[g] | kGbaseWide);
    }
}

// start[i] as the kernels rebuild it (the device form: an in-lane prefix over four deltas, a scan over the 16 lanes of a
// group, the group's base)
inline int32_t ds_decode(const int32_t* start, const uint8_t* ds, const int32_t* gbase, long long i) {
    const long long g = i / kDsGroup;
    if ((uint32_t)gbase[g] & kGbaseWide) return start[i];
    int32_t s = gbase[g];
    for (long long k = g * kDsGroup + 1; k <= i; ++k) s += ds[k];
    return s;
}

// Every comparison one call makes with a fragment's mapq or length.  A part that does not run has run = false.
struct PackedCall {
    bool has_lq = false;  // the contig holds the column (ContigView::lq)
    // the FAST feature blocks: one mapq cut; coverage / histogram length bounds; the histogram's bins
    bool feat = false;
    int feat_q = 0;
    long long feat_min = 0, feat_max = 1 << 30;
    bool hist = false;
    long long len_lo = 0, n_bins = 0;
    // the WPS tiles
    bool wps = false;
    int wps_q = 0;
    long long wps_min = 0, wps_max = 1 << 30;
};

// May this call read lq instead of end and mapq?  The answer depends on the call alone (and on the column being there),
// so the same call takes the same path on every contig that has the column.  What the kernels do with the word:
//   end  = start + (lq >> kLqBits)   exact for every fragment of a contig that has the column (len <= kLqLenMax);
//   mapq = lq & kLqMapqSat           min(mapq, 31).
// * mapq is only compared as `mapq < cut`.  For cut <= 31: min(mapq, 31) < cut <=> mapq < cut.  A cut of 32 or more
//   would reject every saturated fragment: such a call keeps the wide columns.
// * lengths are exact, so every length test is.  The rule still asks that no test could tell a saturated word (2047)
//   from the length it stands for, which keeps it right by construction and not by what the loader let through:
//     lower bounds (len >= lo) hold for lo <= 2047: a saturated word and its true length are both >= lo;
//     upper bounds (len <= hi) hold for hi < 2047, or for hi >= 2^30, which no length reaches (coordinates are
//     below 2^30): "unbounded";
//     histogram bins [len_lo, len_lo + n_bins) need len_lo + n_bins <= 2047: a saturated word lands in the overflow
//     bin like its true length;
//     DELFI's constants (100, 150, 151, 220) lie below 2047.
inline bool packed_call_ok(const PackedCall& c) {
    if (!c.has_lq) return false;
    auto lower_ok = [](long long lo) { return lo <= kLqLenSat; };
    auto upper_ok = [](long long hi) { return hi < kLqLenSat || hi >= (1LL << 30); };
    if (c.feat) {
        if (c.feat_q > kLqMapqSat) return false;
        if (!lower_ok(c.feat_min) || !upper_ok(c.feat_max)) return false;
        if (c.hist && c.len_lo + c.n_bins > kLqLenSat) return false;
    }
    if (c.wps) {
        if (c.wps_q > kLqMapqSat) return false;
        if (!lower_ok(c.wps_min) || !upper_ok(c.wps_max)) return false;
    }
    return c.feat || c.wps;
}

}  // namespace ftk
