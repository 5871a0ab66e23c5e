// The packed (length, mapq) word of a fragment and the rule that decides which calls may read it (host code, plain
// C++: tools/check_packed_rule.cpp exercises it without a GPU).
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
