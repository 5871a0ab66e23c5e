// The interior of a window's candidate range, and what a FAST feature block may derive from its length histogram
// (plain C++: the feature blocks in ftk_kernels.hip and tools/check_feat_interior.cpp, which holds it against a naive
// per-fragment statement of the outputs without a GPU, read this one text).
#pragma once

#include <stdint.h>

#include "ftk_packed.h"

#ifndef FTK_HD
#if defined(__HIPCC__)
#define FTK_HD __host__ __device__ __forceinline__
#else
#define FTK_HD inline
#endif
#endif

namespace ftk {

constexpr int kFeatIndexShift = 9;  // the position index's bin, 512 bp (kBinShift, ftk_internal.h)

// ---- the FAST tabix predicate (fast_group, ftk_kernels.hip), restated ----------------------------------------------
// A block clamps its window [ws_raw, we_raw) to  ws = clamp(ws_raw, -1, 2^30),  we = clamp(we_raw, 0, 2^30)  and accepts
// a fragment [fs, fe) with mapq q (0 <= fs <= fe < 2^30 for every resident fragment) exactly when none of
//     q - ch_q,   m2 - ws2,   we2 - m2,   fe + wsm1
// is negative, with m2 = fs + fe, ws2 = 2 max(ws, 0), we2 = 2 (we - 1) + 1, wsm1 = -1 - ws: the midpoint floor(m2 / 2)
// lies in [max(ws, 0), we - 1] and the fragment ends behind ws.
//
// ---- the interior ---------------------------------------------------------------------------------------------------
// bin_idx[k] is the first fragment whose start is >= 512 k (fragments are sorted by start), lmax is no shorter than the
// contig's longest fragment.  With w0 = clamp(ws_raw, 0, 2^30) (= max(ws, 0)) and we as above:
//     I0 = bin_idx[ceil((w0 + 1) / 512)]                        rounded UP to a multiple of kDsGroup,
//     I1 = bin_idx[floor((we - lmax) / 512)] if we - lmax > 0   rounded DOWN to one; else there is no interior,
// both inside the block's candidate range [lo, hi).  CLAIM: a fragment i in [I0, I1) passes the predicate exactly when
// q >= ch_q.  Proof, term by term, for such a fragment:
//   * i >= I0 >= bin_idx[ceil((w0 + 1) / 512)], so fs >= 512 ceil((w0 + 1) / 512) >= w0 + 1 > w0 >= ws.
//     m2 - ws2:  fe >= fs (lengths are >= 0, a fragment of length zero included), so m2 >= 2 fs >= 2 w0 + 2 > ws2.
//     fe + wsm1: fe >= fs >= w0 + 1 >= ws + 1, so fe - 1 - ws >= 0.  (ws_raw < -1: ws = -1 and fe >= 1 does.)
//   * i < I1 <= bin_idx[floor((we - lmax) / 512)], so fs < 512 floor((we - lmax) / 512) <= we - lmax, fs <= we - lmax - 1.
//     we2 - m2:  fe = fs + len <= fs + lmax <= we - 1 and fs <= we - 1 (lmax >= 0), so m2 <= 2 we - 2 < we2.
//   * no term overflows: 0 <= fs, fe < 2^30 gives 0 <= m2 < 2^31 - 1; ws2 <= 2^31 only for w0 = 2^30, where
//     ceil((w0 + 1) / 512) lies behind every start and I0 = n: no interior.  we2 <= 2^31 - 1.
//   * a window clamped at 2^30 only loses interior (the clamped we is the smaller one); one clamped at 0 has w0 = 0 and
//     the proof reads the same.  we_raw <= 0 or we_raw < ws_raw: the candidate range is empty (window_candidates), and
//     the clamp into [lo, hi) leaves no interior.
//   * the padding fragments behind the contig sit at 2^30 with index >= n; hi <= n and I1 <= hi, so none is interior.
//     (They are edge fragments at most, and fail the window test as before.)
// So an interior fragment needs neither its start nor its end: its packed word gives the mapq test and the length bin.
// The other candidates - the EDGE, [lo, I0) and [I1, hi), whole groups of the delta columns since lo, I0 and I1 are
// multiples of kDsGroup - take the window test as before.
struct FeatInterior {
    int i0, i1;  // [i0, i1); i0 == i1 == hi when empty, so that the edge is always [lo, i0) and [i1, hi)
};

FTK_HD int feat_index_first(const int32_t* bin_idx, int n_bins, int n, long long k) {
    return k >= n_bins ? n : bin_idx[k];
}

// lo, hi: the block's candidate range, lo a multiple of kDsGroup unless the range is empty (feat_fast_body).
FTK_HD FeatInterior feat_interior(const int32_t* bin_idx, int n_bins, int n, int ws_raw, int we_raw, int lmax, int lo,
                                  int hi) {
    const int top = 1 << 30;
    const int w0 = ws_raw < 0 ? 0 : ws_raw > top ? top : ws_raw;
    const int we = we_raw < 0 ? 0 : we_raw > top ? top : we_raw;
    FeatInterior r;
    r.i0 = r.i1 = hi;
    const long long a1 = (long long)we - (lmax < 0 ? 0 : lmax);
    if (a1 <= 0 || hi <= lo) return r;
    const long long k0 = ((long long)w0 + 1 + ((1 << kFeatIndexShift) - 1)) >> kFeatIndexShift;
    long long i0 = feat_index_first(bin_idx, n_bins, n, k0);
    long long i1 = feat_index_first(bin_idx, n_bins, n, a1 >> kFeatIndexShift);
    i0 = (i0 + kDsGroup - 1) & ~(long long)(kDsGroup - 1);
    if (i1 > hi) i1 = hi;
    i1 &= ~(long long)(kDsGroup - 1);
    if (i0 < lo) i0 = lo;
    if (i0 >= i1) return r;
    r.i0 = (int)i0;
    r.i1 = (int)i1;
    return r;
}

// ---- an interior fragment ------------------------------------------------------------------------------------------
// word: its packed (length, mapq) word; -> the histogram bin (n_bins: the overflow bin) and what to add there (1 when
// the fragment passes, else 0)
FTK_HD unsigned feat_interior_bin(unsigned word, int ch_q, int len_lo, int n_bins, unsigned& add) {
    const int q = (int)(word & (unsigned)kLqMapqSat), len = (int)(word >> kLqBits);
    add = ((unsigned)(q - ch_q) >> 31) ^ 1u;
    const unsigned b = (unsigned)(len - len_lo);
    return b < (unsigned)n_bins ? b : (unsigned)n_bins;
}

// ---- the counts from the histogram ----------------------------------------------------------------------------------
// DELFI's length classes (frag/_delfi.py:443-472): short 100 .. 150, long 151 .. 220.
constexpr int kDelfiShortLo = 100, kDelfiShortHi = 150, kDelfiLongHi = 220;

// Every comparison of one launch that bears on the rule.
struct FeatCountsCall {
    bool hist = false;     // the length histogram is requested
    long long len_lo = 0, n_bins = 0;
    bool fast_ok = false;  // feat_fast_ok: midpoint policy, no length bounds on coverage / histogram, ONE mapq cut
    bool packed = false;   // the launch reads the packed columns
    bool bam = false;      // read1 fetch semantics
};

// May the blocks of this launch derive coverage and the DELFI counts from the window's histogram?  Every passing
// fragment of the window lands in one bin (its length's, or the overflow bin), so coverage is the sum of all bins;
// with one mapq cut for coverage and DELFI, a DELFI fragment of a window without blacklist entries and out of reach of
// the gap intervals is a passing fragment with 100 <= len <= 220: the bins of those lengths must all exist.
inline bool feat_counts_from_hist(const FeatCountsCall& c) {
    return c.hist && c.fast_ok && c.packed && !c.bam && c.len_lo <= kDelfiShortLo && c.len_lo + c.n_bins > kDelfiLongHi;
}

// What bin b (length len_lo + b) of the histogram adds to the three counts; the overflow bin adds to coverage alone.
FTK_HD void feat_counts_add(int len_lo, int b, unsigned v, unsigned& cov, unsigned& sh, unsigned& lg) {
    const int len = len_lo + b;
    cov += v;
    sh += ((unsigned)(len - kDelfiShortLo) <= (unsigned)(kDelfiShortHi - kDelfiShortLo)) ? v : 0u;
    lg += ((unsigned)(len - kDelfiShortHi - 1) <= (unsigned)(kDelfiLongHi - kDelfiShortHi - 1)) ? v : 0u;
}

}  // namespace ftk
