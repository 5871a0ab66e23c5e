// The write direction on the device: a resident contig's columns -> text rows (a) with what a tabix index needs (b),
// and text -> BGZF members (c).  DESIGN.md section 3.10.
//
// (a)/(b) Two passes over the columns.  Pass 1 works out every row's length from digit counts and reduces a RowAgg per
// workgroup of 1024 rows; one workgroup scans those; pass 2 recomputes the lengths, scans them inside the workgroup and
// writes the bytes.  The RowAgg carries, besides bytes and rows, the bin of the last kept row and the last 16 kb window
// reached so far: a row knows from its prefix alone whether it opens a bin run and which windows it is the first row
// of, so runs and the linear index are written with plain stores, each entry by exactly one row.  Region masks
// (whitelist / blacklist) come in as a bitmap that mask_keep_kernel writes in front of pass 1, with the same tiling.
//
// (c) One LANE per BGZF block: a greedy LZ77 parse (4-byte hash, one candidate, matches verified and extended with
// 4-byte compares), tokens in per-lane global scratch, and per DEFLATE block of at most 8192 tokens the cheaper of the
// fixed code and a dynamic code (lengths from the symbol counts, made complete by a Kraft fill, RFC 1951 3.2.7 header
// with zero-run symbols 17 / 18); a member that would be larger than its stored form is written as a stored block.
// The block compressor is plain C++ (`FTK_HD`), so the same source runs on the host against zlib.  CRC-32 comes from
// ftk_inflate.hip's kernel; member sizes are scanned and the members compacted into one contiguous image.
#include "ftk_fragtext.h"

#include <hip/hip_runtime.h>

#include <cstring>

#include "ftk_internal.h"

#define FTK_HD __host__ __device__ inline

namespace ftk {

// ---------------------------------------------------------------------------------------------------------------
// (a) rows
// ---------------------------------------------------------------------------------------------------------------
FTK_HD int dec_digits(uint32_t x) {  // comparisons against powers of ten
    return 1 + (x >= 10u) + (x >= 100u) + (x >= 1000u) + (x >= 10000u) + (x >= 100000u) + (x >= 1000000u) +
           (x >= 10000000u) + (x >= 100000000u) + (x >= 1000000000u);
}

FTK_HD bool row_kept(int32_t s, int32_t e, int32_t q, const RowParams& p) {
    const int32_t len = e - s;
    return s < kPadCoord && q >= p.mapq_min && (p.min_len < 0 || len >= p.min_len) && (p.max_len < 0 || len <= p.max_len);
}

FTK_HD uint32_t row_bytes(int32_t s, int32_t e, int32_t q, const RowParams& p) {
    const uint32_t coord = (uint32_t)p.name_len + dec_digits((uint32_t)s) + dec_digits((uint32_t)e);
    if (p.layout == kLayoutBed3) return coord + 3;
    return coord + dec_digits((uint32_t)q) + (p.layout == kLayoutBed6 ? 8 : 6);
}

FTK_HD int32_t reg2bin(int32_t beg, int32_t end) {  // SAM spec 5.3, 14-bit minimum shift, 5 levels
    if (end <= beg) end = beg + 1;
    --end;
    if (beg >> 14 == end >> 14) return 4681 + (beg >> 14);
    if (beg >> 17 == end >> 17) return 585 + (beg >> 17);
    if (beg >> 20 == end >> 20) return 73 + (beg >> 20);
    if (beg >> 23 == end >> 23) return 9 + (beg >> 23);
    if (beg >> 26 == end >> 26) return 1 + (beg >> 26);
    return 0;
}

FTK_HD int32_t last_window(int32_t s, int32_t e) { return (e > s ? e - 1 : s) >> 14; }

FTK_HD RowAgg agg_none() { return RowAgg{0ull, 0u, 0u, -1, -1, -1, 0}; }

FTK_HD RowAgg agg_row(int32_t s, int32_t e, int32_t q, const RowParams& p) {
    const int32_t b = reg2bin(s, e);
    return RowAgg{row_bytes(s, e, q, p), 1u, 0u, b, b, last_window(s, e), 0};
}

FTK_HD RowAgg agg_combine(const RowAgg& a, const RowAgg& b) {  // a in front of b
    if (b.first_bin < 0) return a;
    if (a.first_bin < 0) return b;
    return RowAgg{a.bytes + b.bytes, a.rows + b.rows, a.runs + b.runs + (a.last_bin != b.first_bin ? 1u : 0u),
                  a.first_bin, b.last_bin, a.max_win > b.max_win ? a.max_win : b.max_win, 0};
}

FTK_HD uint8_t* put_dec(uint8_t* p, uint32_t x) {
    const int d = dec_digits(x);
    for (int k = d - 1; k >= 0; --k) {
        p[k] = (uint8_t)('0' + x % 10u);
        x /= 10u;
    }
    return p + d;
}

FTK_HD uint8_t* put_row(uint8_t* w, int32_t s, int32_t e, int32_t q, int strand, const RowParams& p) {
    for (int k = 0; k < p.name_len; ++k) w[k] = (uint8_t)p.name[k];
    w += p.name_len;
    *w++ = '\t';
    w = put_dec(w, (uint32_t)s);
    *w++ = '\t';
    w = put_dec(w, (uint32_t)e);
    if (p.layout != kLayoutBed3) {
        *w++ = '\t';
        if (p.layout == kLayoutBed6) {
            *w++ = '.';
            *w++ = '\t';
        }
        w = put_dec(w, (uint32_t)q);
        *w++ = '\t';
        *w++ = strand ? '+' : '-';
    }
    *w++ = '\n';
    return w;
}

namespace {

constexpr int kFmtThreads = 256;
constexpr int kFmtRows = kRowsPerBlock / kFmtThreads;  // 4: the columns are padded to groups of four

// inclusive scan of one RowAgg per thread over the workgroup (Hillis-Steele in LDS; the operator is not commutative)
__device__ RowAgg block_scan_inclusive(RowAgg v, RowAgg* sh /* [2][threads] */, int threads) {
    const int t = threadIdx.x;
    int cur = 0;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < threads; d <<= 1) {
        RowAgg x = sh[cur * threads + t];
        if (t >= d) x = agg_combine(sh[cur * threads + t - d], x);
        sh[(cur ^ 1) * threads + t] = x;
        cur ^= 1;
        __syncthreads();
    }
    return sh[cur * threads + t];
}

// the mask bits of a thread's four rows (i0 is a multiple of four, so they share a word); no bitmap: all four
__device__ uint32_t keep_nibble(const unsigned long long* __restrict__ keep_bits, int64_t n, int64_t i0) {
    if (!keep_bits || i0 >= n) return 15u;
    return (uint32_t)(keep_bits[i0 >> 6] >> (i0 & 63)) & 15u;
}

__device__ RowAgg thread_rows(const int32_t* __restrict__ start, const int32_t* __restrict__ end,
                              const uint8_t* __restrict__ mapq, int64_t n, int64_t i0, const RowParams& p, uint32_t nib) {
    RowAgg a = agg_none();
    for (int k = 0; k < kFmtRows; ++k) {
        const int64_t i = i0 + k;
        if (i >= n) break;
        const int32_t s = start[i], e = end[i], q = mapq[i];
        if (row_kept(s, e, q, p) && ((nib >> k) & 1u)) a = agg_combine(a, agg_row(s, e, q, p));
    }
    return a;
}

__global__ __launch_bounds__(kFmtThreads) void format_pass1_kernel(const int32_t* __restrict__ start,
                                                                    const int32_t* __restrict__ end,
                                                                    const uint8_t* __restrict__ mapq, int64_t n, RowParams p,
                                                                    RowAgg* __restrict__ block_agg,
                                                                    const unsigned long long* __restrict__ keep_bits) {
    __shared__ RowAgg sh[2 * kFmtThreads];
    const int64_t i0 = ((int64_t)blockIdx.x * kFmtThreads + threadIdx.x) * kFmtRows;
    const RowAgg inc =
        block_scan_inclusive(thread_rows(start, end, mapq, n, i0, p, keep_nibble(keep_bits, n, i0)), sh, kFmtThreads);
    if (threadIdx.x == kFmtThreads - 1) block_agg[blockIdx.x] = inc;
}

constexpr int kScanThreads = 512;
__global__ __launch_bounds__(kScanThreads) void format_scan_kernel(const RowAgg* __restrict__ block_agg, int64_t nb,
                                                                    RowAgg* __restrict__ block_prefix, RowAgg* __restrict__ total) {
    __shared__ RowAgg sh[2 * kScanThreads];
    __shared__ RowAgg carry;
    if (threadIdx.x == 0) carry = agg_none();
    __syncthreads();
    for (int64_t base = 0; base < nb; base += kScanThreads) {
        const int64_t b = base + threadIdx.x;
        const RowAgg v = b < nb ? block_agg[b] : agg_none();
        const RowAgg inc = block_scan_inclusive(v, sh, kScanThreads);
        const RowAgg c = carry;
        __syncthreads();  // everybody holds the carry (and its own scan value) before either is overwritten
        sh[threadIdx.x] = inc;  // exclusive = carry + the left neighbour's inclusive value
        __syncthreads();
        if (b < nb) block_prefix[b] = threadIdx.x ? agg_combine(c, sh[threadIdx.x - 1]) : c;
        if (threadIdx.x == kScanThreads - 1) carry = agg_combine(c, inc);
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(kFmtThreads) void format_pass2_kernel(
    const int32_t* __restrict__ start, const int32_t* __restrict__ end, const uint8_t* __restrict__ mapq,
    const uint8_t* __restrict__ strand, int64_t n, RowParams p, const RowAgg* __restrict__ block_prefix,
    uint8_t* __restrict__ text, int32_t* __restrict__ run_bin, uint32_t* __restrict__ run_off, uint32_t* __restrict__ lin,
    int32_t n_lin, const unsigned long long* __restrict__ keep_bits) {
    __shared__ RowAgg sh[2 * kFmtThreads];
    const int64_t i0 = ((int64_t)blockIdx.x * kFmtThreads + threadIdx.x) * kFmtRows;
    const uint32_t nib = keep_nibble(keep_bits, n, i0);
    const RowAgg mine = thread_rows(start, end, mapq, n, i0, p, nib);
    __shared__ RowAgg incl[kFmtThreads];
    incl[threadIdx.x] = block_scan_inclusive(mine, sh, kFmtThreads);
    __syncthreads();
    RowAgg pre = block_prefix[blockIdx.x];
    if (threadIdx.x) pre = agg_combine(pre, incl[threadIdx.x - 1]);
    if (mine.first_bin < 0) return;
    for (int k = 0; k < kFmtRows; ++k) {
        const int64_t i = i0 + k;
        if (i >= n) break;
        const int32_t s = start[i], e = end[i], q = mapq[i];
        if (!row_kept(s, e, q, p) || !((nib >> k) & 1u)) continue;
        const RowAgg row = agg_row(s, e, q, p);
        const uint32_t off = (uint32_t)pre.bytes;
        put_row(text + pre.bytes, s, e, q, strand[i], p);
        // bin runs: this row opens one when no kept row is in front of it or that row's bin differs
        if (pre.first_bin < 0 || pre.last_bin != row.first_bin) {
            const uint32_t r = pre.first_bin < 0 ? 0u : pre.runs + 1u;
            run_bin[r] = row.first_bin;
            run_off[r] = off;
        }
        // linear index: rows are sorted by start, so the windows up to pre.max_win that this row overlaps have an
        // earlier first row (the one that reached pre.max_win starts at or before this row); the rest are this row's
        int32_t w = s >> 14;
        if (w <= pre.max_win) w = pre.max_win + 1;
        for (; w <= row.max_win && w < n_lin; ++w) lin[w] = off;
        pre = agg_combine(pre, row);
    }
}


// ---- region masks: one keep bit per row, written in front of the two passes above ---------------------------------
// Index of the last a[k] <= key in the sorted a[0..m), -1 when there is none.  Branch-free: the trip count depends on
// m alone (uniform over the workgroup) and every step is a load and a select.
template <class Ptr>
__device__ __forceinline__ int last_le(Ptr a, int m, int32_t key) {
    if (m <= 0) return -1;
    int base = 0;
    for (int len = m; len > 1;) {
        const int half = len >> 1;
        base += a[base + half - 1] <= key ? half : 0;
        len -= half;
    }
    return base - 1 + (a[base] <= key ? 1 : 0);
}

// Bits k = 0..3: row k of this thread is in the mask.  On disjoint sorted intervals the only candidate for a row is
// the last interval with start <= key (midpoint: key = test = (s + e) >> 1; any: key = e - 1, test = s - the ends are
// sorted too, so if that interval ends at or before s every earlier one does): in iff its end > test.
template <class Ptr>
__device__ __forceinline__ uint32_t rows_in_slice(Ptr ps, Ptr pe, int m, const int32_t* key, const int32_t* test, uint32_t valid) {
    uint32_t in = 0;
#pragma unroll
    for (int k = 0; k < kFmtRows; ++k) {
        const int j = last_le(ps, m, key[k]);
        in |= (j >= 0 && pe[j < 0 ? 0 : j] > test[k] ? 1u : 0u) << k;
    }
    return in & valid;
}

// One mask against the workgroup's rows.  [lo, hi) = the intervals its rows can touch (block-uniform, from the
// smallest and largest key).  A slice of at most kMaskLdsIntervals entries (counted from lo rounded down to a group
// of four, so that the loads are 16 bytes wide and aligned) is staged in LDS and searched there; a longer one is
// searched where it lies.
__device__ uint32_t rows_in_mask(const int32_t* __restrict__ gs, const int32_t* __restrict__ ge, int lo, int hi,
                                 int32_t* sh_s, int32_t* sh_e, const int32_t* key, const int32_t* test, uint32_t valid) {
    if (hi <= lo) return 0u;
    const int lo4 = lo & ~3;
    const int n4 = (((hi + 3) & ~3) - lo4) >> 2;  // (the arrays are padded to a multiple of four)
    if (n4 * 4 <= kMaskLdsIntervals) {
        const int4* s4 = reinterpret_cast<const int4*>(gs + lo4);
        const int4* e4 = reinterpret_cast<const int4*>(ge + lo4);
        for (int q = threadIdx.x; q < n4; q += kFmtThreads) {
            reinterpret_cast<int4*>(sh_s)[q] = s4[q];
            reinterpret_cast<int4*>(sh_e)[q] = e4[q];
        }
        __syncthreads();
        return rows_in_slice((const int32_t*)sh_s, (const int32_t*)sh_e, hi - lo4, key, test, valid);
    }
    return rows_in_slice(gs + lo, ge + lo, hi - lo, key, test, valid);
}

__global__ __launch_bounds__(kFmtThreads) void mask_keep_kernel(const int32_t* __restrict__ start,
                                                                 const int32_t* __restrict__ end, int64_t n, MaskView m,
                                                                 unsigned long long* __restrict__ keep_bits, int64_t n_words) {
    __shared__ __attribute__((aligned(16))) int32_t sh_iv[4][kMaskLdsIntervals];
    __shared__ int32_t sh_min[kFmtThreads / 64], sh_max[kFmtThreads / 64];
    __shared__ int sh_slice[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t i0 = ((int64_t)blockIdx.x * kFmtThreads + t) * kFmtRows;
    const bool any = m.policy == FTK_POLICY_ANY;
    int32_t key[kFmtRows], test[kFmtRows];
    uint32_t valid = 0;
    int32_t kmin = INT32_MAX, kmax = INT32_MIN;
#pragma unroll
    for (int k = 0; k < kFmtRows; ++k) {
        key[k] = test[k] = 0;
        if (i0 + k < n) {
            const int32_t s = start[i0 + k], e = end[i0 + k];
            const int32_t mid = (s + e) >> 1;  // (both below 2^30: the sum fits)
            key[k] = any ? e - 1 : mid;
            test[k] = any ? s : mid;
            valid |= 1u << k;
            kmin = key[k] < kmin ? key[k] : kmin;
            kmax = key[k] > kmax ? key[k] : kmax;
        }
    }
    // rows are sorted by start, not by key: the workgroup's key range by a reduction
    for (int d = 32; d; d >>= 1) {
        const int32_t a = __shfl_xor(kmin, d), b = __shfl_xor(kmax, d);
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
    }
    if (lane == 0) {
        sh_min[wave] = kmin;
        sh_max[wave] = kmax;
    }
    __syncthreads();
    if (t < 4) {  // wl lo, wl hi, bl lo, bl hi: two binary searches per mask
        for (int w = 0; w < kFmtThreads / 64; ++w) {
            kmin = sh_min[w] < kmin ? sh_min[w] : kmin;
            kmax = sh_max[w] > kmax ? sh_max[w] : kmax;
        }
        const int32_t* gs = t < 2 ? m.wl_start : m.bl_start;
        const int cnt = t < 2 ? m.n_wl : m.n_bl;
        const int j = last_le(gs, cnt, (t & 1) ? kmax : kmin);
        sh_slice[t] = (t & 1) ? j + 1 : (j < 0 ? 0 : j);
    }
    __syncthreads();
    const uint32_t in_wl = m.n_wl < 0 ? valid
                                      : rows_in_mask(m.wl_start, m.wl_end, sh_slice[0], sh_slice[1], sh_iv[0], sh_iv[1], key, test, valid);
    const uint32_t in_bl = m.n_bl <= 0 ? 0u
                                       : rows_in_mask(m.bl_start, m.bl_end, sh_slice[2], sh_slice[3], sh_iv[2], sh_iv[3], key, test, valid);
    // sixteen lanes hold one 64-bit word (4 bits each): OR them together with lane shuffles; the group's first lane
    // stores the word
    unsigned long long word = (unsigned long long)(in_wl & ~in_bl) << (4 * (lane & 15));
    for (int d = 1; d < 16; d <<= 1) word |= __shfl_xor(word, d);
    const int64_t w = (int64_t)blockIdx.x * (kRowsPerBlock / 64) + wave * 4 + (lane >> 4);
    if ((lane & 15) == 0 && w < n_words) keep_bits[w] = word;
}

}  // namespace

size_t format_agg_bytes(int64_t n) {
    const size_t nb = (size_t)((n + kRowsPerBlock - 1) / kRowsPerBlock) + 1;
    return 2 * ((nb * sizeof(RowAgg) + 255) / 256 * 256) + 256;
}

void format_pass1(hipStream_t s, const int32_t* start, const int32_t* end, const uint8_t* mapq, int64_t n,
                  const RowParams& p, RowAgg* block_agg, RowAgg* block_prefix, RowAgg* total,
                  const unsigned long long* keep_bits) {
    const int64_t nb = (n + kRowsPerBlock - 1) / kRowsPerBlock;
    if (nb > 0)
        hipLaunchKernelGGL(format_pass1_kernel, dim3((unsigned)nb), dim3(kFmtThreads), 0, s, start, end, mapq, n, p, block_agg,
                           keep_bits);
    hipLaunchKernelGGL(format_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, block_agg, nb, block_prefix, total);
}

void format_pass2(hipStream_t s, const int32_t* start, const int32_t* end, const uint8_t* mapq, const uint8_t* strand,
                  int64_t n, const RowParams& p, const RowAgg* block_prefix, uint8_t* text, int32_t* run_bin,
                  uint32_t* run_off, uint32_t* lin, int32_t n_lin, const unsigned long long* keep_bits) {
    const int64_t nb = (n + kRowsPerBlock - 1) / kRowsPerBlock;
    if (nb > 0)
        hipLaunchKernelGGL(format_pass2_kernel, dim3((unsigned)nb), dim3(kFmtThreads), 0, s, start, end, mapq, strand, n, p,
                           block_prefix, text, run_bin, run_off, lin, n_lin, keep_bits);
}

void mask_keep(hipStream_t s, const int32_t* start, const int32_t* end, int64_t n, const MaskView& m,
               unsigned long long* keep_bits) {
    const int64_t nb = (n + kRowsPerBlock - 1) / kRowsPerBlock;
    if (nb > 0)
        hipLaunchKernelGGL(mask_keep_kernel, dim3((unsigned)nb), dim3(kFmtThreads), 0, s, start, end, n, m, keep_bits,
                           (int64_t)mask_words(n));
}

// ---------------------------------------------------------------------------------------------------------------
// (c) DEFLATE of one BGZF block, plain C++ (runs on a lane of the device and, for checking, on the host)
// ---------------------------------------------------------------------------------------------------------------
FTK_HD uint32_t load32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

FTK_HD int floor_log2(uint32_t x) { return 31 - __builtin_clz(x); }

struct BitWriter {
    uint8_t* base;   // 4-byte aligned
    uint32_t pos;    // bytes written (multiple of 4 until finish)
    uint32_t limit;  // give up when the stream would pass this many bytes
    unsigned long long acc;
    int nbits;
    bool overflow;
};

FTK_HD void bw_put(BitWriter& w, uint32_t value, int n) {  // n <= 32
    w.acc |= (unsigned long long)value << w.nbits;
    w.nbits += n;
    if (w.nbits >= 32) {
        if (w.pos + 4 > w.limit) {
            w.overflow = true;
        } else {
            const uint32_t v = (uint32_t)w.acc;
            __builtin_memcpy(w.base + w.pos, &v, 4);
            w.pos += 4;
        }
        w.acc >>= 32;
        w.nbits -= 32;
    }
}

FTK_HD uint32_t bw_finish(BitWriter& w) {  // bytes of the stream
    const uint32_t tail = (uint32_t)(w.nbits + 7) / 8;
    if (w.pos + tail > w.limit) {
        w.overflow = true;
        return w.pos;
    }
    const uint32_t v = (uint32_t)w.acc;
    __builtin_memcpy(w.base + w.pos, &v, 4);  // (the slot has room behind the limit)
    return w.pos + tail;
}

FTK_HD void length_symbol(uint32_t len, int& sym, int& eb, uint32_t& ev) {  // len 3..258
    const uint32_t l = len - 3;
    if (l == 255) { sym = 285; eb = 0; ev = 0; return; }
    if (l < 4) { sym = 257 + (int)l; eb = 0; ev = 0; return; }
    const int k = floor_log2(l);
    eb = k - 2;
    sym = 257 + 4 * k - 4 + (int)((l >> eb) & 3u);
    ev = l & ((1u << eb) - 1u);
}

FTK_HD void dist_symbol(uint32_t dist, int& sym, int& eb, uint32_t& ev) {  // dist 1..32768
    const uint32_t d = dist - 1;
    if (d < 2) { sym = (int)d; eb = 0; ev = 0; return; }
    const int k = floor_log2(d);
    eb = k - 1;
    sym = 2 * k + (int)((d >> eb) & 1u);
    ev = d & ((1u << eb) - 1u);
}

FTK_HD int fixed_litlen_bits(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }

// Code lengths (<= limit) of a complete prefix code for the symbols with freq > 0.  Shannon lengths
// ceil(log2(total / f)) satisfy Kraft's inequality; where the clamp to `limit` breaks it, the rarest symbols are
// lengthened; then the gap to a COMPLETE code (zlib's inflate refuses incomplete ones) is closed by shortening, one
// step at a time, the most frequent symbol whose step still fits - a symbol of the greatest length always does.
FTK_HD void code_lengths(const uint16_t* freq, int n, int limit, uint8_t* len) {
    uint32_t total = 0;
    int nz = 0, one = -1;
    for (int i = 0; i < n; ++i) {
        len[i] = 0;
        if (freq[i]) { total += freq[i]; ++nz; one = i; }
    }
    if (nz == 0) { len[0] = len[1] = 1; return; }
    if (nz == 1) { len[one] = 1; len[one ? 0 : 1] = 1; return; }
    const int32_t cap = 1 << limit;
    int32_t kraft = 0;
    for (int i = 0; i < n; ++i) {
        if (!freq[i]) continue;
        int l = 1;
        while (((uint32_t)freq[i] << l) < total) ++l;
        if (l > limit) l = limit;
        len[i] = (uint8_t)l;
        kraft += 1 << (limit - l);
    }
    while (kraft > cap) {
        int best = -1;
        for (int i = 0; i < n; ++i)
            if (len[i] && len[i] < limit && (best < 0 || freq[i] <= freq[best])) best = i;
        ++len[best];
        kraft -= 1 << (limit - len[best]);
    }
    while (kraft < cap) {
        const int32_t gap = cap - kraft;
        int best = -1;
        for (int i = 0; i < n; ++i)
            if (len[i] > 1 && (1 << (limit - len[i])) <= gap && (best < 0 || freq[i] > freq[best])) best = i;
        if (best < 0) break;  // (cannot happen: a symbol of the greatest length fits)
        kraft += 1 << (limit - len[best]);
        --len[best];
    }
}

FTK_HD uint16_t bit_reverse(uint32_t code, int len) {
    uint32_t r = 0;
    for (int k = 0; k < len; ++k) r |= ((code >> k) & 1u) << (len - 1 - k);
    return (uint16_t)r;
}

FTK_HD void canonical_codes(const uint8_t* len, int n, int limit, uint16_t* code) {  // RFC 1951 3.2.2, bit-reversed
    uint16_t count[16], next[16];
    for (int l = 0; l <= limit; ++l) count[l] = 0;
    for (int i = 0; i < n; ++i) ++count[len[i]];
    count[0] = 0;
    uint32_t c = 0;
    next[0] = 0;
    for (int l = 1; l <= limit; ++l) {
        c = (c + count[l - 1]) << 1;
        next[l] = (uint16_t)c;
    }
    for (int i = 0; i < n; ++i) code[i] = len[i] ? bit_reverse(next[len[i]]++, len[i]) : (uint16_t)0;
}

struct BlockCodes {
    uint16_t ll_freq[286], d_freq[30];
    uint8_t ll_len[286], d_len[30];
    uint16_t ll_code[286], d_code[30];
    uint32_t extra_bits;
};

FTK_HD void codes_reset(BlockCodes& c) {
    for (int i = 0; i < 286; ++i) c.ll_freq[i] = 0;
    for (int i = 0; i < 30; ++i) c.d_freq[i] = 0;
    c.extra_bits = 0;
}

// One DEFLATE block from n_tok tokens (literal: the byte; match: bit 31 | (len - 3) << 16 | (dist - 1)).
FTK_HD void emit_block(BitWriter& w, const uint32_t* tok, int n_tok, BlockCodes& c, bool final) {
    c.ll_freq[256] = 1;
    // ---- the dynamic code and what its header costs
    code_lengths(c.ll_freq, 286, 15, c.ll_len);
    code_lengths(c.d_freq, 30, 15, c.d_len);
    int n_ll = 286, n_d = 30;
    while (n_ll > 257 && !c.ll_len[n_ll - 1]) --n_ll;
    while (n_d > 1 && !c.d_len[n_d - 1]) --n_d;
    uint16_t seq[316];  // code-length symbols: sym | extra value << 8
    int n_seq = 0;
    uint16_t cl_freq[19];
    for (int i = 0; i < 19; ++i) cl_freq[i] = 0;
    {
        const int n_all = n_ll + n_d;
        int i = 0;
        while (i < n_all) {
            const int l = i < n_ll ? c.ll_len[i] : c.d_len[i - n_ll];
            if (l) {
                seq[n_seq++] = (uint16_t)l;
                ++cl_freq[l];
                ++i;
                continue;
            }
            int run = 1;
            while (i + run < n_all && run < 138 && !((i + run) < n_ll ? c.ll_len[i + run] : c.d_len[i + run - n_ll])) ++run;
            if (run >= 11) {
                seq[n_seq++] = (uint16_t)(18 | ((run - 11) << 8));
                ++cl_freq[18];
            } else if (run >= 3) {
                seq[n_seq++] = (uint16_t)(17 | ((run - 3) << 8));
                ++cl_freq[17];
            } else {
                for (int k = 0; k < run; ++k) seq[n_seq++] = 0;
                cl_freq[0] += (uint16_t)run;
            }
            i += run;
        }
    }
    uint8_t cl_len[19];
    uint16_t cl_code[19];
    code_lengths(cl_freq, 19, 7, cl_len);
    canonical_codes(cl_len, 19, 7, cl_code);
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int n_cl = 19;
    while (n_cl > 4 && !cl_len[order[n_cl - 1]]) --n_cl;
    uint32_t dyn_bits = 14 + 3 * (uint32_t)n_cl + 3u * cl_freq[17] + 7u * cl_freq[18];
    for (int i = 0; i < 19; ++i) dyn_bits += (uint32_t)cl_freq[i] * cl_len[i];
    uint32_t fix_bits = 0;
    for (int i = 0; i < n_ll; ++i) {
        dyn_bits += (uint32_t)c.ll_freq[i] * c.ll_len[i];
        fix_bits += (uint32_t)c.ll_freq[i] * (uint32_t)fixed_litlen_bits(i);
    }
    for (int i = 0; i < n_d; ++i) {
        dyn_bits += (uint32_t)c.d_freq[i] * c.d_len[i];
        fix_bits += 5u * c.d_freq[i];
    }
    const bool dynamic = dyn_bits < fix_bits;
    bw_put(w, final ? 1u : 0u, 1);
    bw_put(w, dynamic ? 2u : 1u, 2);
    if (dynamic) {
        bw_put(w, (uint32_t)(n_ll - 257), 5);
        bw_put(w, (uint32_t)(n_d - 1), 5);
        bw_put(w, (uint32_t)(n_cl - 4), 4);
        for (int i = 0; i < n_cl; ++i) bw_put(w, cl_len[order[i]], 3);
        for (int i = 0; i < n_seq; ++i) {
            const int sym = seq[i] & 255;
            bw_put(w, cl_code[sym], cl_len[sym]);
            if (sym == 17) bw_put(w, (uint32_t)(seq[i] >> 8), 3);
            if (sym == 18) bw_put(w, (uint32_t)(seq[i] >> 8), 7);
        }
        canonical_codes(c.ll_len, 286, 15, c.ll_code);
        canonical_codes(c.d_len, 30, 15, c.d_code);
    } else {
        for (int i = 0; i < 286; ++i) c.ll_len[i] = (uint8_t)fixed_litlen_bits(i);
        for (int i = 0; i < 30; ++i) c.d_len[i] = 5;
        // (the fixed code is the canonical code of the lengths 8 / 9 / 7 / 8 over 288 symbols; 286 and 287 never occur
        // and are the last two of the 8-bit group, so leaving them out moves no code)
        for (int i = 0; i < 286; ++i) {
            const uint32_t code = i < 144 ? 0x30u + i : i < 256 ? 0x190u + (i - 144) : i < 280 ? (uint32_t)(i - 256) : 0xC0u + (i - 280);
            c.ll_code[i] = bit_reverse(code, c.ll_len[i]);
        }
        for (int i = 0; i < 30; ++i) c.d_code[i] = bit_reverse((uint32_t)i, 5);
    }
    for (int t = 0; t < n_tok && !w.overflow; ++t) {
        const uint32_t k = tok[t];
        if (!(k >> 31)) {
            bw_put(w, c.ll_code[k], c.ll_len[k]);
            continue;
        }
        int sym, eb;
        uint32_t ev;
        length_symbol(((k >> 16) & 255u) + 3u, sym, eb, ev);
        bw_put(w, (uint32_t)c.ll_code[sym] | (ev << c.ll_len[sym]), c.ll_len[sym] + eb);
        dist_symbol((k & 0x7FFFu) + 1u, sym, eb, ev);
        bw_put(w, (uint32_t)c.d_code[sym] | (ev << c.d_len[sym]), c.d_len[sym] + eb);
    }
    bw_put(w, c.ll_code[256], c.ll_len[256]);
    codes_reset(c);
}

// The raw DEFLATE stream of in[0..n) (1 <= n <= 0xFF00) at `payload` (4-byte aligned, n + 16 bytes of room); returns
// its size, at most n + 5.  hash: kDeflateHash entries whose upper 16 bits differ from `gen` (or are stale); tok:
// kDeflateTokens entries.
FTK_HD uint32_t deflate_payload(const uint8_t* in, uint32_t n, uint8_t* payload, uint32_t* hash, uint32_t gen, uint32_t* tok) {
    BitWriter w{payload, 0u, n + 5u, 0ull, 0, false};
    BlockCodes c;
    codes_reset(c);
    int n_tok = 0;
    uint32_t p = 0;
    const uint32_t tag = gen << 16;
    while (p < n && !w.overflow) {
        uint32_t len = 0, dist = 0;
        if (p + 4 <= n) {
            const uint32_t v = load32(in + p);
            const uint32_t h = (v * 2654435761u) >> 20;
            const uint32_t e = hash[h];
            hash[h] = tag | p;
            if ((e & 0xFFFF0000u) == tag) {
                const uint32_t q = e & 0xFFFFu;
                if (p - q <= 32768u && load32(in + q) == v) {
                    const uint32_t max_len = n - p < 258u ? n - p : 258u;
                    len = 4;
                    while (len + 4 <= max_len && load32(in + q + len) == load32(in + p + len)) len += 4;
                    while (len < max_len && in[q + len] == in[p + len]) ++len;
                    dist = p - q;
                }
            }
        }
        if (len) {
            int sym, eb;
            uint32_t ev;
            length_symbol(len, sym, eb, ev);
            ++c.ll_freq[sym];
            c.extra_bits += (uint32_t)eb;
            dist_symbol(dist, sym, eb, ev);
            ++c.d_freq[sym];
            c.extra_bits += (uint32_t)eb;
            tok[n_tok++] = 0x80000000u | ((len - 3u) << 16) | (dist - 1u);
            for (uint32_t q = p + 1; q < p + len && q + 4 <= n; ++q) hash[(load32(in + q) * 2654435761u) >> 20] = tag | q;
            p += len;
        } else {
            ++c.ll_freq[in[p]];
            tok[n_tok++] = in[p];
            ++p;
        }
        if (n_tok == kDeflateTokens && p < n) {
            emit_block(w, tok, n_tok, c, false);
            n_tok = 0;
        }
    }
    if (!w.overflow) emit_block(w, tok, n_tok, c, true);
    uint32_t size = w.overflow ? 0u : bw_finish(w);
    if (w.overflow) {  // does not compress: one stored block
        payload[0] = 1;
        payload[1] = (uint8_t)(n & 255u);
        payload[2] = (uint8_t)(n >> 8);
        payload[3] = (uint8_t)(~n & 255u);
        payload[4] = (uint8_t)((~n >> 8) & 255u);
        for (uint32_t i = 0; i < n; ++i) payload[5 + i] = in[i];
        size = n + 5u;
    }
    return size;
}

// The member of one block in its slot: slot[2..20) header, payload from slot[20), ISIZE; the CRC is filled in by the
// compaction.  Returns the member's size.
FTK_HD uint32_t deflate_member(const uint8_t* in, uint32_t n, uint8_t* slot, uint32_t* hash, uint32_t gen, uint32_t* tok) {
    const uint32_t payload = deflate_payload(in, n, slot + 20, hash, gen, tok);
    const uint32_t total = 18u + payload + 8u;
    const uint8_t head[18] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, (uint8_t)((total - 1u) & 255u),
                              (uint8_t)((total - 1u) >> 8)};
    for (int i = 0; i < 18; ++i) slot[2 + i] = head[i];
    uint8_t* tr = slot + 20 + payload;
    for (int i = 0; i < 4; ++i) tr[i] = 0;
    for (int i = 0; i < 4; ++i) tr[4 + i] = (uint8_t)(n >> (8 * i));
    return total;
}

namespace {

__global__ __launch_bounds__(64) void bgzf_deflate_kernel(const uint8_t* __restrict__ text, unsigned long long n,
                                                          long long n_blocks, int lanes, uint8_t* __restrict__ slots,
                                                          uint32_t* __restrict__ sizes, InflateBlock* __restrict__ tab,
                                                          uint32_t* __restrict__ hash, uint32_t* __restrict__ tokens) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= lanes) return;
    uint32_t* my_hash = hash + (size_t)g * kDeflateHash;
    uint32_t* my_tok = tokens + (size_t)g * kDeflateTokens;
    uint32_t gen = 0;
    for (long long b = g; b < n_blocks; b += lanes) {
        const unsigned long long off = (unsigned long long)b * kBgzfData;
        const uint32_t len = (uint32_t)(n - off < (unsigned long long)kBgzfData ? n - off : (unsigned long long)kBgzfData);
        ++gen;  // (the hash scratch is cleared per call; a lane meets fewer than 2^16 blocks: n < 2^32)
        sizes[b] = deflate_member(text + off, len, slots + (size_t)b * kBgzfSlot, my_hash, gen, my_tok);
        tab[b] = InflateBlock{0u, 0u, (uint32_t)off, len};
    }
}

// offs[k] = sum of sizes[0..k), offs[n] = total (one workgroup; n is a few thousand per contig)
__global__ __launch_bounds__(1024) void sizes_scan_kernel(const uint32_t* __restrict__ sizes, long long n,
                                                           unsigned long long* __restrict__ offs) {
    __shared__ unsigned long long sh[2][1024];
    __shared__ unsigned long long carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (long long base = 0; base < n; base += 1024) {
        const long long i = base + t;
        int cur = 0;
        sh[0][t] = i < n ? sizes[i] : 0u;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            unsigned long long x = sh[cur][t];
            if (t >= d) x += sh[cur][t - d];
            sh[cur ^ 1][t] = x;
            cur ^= 1;
            __syncthreads();
        }
        const unsigned long long c = carry, inc = sh[cur][t];
        if (i < n) offs[i] = c + inc - sizes[i];
        __syncthreads();
        if (t == 1023) carry = c + inc;
        __syncthreads();
    }
    if (t == 0) offs[n] = carry;
}

__global__ __launch_bounds__(256) void bgzf_compact_kernel(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ sizes,
                                                           const uint32_t* __restrict__ crc,
                                                           const unsigned long long* __restrict__ offs,
                                                           uint8_t* __restrict__ out) {
    const size_t b = blockIdx.x;
    const uint8_t* src = slots + b * kBgzfSlot + 2;
    uint8_t* dst = out + offs[b];
    const uint32_t size = sizes[b], c = crc[b];
    for (uint32_t i = threadIdx.x; i < size; i += 256) {
        uint8_t v = src[i];
        const uint32_t k = i - (size - 8u);  // CRC bytes: size - 8 .. size - 5
        if (i >= size - 8u && k < 4u) v = (uint8_t)(c >> (8u * k));
        dst[i] = v;
    }
}

}  // namespace

void deflate_members(hipStream_t s, const uint8_t* text, int64_t n, const DeflateScratch& sc) {
    const int64_t nb = bgzf_blocks(n);
    if (nb <= 0) return;
    const int lanes = deflate_lanes(nb);
    (void)hipMemsetAsync(sc.hash, 0, (size_t)lanes * kDeflateHash * sizeof(uint32_t), s);
    hipLaunchKernelGGL(bgzf_deflate_kernel, dim3((lanes + 63) / 64), dim3(64), 0, s, text, (unsigned long long)n,
                       (long long)nb, lanes, sc.slots, sc.sizes, sc.tab, sc.hash, sc.tokens);
    crc_launch(s, sc.tab, (int)nb, text, sc.crc);
}

void deflate_compact(hipStream_t s, int64_t n_blocks, const DeflateScratch& sc) {
    if (n_blocks <= 0) return;
    hipLaunchKernelGGL(sizes_scan_kernel, dim3(1), dim3(1024), 0, s, sc.sizes, (long long)n_blocks, sc.offs);
    hipLaunchKernelGGL(bgzf_compact_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, sc.slots, sc.sizes, sc.crc, sc.offs, sc.out);
}

}  // namespace ftk
