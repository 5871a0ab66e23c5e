// Nucleosome calls from an adjusted WPS track (ftk_track_peaks, ftk_wps_peaks); the rule is stated in include/ftk.h,
// "peaks".  Every comparison and every sum is float64, no float meets an atomic, and a call's values depend on its
// region's scores alone: the same bits whatever else the launch holds.
//
// peaks_mark_kernel   one workgroup per tile of kPeaksTile positions of one run.  The tile and a halo of kPeaksHalo
//                     positions on either side become one bit per position ("inside the callable track and > 0";
//                     positions beyond the run's ends are never read and count as 0), 18 words of LDS.  A position
//                     starts a region when it is set and the max_gap + 1 bits before it are clear - one 64-bit window
//                     cut from two words - and ends one by the mirror test.  The first launch counts starts and ends
//                     per tile (and flags a score that is not finite); after the scan the second launch writes them at
//                     offset + rank, the rank from popcounts of the tile's start / end words, so the lists are in
//                     position order and the k-th start pairs with the k-th end.
// peaks_scan_kernel   exclusive scan of 64-bit counts by one workgroup, 8 192 elements per trip; starts and ends share a
//                     word (low / high half), so one scan serves both.
// peaks_call_kernel   one wave per region.  First launch: classify (open / short / long), stage the <= 1024 values in
//                     LDS, sort a padded copy bitonically for the median, walk the windows, count the calls and keep
//                     the median.  After the scan of the counts the second launch stages the called regions again,
//                     walks the windows against the kept median and writes the calls at offset + rank: ordered by
//                     (run, start) whatever the block schedule.  A window is walked by the lane that owns its first
//                     element, left to right, one addition per value.
#include <cfloat>
#include <cmath>

#include "ftk_device.h"
#include "ftk_peaks.h"

namespace ftk {

namespace {

constexpr int kMarkThreads = 256;
constexpr int kMarkWords = (kPeaksTile + 2 * kPeaksHalo) / 64;  // 18
constexpr int kTileWords = kPeaksTile / 64;                     // 16
constexpr int kScanPerThread = 8;
static_assert(kPeaksHalo == 64 && kPeaksMaxGap + 1 <= kPeaksHalo, "a neighbourhood is one 64-bit window");
static_assert(kPeaksTile % kMarkThreads == 0 && kMarkThreads % 64 == 0, "whole waves per trip");

__device__ inline int popc64(uint64_t x) { return __popcll((unsigned long long)x); }

template <bool WRITE>
__global__ __launch_bounds__(kMarkThreads) void peaks_mark_kernel(const double* __restrict__ a, const int64_t* __restrict__ off,
                                                                  const int32_t* __restrict__ tile_run,
                                                                  const int32_t* __restrict__ tile_k, int skip, int gap,
                                                                  uint64_t* __restrict__ tile_cnt, int64_t* __restrict__ reg_start,
                                                                  int64_t* __restrict__ reg_end, int32_t* __restrict__ reg_run,
                                                                  int64_t reg_cap, int* __restrict__ bad) {
    __shared__ uint64_t pos_bits[kMarkWords];
    __shared__ uint64_t start_bits[kTileWords], end_bits[kTileWords];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int run = tile_run[t];
    const int64_t base = off[run], n = off[run + 1] - base;
    const int64_t lo = skip, hi = n - skip;
    const int64_t p0 = (int64_t)tile_k[t] * kPeaksTile;  // the tile's first position of the run
    // bit q of pos_bits: position p0 - kPeaksHalo + q
    for (int it = 0; it * kMarkThreads < kPeaksTile + 2 * kPeaksHalo; ++it) {
        const int q = it * kMarkThreads + tid;
        const int64_t p = p0 - kPeaksHalo + q;
        bool pos = false;
        if (q < kPeaksTile + 2 * kPeaksHalo && p >= 0 && p < n) {
            const double v = a[base + p];
            if (!WRITE && q >= kPeaksHalo && q < kPeaksHalo + kPeaksTile && !(fabs(v) <= DBL_MAX)) *bad = 1;
            pos = v > 0.0 && p >= lo && p < hi;
        }
        const uint64_t m = __ballot(pos);
        const int w = it * (kMarkThreads / 64) + wave;
        if (lane == 0 && w < kMarkWords) pos_bits[w] = m;
    }
    __syncthreads();
    const int g1 = gap + 1;  // 1 .. 64
    for (int it = 0; it < kPeaksTile / kMarkThreads; ++it) {
        const int q = it * kMarkThreads + tid + kPeaksHalo, qi = q >> 6, r = q & 63;
        const bool pos = (pos_bits[qi] >> r) & 1;
        // the 64 positions before q (the nearest in the top bit) and the 64 behind it (the nearest in the bottom bit)
        const uint64_t before = r ? (pos_bits[qi - 1] >> r) | (pos_bits[qi] << (64 - r)) : pos_bits[qi - 1];
        const int s = q + 1, si = s >> 6, sr = s & 63;
        const uint64_t behind = sr ? (pos_bits[si] >> sr) | (pos_bits[si + 1] << (64 - sr)) : pos_bits[si];
        const uint64_t sm = __ballot(pos && (before >> (64 - g1)) == 0);
        const uint64_t em = __ballot(pos && (behind << (64 - g1)) == 0);
        if (lane == 0) {
            start_bits[it * (kMarkThreads / 64) + wave] = sm;
            end_bits[it * (kMarkThreads / 64) + wave] = em;
        }
    }
    __syncthreads();
    if (!WRITE) {
        if (tid == 0) {
            uint32_t ns = 0, ne = 0;
            for (int w = 0; w < kTileWords; ++w) {
                ns += popc64(start_bits[w]);
                ne += popc64(end_bits[w]);
            }
            tile_cnt[t] = (uint64_t)ns | ((uint64_t)ne << 32);
        }
        return;
    }
    const uint64_t first = tile_cnt[t];  // (scanned: the starts and the ends in front of this tile)
    for (int it = 0; it < kPeaksTile / kMarkThreads; ++it) {
        const int w = it * (kMarkThreads / 64) + wave;
        const int64_t at = base + p0 + it * kMarkThreads + tid;
        const uint64_t below = (uint64_t(1) << lane) - 1;
        if ((start_bits[w] >> lane) & 1) {
            int64_t k = (uint32_t)first + popc64(start_bits[w] & below);
            for (int x = 0; x < w; ++x) k += popc64(start_bits[x]);
            if (k < reg_cap) {
                reg_start[k] = at;
                reg_run[k] = run;
            }
        }
        if ((end_bits[w] >> lane) & 1) {
            int64_t k = (uint32_t)(first >> 32) + popc64(end_bits[w] & below);
            for (int x = 0; x < w; ++x) k += popc64(end_bits[x]);
            if (k < reg_cap) reg_end[k] = at + 1;
        }
    }
}

// v[i] = *running + sum of v[0 .. i) for i <= n, then *running = v[n] (running NULL: 0, and nothing kept).  n: n_host, or
// the low half of *n_dev where that is given (a count the device holds) and smaller.
__global__ __launch_bounds__(1024) void peaks_scan_kernel(uint64_t* __restrict__ v, int64_t n_host, const uint64_t* __restrict__ n_dev,
                                                          uint64_t* __restrict__ running) {
    __shared__ uint64_t wave_tot[16];
    __shared__ uint64_t carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n = n_dev ? min((int64_t)(uint32_t)*n_dev, n_host) : n_host;
    if (tid == 0) carry = running ? *running : 0;
    __syncthreads();
    for (int64_t c0 = 0; c0 < n; c0 += 1024 * kScanPerThread) {
        const int64_t i0 = c0 + (int64_t)tid * kScanPerThread;
        uint64_t x[kScanPerThread], sum = 0;
#pragma unroll
        for (int k = 0; k < kScanPerThread; ++k) {
            x[k] = i0 + k < n ? v[i0 + k] : 0;
            sum += x[k];
        }
        uint64_t inc = sum;
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t y = __shfl_up((unsigned long long)inc, d);
            if (lane >= d) inc += y;
        }
        if (lane == 63) wave_tot[wave] = inc;
        __syncthreads();
        uint64_t at = carry + inc - sum;
        for (int w = 0; w < wave; ++w) at += wave_tot[w];
#pragma unroll
        for (int k = 0; k < kScanPerThread; ++k) {
            if (i0 + k < n) v[i0 + k] = at;
            at += x[k];
        }
        __syncthreads();
        if (tid == 1023) carry = at;
        __syncthreads();
    }
    if (tid == 0) {
        v[n] = carry;
        if (running) *running = carry;
    }
}

struct Window {
    int start, len, summit;
    double height, area;
};

template <bool EMIT>
__global__ __launch_bounds__(64) void peaks_call_kernel(const double* __restrict__ a, const int64_t* __restrict__ off, int n_runs,
                                                        PeaksParams P, const uint64_t* __restrict__ n_regions,
                                                        const int64_t* __restrict__ reg_start, const int64_t* __restrict__ reg_end,
                                                        double* __restrict__ reg_med, uint64_t* __restrict__ reg_cnt,
                                                        unsigned long long* __restrict__ stats, int run_base, PeaksBufs o) {
    __shared__ double vals[kPeaksMaxRegion];
    __shared__ double sorted[EMIT ? 1 : kPeaksMaxRegion];
    const int lane = threadIdx.x;
    const uint32_t n_reg = min((uint64_t)(uint32_t)*n_regions, (uint64_t)o.reg_cap);
    for (uint32_t k = blockIdx.x; k < n_reg; k += gridDim.x) {  // (every test below is the same in all lanes)
        uint64_t first = 0;
        if (EMIT) {
            first = reg_cnt[k];
            if (reg_cnt[k + 1] == first) continue;
        }
        const int64_t rs = reg_start[k], re = reg_end[k];
        const int r = o.reg_run[k];
        if (r < 0 || r >= n_runs) continue;  // (cannot be)
        const int64_t base = off[r], n = off[r + 1] - base, lo = P.skip, hi = n - P.skip;
        const int64_t r0 = rs - base, r1 = re - base, len64 = r1 - r0;
        if (!EMIT) {
            unsigned long long* st = stats + (size_t)(run_base + r) * 6;
            const bool open = r0 - lo <= P.max_gap || hi - r1 <= P.max_gap;
            const int kind = open ? 1 : len64 < P.min_region ? 2 : len64 > P.max_region ? 3 : 0;
            if (lane == 0) {
                atomicAdd(st + 0, 1ull);
                if (kind) atomicAdd(st + kind, 1ull);
            }
            if (kind || len64 < 1 || r1 > n) {  // (starts and ends out of step: cannot be, and must not index LDS or leave the run)
                if (lane == 0) reg_cnt[k] = 0;
                continue;
            }
        }
        if (len64 < 1 || len64 > kPeaksMaxRegion || r1 > n) continue;
        const int L = (int)len64;
        __syncthreads();  // (the previous region's readers are done with the LDS)
        for (int i = lane; i < L; i += 64) vals[i] = a[rs + i];
        double m;
        if (!EMIT) {
            int n2 = 1;
            while (n2 < L) n2 <<= 1;
            for (int i = lane; i < n2; i += 64) sorted[i] = i < L ? a[rs + i] : HUGE_VAL;
            __syncthreads();
            for (int size = 2; size <= n2; size <<= 1)
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    for (int t = lane; t < n2 / 2; t += 64) {
                        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                        const double x = sorted[i], y = sorted[j];
                        if ((x > y) == ((i & size) == 0)) {
                            sorted[i] = y;
                            sorted[j] = x;
                        }
                    }
                    __syncthreads();
                }
            m = (L & 1) ? sorted[L / 2] : (sorted[L / 2 - 1] + sorted[L / 2]) / 2.0;
            if (lane == 0) reg_med[k] = m;
        } else {
            m = reg_med[k];
            __syncthreads();
        }
        const bool single = L <= P.short_max;
        Window best{-1, 0, 0, 0.0, 0.0};
        uint32_t calls = 0;
        bool any = false;
        for (int c = 0; c < L; c += 64) {
            const int i = c + lane;
            const bool starts = i < L && vals[i] > m && !(i > 0 && vals[i - 1] > m);
            Window w{i, 0, i, 0.0, 0.0};
            if (starts) {
                w.height = vals[i];
                int j = i;
                do {
                    const double v = vals[j];
                    w.area = w.area + v;
                    if (v > w.height) {
                        w.height = v;
                        w.summit = j;
                    }
                    ++j;
                } while (j < L && vals[j] > m);
                w.len = j - i;
            }
            any |= __ballot(starts) != 0;
            if (single) {
                if (starts && (best.start < 0 || w.area > best.area)) best = w;  // (a lane meets its windows left to right)
            } else {
                const bool called = starts && w.len >= P.min_region && w.len <= P.short_max;
                const uint64_t mask = __ballot(called);
                if (EMIT && called) {
                    const int64_t at = (int64_t)first + calls + popc64(mask & ((uint64_t(1) << lane) - 1));
                    if (at < o.out_cap) {
                        o.o_run[at] = run_base + r;
                        o.o_start[at] = r0 + w.start;
                        o.o_stop[at] = r0 + w.start + w.len;
                        o.o_summit[at] = r0 + w.summit;
                        o.o_height[at] = w.height;
                        o.o_area[at] = w.area;
                    }
                }
                calls += popc64(mask);
            }
        }
        if (single && any) {
            double win_area = best.area;
            int win_start = best.start;
            for (int d = 32; d > 0; d >>= 1) {  // the largest area, the leftmost of equals
                const double oa = __shfl_xor(win_area, d);
                const int os = __shfl_xor(win_start, d);
                if (os >= 0 && (win_start < 0 || oa > win_area || (oa == win_area && os < win_start))) {
                    win_area = oa;
                    win_start = os;
                }
            }
            calls = 1;
            if (EMIT && best.start == win_start && (int64_t)first < o.out_cap) {
                o.o_run[first] = run_base + r;
                o.o_start[first] = r0 + best.start;
                o.o_stop[first] = r0 + best.start + best.len;
                o.o_summit[first] = r0 + best.summit;
                o.o_height[first] = best.height;
                o.o_area[first] = best.area;
            }
        }
        if (!EMIT && lane == 0) {
            reg_cnt[k] = calls;
            unsigned long long* st = stats + (size_t)(run_base + r) * 6;
            if (!any) atomicAdd(st + 4, 1ull);
            if (calls) atomicAdd(st + 5, (unsigned long long)calls);
        }
    }
}

__global__ __launch_bounds__(256) void i64_to_f64_kernel(void* v, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const int64_t x = ((const int64_t*)v)[i];
        ((double*)v)[i] = (double)x;
    }
}

}  // namespace

void launch_peaks(hipStream_t s, const double* a, const int64_t* off, int n_runs, int64_t n_tiles, const PeaksParams& p,
                  int run_base, const PeaksBufs& b) {
    if (n_tiles <= 0 || n_runs <= 0) return;
    peaks_mark_kernel<false><<<(unsigned)n_tiles, kMarkThreads, 0, s>>>(a, off, b.tile_run, b.tile_k, p.skip, p.max_gap, b.tile_cnt,
                                                                        b.reg_start, b.reg_end, b.reg_run, b.reg_cap, b.bad);
    peaks_scan_kernel<<<1, 1024, 0, s>>>(b.tile_cnt, n_tiles, nullptr, nullptr);
    peaks_mark_kernel<true><<<(unsigned)n_tiles, kMarkThreads, 0, s>>>(a, off, b.tile_run, b.tile_k, p.skip, p.max_gap, b.tile_cnt,
                                                                       b.reg_start, b.reg_end, b.reg_run, b.reg_cap, b.bad);
    // one wave per region, as many of them as keep the device full; a wave takes every grid-th region
    const unsigned grid = (unsigned)std::min<int64_t>(std::max<int64_t>(b.reg_cap, 1), 1 << 14);
    const uint64_t* n_regions = b.tile_cnt + n_tiles;
    peaks_call_kernel<false><<<grid, 64, 0, s>>>(a, off, n_runs, p, n_regions, b.reg_start, b.reg_end, b.reg_med, b.reg_cnt,
                                                 (unsigned long long*)b.stats, run_base, b);
    peaks_scan_kernel<<<1, 1024, 0, s>>>(b.reg_cnt, b.reg_cap, n_regions, b.n_calls);
    peaks_call_kernel<true><<<grid, 64, 0, s>>>(a, off, n_runs, p, n_regions, b.reg_start, b.reg_end, b.reg_med, b.reg_cnt,
                                                (unsigned long long*)b.stats, run_base, b);
}

void launch_i64_to_f64(hipStream_t s, void* v, int64_t n) {
    if (n > 0) i64_to_f64_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(v, n);
}

}  // namespace ftk
