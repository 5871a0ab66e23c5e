// Periodogram of integer score runs at integer periods (ftk_track_spectrum, ftk_wps_spectrum); the rule is stated in
// include/ftk.h, "spectrum".  All arithmetic is float64.
//
// The twiddle of sample n at period p depends on j = n mod p alone, so the sum over n factors:
//     re_p = sum_j cos(2 pi j / p) * F[j],   F[j] = sum_k x[j + k P],   P = p * q a multiple of p
// The N samples of a run are FOLDED into P bins with one addition each - no multiply and no table read per (sample,
// period) - and only the P bins meet the twiddles.  That is half the flops of the direct contraction and half of
// its bytes per (sample, period): one float64 of x instead of the sample's 16-byte (cos, sin) pair.
//
// spectrum_twiddle_kernel  the table of every requested period: (cos, sin)(2 pi j / p), j < p, the angle formed as
//                          ((2 pi) * j) / p.
// spectrum_prep_kernel     one workgroup per run: sum v exactly in int64 (and flag |v| >= 2^31), m = sum / N in one
//                          float64 division, x[n] = (v[n] - m) * w[n] to a device array, and ssw = (N - 2 M) + 2 * sum
//                          of w^2 over the left bell.  The right bell is evaluated from its mirror index, so w[n] and
//                          w[N - 1 - n] are the same bits.
// spectrum_fold_kernel     one WAVE per (run, period).  A run of at most kSpectrumLdsSamples samples is copied to LDS
//                          once per workgroup of eight waves, which then takes kSpectrumStagedPeriods periods from
//                          it (x crosses the L2 once per 32 periods, not once per period); a longer run is read from
//                          memory, kSpectrumWaves periods per workgroup.  The same code adds the same numbers in
//                          the same order either way.  P = p * max(1, 64 / p): periods below 33 fold to a multiple of
//                          themselves so that the 64 lanes all own a bin.  Lane l owns the bins j = l, l + 64, ... < P;
//                          a bin is summed in four interleaved partial sums (k mod 4) joined as (a0 + a1) + (a2 + a3),
//                          multiplied by the twiddle of j mod p and added to the lane's (re, im) in rising j; a
//                          butterfly over the wave (xor 32, 16, ... 1) closes the sum.  Consecutive lanes read
//                          consecutive float64.
//
// Order: what is added to what depends on N and p only - not on the other runs or periods of the call, on their order,
// on the grid or on the run's address - and no atomic touches a float.  A (run, period) result is therefore the same bits
// in every call that asks for it.  LDS holds a whole run or nothing, so a run's length is bounded by kSpectrumMaxRun alone.
#include <algorithm>
#include <cmath>

#include "ftk_device.h"
#include "ftk_spectrum.h"

namespace ftk {

namespace {

constexpr int kSpecThreads = 64 * kSpectrumWaves;

__global__ __launch_bounds__(256) void spectrum_twiddle_kernel(const int32_t* __restrict__ periods, const int32_t* __restrict__ tab_off,
                                                               Twiddle* __restrict__ table) {
    const int p = periods[blockIdx.x];
    Twiddle* t = table + tab_off[blockIdx.x];
    for (int j = threadIdx.x; j < p; j += 256) {
        const double ang = (2.0 * M_PI) * (double)j / (double)p;
        double s, c;
        sincos(ang, &s, &c);
        t[j] = Twiddle{c, s};
    }
}

__global__ __launch_bounds__(256) void spectrum_prep_kernel(const int64_t* __restrict__ v, const int64_t* __restrict__ beg,
                                                            const int64_t* __restrict__ end, double taper, int detrend,
                                                            double* __restrict__ x, double* __restrict__ ssw,
                                                            int* __restrict__ bad) {
    __shared__ unsigned long long sum_s[4];
    __shared__ double sq_s[256];
    const int tid = threadIdx.x;
    const long long a = beg[blockIdx.x];
    const int N = (int)(end[blockIdx.x] - a);  // 0 <= N <= kSpectrumMaxRun (checked by the caller)
    if (N <= 0) {
        if (tid == 0 && ssw) ssw[blockIdx.x] = 0.0;
        return;
    }
    const int64_t* vr = v + a;
    unsigned long long part = 0;  // (unsigned: a run that holds out-of-range values may wrap; the call then fails)
    bool wide = false;
    for (int n = tid; n < N; n += 256) {
        const long long val = vr[n];
        part += (unsigned long long)val;
        wide |= val >= (1LL << 31) || val <= -(1LL << 31);
    }
    for (int d = 32; d; d >>= 1) part += __shfl_xor(part, d);
    const bool wave_wide = __ballot(wide) != 0;
    if ((tid & 63) == 0) {
        sum_s[tid >> 6] = part;
        if (wave_wide) atomicOr(bad, 1);
    }
    __syncthreads();
    const long long total = (long long)(sum_s[0] + sum_s[1] + sum_s[2] + sum_s[3]);
    const double m = detrend ? (double)total / (double)N : 0.0;
    const int M = (int)floor(taper * (double)N);  // <= N / 2: the bells do not meet
    double* xr = x + a;
    double sq = 0.0;
    for (int n = tid; n < N; n += 256) {
        const int e = min(n, N - 1 - n);
        double w = 1.0;
        if (e < M) {
            w = 0.5 * (1.0 - cos(M_PI * (double)(2 * e + 1) / (double)(2 * M)));
            if (n < M) sq += w * w;
        }
        xr[n] = ((double)vr[n] - m) * w;
    }
    sq_s[tid] = sq;
    __syncthreads();
    for (int d = 128; d; d >>= 1) {
        if (tid < d) sq_s[tid] += sq_s[tid + d];
        __syncthreads();
    }
    if (tid == 0 && ssw) ssw[blockIdx.x] = (double)(N - 2 * M) + 2.0 * sq_s[0];
}

// One (run, period) sum out of xr (global memory, or the run's copy in LDS): see the head of the file for the order.
template <class X>
__device__ __forceinline__ void fold_one(const X* xr, int N, int p, const Twiddle* __restrict__ tab, int lane, double* __restrict__ o) {
    const int P = p < 64 ? p * (64 / p) : p;
    double re = 0.0, im = 0.0;
    for (int j = lane; j < P; j += 64) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int n = j;
        for (; n + 3 * P < N; n += 4 * P) {
            a0 += xr[n];
            a1 += xr[n + P];
            a2 += xr[n + 2 * P];
            a3 += xr[n + 3 * P];
        }
        for (; n < N; n += P) a0 += xr[n];
        const double f = (a0 + a1) + (a2 + a3);
        const Twiddle tw = tab[j % p];
        re += f * tw.c;
        im -= f * tw.s;
    }
    for (int d = 32; d; d >>= 1) {
        re += __shfl_xor(re, d);
        im += __shfl_xor(im, d);
    }
    if (lane == 0) {
        o[0] = re;
        o[1] = im;
    }
}

// STAGED: the runs of at most `limit` samples, copied to LDS once per workgroup and read from there by every period of
// the workgroup's chunk; else the longer runs, read from memory.  A workgroup whose run is the other kernel's leaves.
template <bool STAGED>
__global__ __launch_bounds__(STAGED ? kSpectrumStagedThreads : kSpecThreads) void spectrum_fold_kernel(
    const double* __restrict__ x, const int64_t* __restrict__ beg, const int64_t* __restrict__ end, const int32_t* __restrict__ periods,
    const int32_t* __restrict__ tab_off, const Twiddle* __restrict__ table, int n_per, int chunks, int per_block, int limit,
    double* __restrict__ out) {
    extern __shared__ double spectrum_x_s[];
    const int lane = threadIdx.x & 63, n_waves = blockDim.x >> 6;
    const long long r = blockIdx.x / (unsigned)chunks;
    const int k0 = (int)(blockIdx.x % (unsigned)chunks) * per_block, k1 = min(n_per, k0 + per_block);
    const long long a = beg[r];
    const int N = (int)(end[r] - a);
    if ((N <= limit) != STAGED) return;  // (the whole workgroup)
    if constexpr (STAGED) {
        for (int n = threadIdx.x; n < N; n += blockDim.x) spectrum_x_s[n] = x[a + n];  // N <= limit: within the launch's LDS
        __syncthreads();
    }
    for (int k = k0 + (threadIdx.x >> 6); k < k1; k += n_waves) {  // (a wave's lanes share k: the shuffles see all 64)
        double* o = out + (r * n_per + k) * 2;
        if constexpr (STAGED) fold_one(spectrum_x_s, N, periods[k], table + tab_off[k], lane, o);
        else fold_one(x + a, N, periods[k], table + tab_off[k], lane, o);
    }
}

}  // namespace

void launch_spectrum_twiddles(hipStream_t s, const int32_t* periods, const int32_t* tab_off, int n_per, Twiddle* table) {
    hipLaunchKernelGGL(spectrum_twiddle_kernel, dim3((unsigned)n_per), dim3(256), 0, s, periods, tab_off, table);
}

void launch_spectrum_prep(hipStream_t s, const int64_t* v, const int64_t* beg, const int64_t* end, long long n_runs, double taper,
                          int detrend, double* x, double* ssw, int* bad) {
    hipLaunchKernelGGL(spectrum_prep_kernel, dim3((unsigned)n_runs), dim3(256), 0, s, v, beg, end, taper, detrend, x, ssw, bad);
}

hipError_t spectrum_lds_samples(int device, int* samples_out) {
    int limit = 0;
    hipError_t e = hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device);
    if (e != hipSuccess) return e;
    const int samples = std::min(kSpectrumLdsSamples, limit / 8);
    if (samples * 8 > (64 << 10) &&
        (e = hipFuncSetAttribute(reinterpret_cast<const void*>(&spectrum_fold_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 samples * 8)) != hipSuccess)
        return e;
    *samples_out = samples;
    return hipSuccess;
}

void launch_spectrum_fold(hipStream_t s, const double* x, const int64_t* beg, const int64_t* end, long long n_runs,
                          const int32_t* periods, const int32_t* tab_off, const Twiddle* table, int n_per, int limit, int longest_staged,
                          bool any_longer, double* out) {
    if (longest_staged >= 0) {
        const int chunks = spectrum_chunks(n_per, kSpectrumStagedPeriods);
        hipLaunchKernelGGL(spectrum_fold_kernel<true>, dim3((unsigned)(n_runs * chunks)), dim3(kSpectrumStagedThreads),
                           (size_t)longest_staged * 8, s, x, beg, end, periods, tab_off, table, n_per, chunks, kSpectrumStagedPeriods, limit,
                           out);
    }
    if (any_longer) {
        const int chunks = spectrum_chunks(n_per, kSpectrumWaves);
        hipLaunchKernelGGL(spectrum_fold_kernel<false>, dim3((unsigned)(n_runs * chunks)), dim3(kSpecThreads), 0, s, x, beg, end, periods,
                           tab_off, table, n_per, chunks, kSpectrumWaves, limit, out);
    }
}

}  // namespace ftk
