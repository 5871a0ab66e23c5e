// Part of ftk_api.hip's translation unit (#included there, in this order: perbase, ref, comm, export) - per-base entry points: `ftk_wps*` (the narrow wire to the host, the merged feature + WPS launch, batches, intervals), `ftk_cleavage*`, `ftk_wps_adjust`, and their shared helpers (`ScoreOutput`, `open_wps_call`, `cleave_params`, `plan_interval_tiles`); buffers are bound through `Scratch` (ftk_api.hip).

// ---- per-base scores to the host on a narrow wire -------------------------------------------------------------------
// The reference's WPS is int64 per base (frag/_wps.py:176-188): 2 GB for chr1, 24.8 GB for a genome - and a device -> host
// copy of it runs at the link's 55 GB/s whatever the kernels do (0.45 s of the 0.54 s a genome's every-feature run takes).
// The VALUES are small (a score is bounded by the fragments over a base: a few hundred at 60x), so they cross the link
// as int16 - a quarter of the bytes - and the host threads widen them into the caller's int64 array while the next
// chunk is on its way.  A score that does not fit (checked on the device, before anything is copied) sends the whole
// result the plain way.  FTK_WPS_NARROW_WIRE=0 keeps the plain copy.
namespace {
constexpr int64_t kNarrowChunk = int64_t(1) << 24;     // scores per chunk (32 MB on the wire, 128 MB widened)
constexpr int64_t kNarrowMin = int64_t(1) << 22;       // shorter results take the plain copy

__global__ __launch_bounds__(256) void narrow_i16_kernel(const int64_t* __restrict__ in, int16_t* __restrict__ out, int64_t n,
                                                         int* __restrict__ misfit) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 8;
    bool bad = false;
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8; i < n; i += stride) {
        if (i + 8 <= n) {
            typedef long long ll2 __attribute__((ext_vector_type(2)));
            const ll2* p = reinterpret_cast<const ll2*>(in + i);  // (in and out are 16-byte aligned, i % 8 == 0)
            long long v[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const ll2 t = __builtin_nontemporal_load(p + k);
                v[2 * k] = t.x;
                v[2 * k + 1] = t.y;
            }
            unsigned w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                bad |= v[2 * k] != (long long)(short)v[2 * k] || v[2 * k + 1] != (long long)(short)v[2 * k + 1];
                w[k] = ((unsigned)v[2 * k] & 0xffffu) | ((unsigned)v[2 * k + 1] << 16);
            }
            *reinterpret_cast<uint4*>(out + i) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            for (int64_t j = i; j < n; ++j) {
                const long long v = in[j];
                bad |= v != (long long)(short)v;
                out[j] = (int16_t)v;
            }
        }
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(misfit, 1);
}

#if defined(__x86_64__)
__attribute__((target("avx2"))) void widen_avx2(const int16_t* src, int64_t* dst, size_t a, size_t b) {
    size_t i = a;
    for (; i < b && ((uintptr_t)(dst + i) & 31u); ++i) dst[i] = src[i];
    for (; i + 16 <= b; i += 16) {  // 16 scores: one 32-byte load, four sign extensions, four streaming stores
        const __m256i v = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + i));
        const __m128i lo = _mm256_castsi256_si128(v), hi = _mm256_extracti128_si256(v, 1);
        _mm256_stream_si256(reinterpret_cast<__m256i*>(dst + i), _mm256_cvtepi16_epi64(lo));
        _mm256_stream_si256(reinterpret_cast<__m256i*>(dst + i + 4), _mm256_cvtepi16_epi64(_mm_srli_si128(lo, 8)));
        _mm256_stream_si256(reinterpret_cast<__m256i*>(dst + i + 8), _mm256_cvtepi16_epi64(hi));
        _mm256_stream_si256(reinterpret_cast<__m256i*>(dst + i + 12), _mm256_cvtepi16_epi64(_mm_srli_si128(hi, 8)));
    }
    for (; i < b; ++i) dst[i] = src[i];
    _mm_sfence();
}

#endif

void widen_i16(const int16_t* src, int64_t* dst, size_t n, int nt) {
#if defined(__x86_64__)
    static const bool avx2 = __builtin_cpu_supports("avx2");
#endif
    nt = std::max(1, std::min(nt, (int)(n >> 18) + 1));
    ftk_host::parallel_run_results(nt, [&](int t) {
        const size_t a = n * (size_t)t / (size_t)nt, b = n * (size_t)(t + 1) / (size_t)nt;
#if defined(__x86_64__)
        if (avx2) { widen_avx2(src, dst, a, b); return; }
#endif
        for (size_t i = a; i < b; ++i) dst[i] = src[i];
    });
}

// d_scores[0, n) (device, int64, complete on ctx->stream) -> host_out[0, n); FTK_OK, or a HIP error.  *done = false:
// nothing was copied (scores that do not fit 16 bits, no page-locked staging): the caller copies the plain way.
int copy_scores_narrow(ftk_ctx* ctx, const int64_t* d_scores, int16_t* d_narrow, int* d_misfit, int64_t n, int64_t* host_out,
                       bool* done) {
    *done = false;
    for (int k = 0; k < 2; ++k) {
        // (page-locked blocks of the library's result cache: a ctx that is destroyed hands them back and the next one
        // finds them there - pinning 64 MB anew for every engine cost the small file legs 4-5 ms)
        if (!ctx->narrow_stage[k] && ftk_host_alloc(kNarrowChunk * 2, &ctx->narrow_stage[k]) != FTK_OK) {
            ctx->narrow_stage[k] = nullptr;
            return FTK_OK;
        }
        if (!ctx->narrow_done[k]) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->narrow_done[k], hipEventDisableTiming));
    }
    HIPCHK(ctx, hipMemsetAsync(d_misfit, 0, sizeof(int), ctx->stream));
    const int blocks = (int)std::min<int64_t>((n / 8 + 255) / 256 + 1, 8192);
    hipLaunchKernelGGL(narrow_i16_kernel, dim3(blocks), dim3(256), 0, ctx->stream, d_scores, d_narrow, n, d_misfit);
    HIPCHK(ctx, hipGetLastError());
    int misfit = 0;
    HIPCHK(ctx, hipMemcpyAsync(&misfit, d_misfit, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (misfit) return FTK_OK;
    // FTK_WPS_TIMING=<ms>: a call that takes longer says where (stderr) - kernels, waits for chunks, widening
    static const double slow_ms = getenv("FTK_WPS_TIMING") ? atof(getenv("FTK_WPS_TIMING")) : 0.0;
    const auto t_start = std::chrono::steady_clock::now();
    auto ms_since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    double t_wait = 0, t_widen = 0, widen_max = 0;
    const int nt = ftk_host::default_threads();
    const int64_t n_chunks = (n + kNarrowChunk - 1) / kNarrowChunk;
    // (Four staging chunks with three copies in flight were measured: the copy engine then never idles - waits 65 -> 15 ms
    // per genome - but the threads widen a third slower beside it, 113 -> 165 ms: the host's memory is the shared
    // resource, and the leg got no faster.)
    for (int64_t c = 0; c <= n_chunks; ++c) {
        if (c < n_chunks) {  // chunk c on its way (its staging buffer's previous chunk, c - 2, was widened in the last turn)
            const int64_t a = c * kNarrowChunk, m = std::min(kNarrowChunk, n - a);
            HIPCHK(ctx, hipMemcpyAsync(ctx->narrow_stage[c & 1], d_narrow + a, (size_t)m * 2, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipEventRecord(ctx->narrow_done[c & 1], ctx->stream));
        }
        if (c > 0) {  // ... while the host threads widen chunk c - 1
            const int64_t a = (c - 1) * kNarrowChunk, m = std::min(kNarrowChunk, n - a);
            const auto t0 = std::chrono::steady_clock::now();
            HIPCHK(ctx, hipEventSynchronize(ctx->narrow_done[(c - 1) & 1]));
            const auto t1 = std::chrono::steady_clock::now();
            widen_i16(static_cast<const int16_t*>(ctx->narrow_stage[(c - 1) & 1]), host_out + a, (size_t)m, nt);
            const double w = ms_since(t1);
            t_wait += std::chrono::duration<double, std::milli>(t1 - t0).count();
            t_widen += w;
            widen_max = std::max(widen_max, w);
        }
    }
    if (slow_ms > 0 && ms_since(t_start) > slow_ms)
        fprintf(stderr, "[ftk_wps] narrow copy of %lld scores: %.1f ms (waiting for chunks %.1f, widening %.1f - slowest of %lld chunks %.1f - on %d threads)\n",
                (long long)n, ms_since(t_start), t_wait, t_widen, (long long)n_chunks, widen_max, nt);
    *done = true;
    return FTK_OK;
}

// Whole-interval scores and their way into host memory (ftk_wps, ftk_window_features_wps).  Declared first on a Scratch,
// host-bound scores sit at its base as wide | narrow | misfit; to_host() sends them on the narrow wire when that is on
// and they fit, the plain way otherwise.  Scores the caller wants on the device need neither.
struct ScoreOutput {
    int64_t *user = nullptr, *d_wide = nullptr, n_pos = 0;
    int16_t* d_narrow = nullptr;
    int* d_misfit = nullptr;
    bool host = false, narrow = false;
    void declare(Scratch& s, int64_t* wps_out, int64_t n) {
        static const bool narrow_env = !(getenv("FTK_WPS_NARROW_WIRE") && atoi(getenv("FTK_WPS_NARROW_WIRE")) == 0);
        user = wps_out, n_pos = n;
        host = s.out(&d_wide, wps_out, n, /*copy_back=*/false);
        narrow = host && narrow_env && n >= kNarrowMin;
        if (narrow) {
            s.tmp(&d_narrow, n);
            s.tmp(&d_misfit, 1);
        }
    }
    int to_host(ftk_ctx* ctx) const {
        if (!host) return FTK_OK;
        bool done = false;
        int rc;
        if (narrow && (rc = copy_scores_narrow(ctx, d_wide, d_narrow, d_misfit, n_pos, user, &done))) return rc;
        if (!done) {
            HIPCHK(ctx, hipMemcpyAsync(user, d_wide, (size_t)n_pos * 8, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
        return FTK_OK;
    }
};

// the opening of the per-base WPS entry points: the ctx, its contig, the WPS parameters
int open_wps_call(ftk_ctx* ctx, int contig_id, int64_t chrom_size, int32_t window_size, int32_t min_len, int32_t max_len,
                  int32_t mapq_min, ContigData** c, WpsParams* p) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    int rc = get_contig(ctx, contig_id, c);
    return rc ? rc : wps_params(ctx, **c, chrom_size, window_size, min_len, max_len, mapq_min, p);
}

CleaveParams cleave_params(const ContigData& c, int32_t min_len, int32_t max_len, int32_t mapq_min) {
    CleaveParams p{};
    p.min_len = min_len < 0 ? INT32_MIN : min_len;
    p.max_len = max_len < 0 ? INT32_MAX : max_len;
    p.mapq_min = mapq_min;
    p.lmax = std::max(0, max_len < 0 ? c.max_len : std::min(max_len, c.max_len));
    return p;
}

// Many intervals of one contig as ONE launch: per interval its start, stop and output offset, per tile its interval and
// its number within that (ftk_wps_intervals, ftk_cleavage_intervals).
struct TilePlan {
    int64_t *d_s = nullptr, *d_e = nullptr, *d_o = nullptr;
    int32_t *d_ti = nullptr, *d_tk = nullptr;
    int64_t n_tiles = 0, total_out = 0;
    std::vector<int32_t> tile_iv, tile_k;  // pageable staging of the uploads: the caller's finish(true) waits for them
};

// Checks the arguments (an interval may start at `lowest`), builds the plan, binds it and the output - *d_out: `out` or
// its stand-in in the scratch, for s.finish() to copy back - and uploads it.  FTK_OK with n_tiles == 0: nothing to do.
extern "C++" {  // (a template, in a file that is included inside ftk_api.hip's extern "C" block)
template <class T>
int plan_interval_tiles(ftk_ctx* ctx, Scratch& s, const int64_t* iv_start, const int64_t* iv_stop, int64_t n_iv,
                        const int64_t* out_offset, int64_t lowest, const char* tiles_name, T* out, T** d_out, TilePlan* tp) {
    if (n_iv < 0 || n_iv > INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "n_iv out of range");
    if (n_iv == 0) return FTK_OK;
    if (!iv_start || !iv_stop || !out_offset || !out) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    if (is_device_ptr(iv_start) || is_device_ptr(iv_stop) || is_device_ptr(out_offset))
        return fail(ctx, FTK_ERR_INVALID, "interval arrays must be host arrays");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (int64_t i = 0; i < n_iv; ++i) {
        const int64_t len = iv_stop[i] - iv_start[i];
        if (len <= 0) continue;
        if (iv_start[i] < lowest || iv_stop[i] > (1LL << 31)) return fail(ctx, FTK_ERR_INVALID, "interval out of range");
        if (out_offset[i] < 0) return fail(ctx, FTK_ERR_INVALID, "negative output offset");
        tp->total_out = std::max(tp->total_out, out_offset[i] + len);
        for (int64_t k = 0; k < (len + kWpsTile - 1) / kWpsTile; ++k) {
            tp->tile_iv.push_back((int32_t)i);
            tp->tile_k.push_back((int32_t)k);
        }
    }
    const size_t n_tiles = tp->tile_iv.size();
    if (n_tiles == 0) return FTK_OK;
    if (n_tiles > (size_t)INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "too many %s in one call", tiles_name);
    s.tmp(&tp->d_s, n_iv);
    s.tmp(&tp->d_e, n_iv);
    s.tmp(&tp->d_o, n_iv);
    s.tmp(&tp->d_ti, n_tiles);
    s.tmp(&tp->d_tk, n_tiles);
    s.out(d_out, out, tp->total_out);
    int rc = s.reserve();
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(tp->d_s, iv_start, n_iv * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(tp->d_e, iv_stop, n_iv * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(tp->d_o, out_offset, n_iv * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(tp->d_ti, tp->tile_iv.data(), n_tiles * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(tp->d_tk, tp->tile_k.data(), n_tiles * 4, hipMemcpyHostToDevice, ctx->stream));
    tp->n_tiles = (int64_t)n_tiles;
    return FTK_OK;
}
}  // extern "C++"

// The device half of ftk_wps_adjust over runs whose scores are already on the device: the tile lists of both kinds
// counted and filled from the run offsets, the running median (or mean) and the Savitzky-Golay pass.  The caller
// validates the runs, declares the buffers in its own Scratch and owns every copy; ftk_wps_peaks runs it batch after
// batch on scores that never leave the device.
struct AdjustChain {
    int W = 0, tile = 0;
    bool fast = false;  // the histogram median in front of the sort kernel
    int64_t n_iv = 0;
    AdjustTile *d_tiles = nullptr, *d_fast = nullptr;
    int *d_todo = nullptr, *d_pre0 = nullptr, *d_pre1 = nullptr;
    int64_t* d_offs = nullptr;

    // at most n_iv runs with total_out outputs between them (of any one launch of the call)
    void declare(Scratch& s, int64_t n_iv_, int W_, bool use_mean, int64_t total_out) {
        // FTK_ADJUST_HIST=0: every interval through the sort kernel (the tests hold the two medians together)
        static const bool use_hist = !(getenv("FTK_ADJUST_HIST") && atoi(getenv("FTK_ADJUST_HIST")) == 0);
        W = W_;
        n_iv = n_iv_;
        adjust_sort_size(W, &tile);
        fast = use_hist && !use_mean;
        s.tmp(&d_tiles, (size_t)tiles_ub(total_out));
        if (fast) {
            s.tmp(&d_fast, (size_t)(total_out / kAdjustFastTile + n_iv));
            s.tmp(&d_todo, (size_t)n_iv + 2);
        }
        s.tmp(&d_offs, (size_t)n_iv + 1);
        s.tmp(&d_pre0, (size_t)n_iv + 1);
        s.tmp(&d_pre1, (size_t)n_iv + 1);
    }
    int64_t tiles_ub(int64_t total_out) const { return total_out / tile + n_iv; }
    // the tiles of a run of len scores, added to *n_tiles / *n_fast
    void count(int64_t len, int64_t* n_tiles, int64_t* n_fast) const {
        const int64_t m = len - W;
        *n_tiles += (m + tile - 1) / tile;
        if (fast) *n_fast += (m + kAdjustFastTile - 1) / kAdjustFastTile;
    }
    // offs_src: n + 1 run offsets in device-readable memory.  Touches nothing but the chain's own arrays whatever they hold.
    void counts(hipStream_t st, const int64_t* offs_src, int64_t n) const {
        launch_adjust_tile_counts(st, offs_src, d_offs, (int)n, W, tile, fast ? kAdjustFastTile : 0, d_pre0, d_pre1, d_todo);
    }
    // behind counts(), for the same n runs: their n_tiles / n_fast tiles filled, d_in filtered into d_adj and, with sw, that
    // smoothed into d_out
    void run(hipStream_t st, int64_t n, int64_t n_tiles, int64_t n_fast, const double* d_in, const double* d_sub, int use_mean,
             double* d_adj, int sw, const double* d_coef, const double* d_edge, double* d_out) const {
        AdjustTile* fast_tiles = n_fast ? d_fast : nullptr;
        int* todo = n_fast ? d_todo : nullptr;
        launch_adjust_tile_fill(st, d_offs, (int)n, W, tile, n_fast ? kAdjustFastTile : 0, d_pre0, d_pre1, d_tiles, (int)n_tiles,
                                fast_tiles, (int)n_fast);
        launch_adjust_filter(st, d_in, d_tiles, (int)n_tiles, d_sub, W, use_mean, d_adj, fast_tiles, (int)n_fast, todo, (int)n);
        if (sw) launch_savgol(st, d_adj, d_tiles, (int)n_tiles, d_coef, d_edge, sw, d_out);
    }
};
}  // namespace

int ftk_wps(ftk_ctx* ctx, int contig_id, int64_t start, int64_t stop, int64_t chrom_size, int32_t window_size,
            int32_t min_len, int32_t max_len, int32_t mapq_min, int64_t* wps_out) {
    ContigData* c;
    WpsParams p{};
    int rc = open_wps_call(ctx, contig_id, chrom_size, window_size, min_len, max_len, mapq_min, &c, &p);
    if (rc) return rc;
    if (stop <= start) return FTK_OK;  // degenerate interval: empty result (frag/_wps.py:145-152)
    if (start < -(1LL << 30) || stop > (1LL << 31)) return fail(ctx, FTK_ERR_INVALID, "interval out of range");
    if (!wps_out) return fail(ctx, FTK_ERR_INVALID, "wps_out is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t n_pos = stop - start;
    static const double slow_ms = getenv("FTK_WPS_TIMING") ? atof(getenv("FTK_WPS_TIMING")) : 0.0;
    const auto t_call = std::chrono::steady_clock::now();
    struct Slow {
        double limit;
        std::chrono::steady_clock::time_point t0;
        long long n;
        double reserve_ms = 0, kernel_ms = 0;
        ~Slow() {
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (limit > 0 && ms > limit)
                fprintf(stderr, "[ftk_wps] %lld positions: %.1f ms (scratch %.1f, launch %.1f)\n", n, ms, reserve_ms, kernel_ms);
        }
    } slow{slow_ms, t_call, (long long)n_pos};
    ScoreOutput so;
    Scratch s(ctx);
    so.declare(s, wps_out, n_pos);
    if ((rc = s.reserve())) return rc;
    slow.reserve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    p.start = start;
    p.stop = stop;
    const int64_t n_tiles = (n_pos + kWpsTile - 1) / kWpsTile;
    launch_wps(ctx->stream, c->v, p, n_tiles, nullptr, nullptr, nullptr, nullptr, nullptr, so.d_wide);
    HIPCHK(ctx, hipGetLastError());
    slow.kernel_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count() - slow.reserve_ms;
    return so.to_host(ctx);
}

// ftk_window_features followed by ftk_wps on the same contig, as ONE launch when the request takes the FAST block
// path (grid = the feature blocks, then the WPS tiles: feat_then_wps_kernel); otherwise the two launches.
int ftk_window_features_wps(ftk_ctx* ctx, int contig_id, const int32_t* w_start, const int32_t* w_end, int64_t n_win,
                            const ftk_filter* f, int64_t* count_out, int32_t len_lo, int32_t n_bins, uint32_t* hist_out,
                            int64_t* overflow_out, int32_t delfi_mapq_min, const int32_t* bl_start, const int32_t* bl_end,
                            int64_t n_bl, const ftk_gaps* gaps, int64_t* short_out, int64_t* long_out, int64_t start,
                            int64_t stop, int64_t chrom_size, int32_t window_size, int32_t min_len, int32_t max_len,
                            int32_t mapq_min, int64_t* wps_out) {
    ContigData* c;
    WpsTail tail{};
    int rc = open_wps_call(ctx, contig_id, chrom_size, window_size, min_len, max_len, mapq_min, &c, &tail.p);
    if (rc) return rc;
    const bool wps_ok = stop > start && start >= -(1LL << 30) && stop <= (1LL << 31) && wps_out && n_win > 0;
    // scores bound for host memory: the merged launch writes them to the head of the ctx scratch - the prefix that
    // features_common reserves in front of its own buffers - and they cross the link like ftk_wps' (ScoreOutput)
    ScoreOutput so;
    Scratch head(ctx);
    if (wps_ok) so.declare(head, wps_out, stop - start);
    FeatCall fc;
    every_feature_call(&fc, f, count_out, len_lo, n_bins, hist_out, overflow_out, delfi_mapq_min, bl_start, bl_end, n_bl, gaps,
                       short_out, long_out);
    bool merged = false;
    if (wps_ok) {
        tail.p.start = start;
        tail.p.stop = stop;
        tail.n_tiles = (stop - start + kWpsTile - 1) / kWpsTile;
        tail.out = wps_out;  // (host scores: replaced by the scratch base inside features_common)
    }
    if ((rc = features_common(ctx, contig_id, w_start, w_end, n_win, fc, wps_ok ? &tail : nullptr, &merged, head.bytes()))) return rc;
    if (!merged) return ftk_wps(ctx, contig_id, start, stop, chrom_size, window_size, min_len, max_len, mapq_min, wps_out);
    if ((rc = head.place())) return rc;
    return so.to_host(ctx);
}

int ftk_wps_async(ftk_ctx* ctx, int contig_id, int64_t start, int64_t stop, int64_t chrom_size, int32_t window_size,
                  int32_t min_len, int32_t max_len, int32_t mapq_min, int64_t* wps_out_host, int* token_out) {
    ContigData* c;
    WpsParams p{};
    int rc = open_wps_call(ctx, contig_id, chrom_size, window_size, min_len, max_len, mapq_min, &c, &p);
    if (rc) return rc;
    if (!token_out) return fail(ctx, FTK_ERR_INVALID, "token_out is NULL");
    *token_out = -1;
    if (stop <= start) return FTK_OK;  // degenerate interval: empty result, nothing to wait for
    if (start < -(1LL << 30) || stop > (1LL << 31)) return fail(ctx, FTK_ERR_INVALID, "interval out of range");
    if (!wps_out_host || is_device_ptr(wps_out_host)) return fail(ctx, FTK_ERR_INVALID, "wps_out_host must be a host array");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!ctx->copy_stream) {
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) {
            HIPCHK(ctx, hipEventCreateWithFlags(&ctx->a_kernel_done[k], hipEventDisableTiming));
            HIPCHK(ctx, hipEventCreateWithFlags(&ctx->a_copy_done[k], hipEventDisableTiming));
        }
    }
    const int k = ctx->a_issued & 1;  // tokens count up; a token's buffer is its lowest bit
    if (ctx->a_pending[k]) {  // the buffer's previous result is still on its way to the host
        HIPCHK(ctx, hipEventSynchronize(ctx->a_copy_done[k]));
        ctx->a_pending[k] = false;
    }
    const int64_t n_pos = stop - start;
    const size_t need = align_up((size_t)n_pos * 8);
    if (need > ctx->abuf_bytes[k]) {
        if (ctx->abuf[k]) HIPCHK(ctx, hipFree(ctx->abuf[k]));
        ctx->abuf[k] = nullptr;
        ctx->abuf_bytes[k] = 0;
        HIPCHK(ctx, hipMalloc(&ctx->abuf[k], need));
        ctx->abuf_bytes[k] = need;
    }
    p.start = start;
    p.stop = stop;
    const int64_t n_tiles = (n_pos + kWpsTile - 1) / kWpsTile;
    launch_wps(ctx->stream, c->v, p, n_tiles, nullptr, nullptr, nullptr, nullptr, nullptr, (int64_t*)ctx->abuf[k]);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ctx->a_kernel_done[k], ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->a_kernel_done[k], 0));
    HIPCHK(ctx, hipMemcpyAsync(wps_out_host, ctx->abuf[k], (size_t)n_pos * 8, hipMemcpyDeviceToHost, ctx->copy_stream));
    HIPCHK(ctx, hipEventRecord(ctx->a_copy_done[k], ctx->copy_stream));
    ctx->a_pending[k] = true;
    ctx->a_token[k] = ctx->a_issued;
    *token_out = ctx->a_issued;
    ctx->a_issued = ctx->a_issued == INT32_MAX ? (ctx->a_issued & 1) ^ 1 : ctx->a_issued + 1;  // (wraps with the parity kept)
    return FTK_OK;
}

int ftk_result_wait(ftk_ctx* ctx, int token) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (token < 0) return FTK_OK;  // an empty result
    const int k = token & 1;
    if (ctx->a_token[k] < 0 || (ctx->a_token[k] != token && ctx->a_token[1 - k] != token && token >= ctx->a_issued))
        return fail(ctx, FTK_ERR_INVALID, "result token %d was never handed out", token);
    // a token older than the one in its buffer names a result that is complete: the call that reused the buffer waited
    // for its copy first
    if (ctx->a_token[k] == token && ctx->a_pending[k]) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        HIPCHK(ctx, hipEventSynchronize(ctx->a_copy_done[k]));
        ctx->a_pending[k] = false;
    }
    return FTK_OK;
}

int ftk_wps_intervals(ftk_ctx* ctx, int contig_id, const int64_t* iv_start, const int64_t* iv_stop, int64_t n_iv,
                      const int64_t* out_offset, int64_t chrom_size, int32_t window_size, int32_t min_len,
                      int32_t max_len, int32_t mapq_min, int64_t* wps_out) {
    ContigData* c;
    WpsParams p{};
    int rc = open_wps_call(ctx, contig_id, chrom_size, window_size, min_len, max_len, mapq_min, &c, &p);
    if (rc) return rc;
    Scratch s(ctx);
    TilePlan tp;
    int64_t* d_out = nullptr;
    if ((rc = plan_interval_tiles(ctx, s, iv_start, iv_stop, n_iv, out_offset, -(1LL << 30), "WPS tiles", wps_out, &d_out, &tp)))
        return rc;
    if (tp.n_tiles == 0) return FTK_OK;
    launch_wps(ctx->stream, c->v, p, tp.n_tiles, tp.d_s, tp.d_e, tp.d_o, tp.d_ti, tp.d_tk, d_out);
    HIPCHK(ctx, hipGetLastError());
    return s.finish(/*must_sync=*/true);  // (the plan's tile vectors are pageable staging)
}

int ftk_wps_window_features(ftk_ctx* ctx, int contig_id, int64_t start, int64_t stop, int64_t chrom_size,
                            int32_t window_size, int32_t min_len, int32_t max_len, int32_t mapq_min, int64_t* wps_out,
                            int32_t win_start, int32_t win_len, int32_t n_win, const ftk_filter* f, int64_t* count_out,
                            int32_t len_lo, int32_t n_bins, uint32_t* hist_out, int64_t* overflow_out,
                            int32_t delfi_mapq_min, const int32_t* bl_start, const int32_t* bl_end, int64_t n_bl,
                            const ftk_gaps* gaps, int64_t* short_out, int64_t* long_out) {
    ContigData* c;
    WpsParams p{};
    int rc = open_wps_call(ctx, contig_id, chrom_size, window_size, min_len, max_len, mapq_min, &c, &p);
    if (rc) return rc;
    const bool ch = count_out || hist_out, df = short_out || long_out;
    if (!wps_out || (!ch && !df)) return fail(ctx, FTK_ERR_INVALID, "needs wps_out and at least one feature output");
    if (ch && (!f || f->policy != FTK_POLICY_MIDPOINT))
        return fail(ctx, FTK_ERR_INVALID, "the fused pass needs a midpoint-policy filter");
    if (ch && (rc = check_filter(ctx, f, *c))) return rc;
    // fetch semantics as everywhere else: read1 overlap (io/alignment.py:245) on a contig with read1 columns unless
    // the filter asks for the tabix rule
    const bool bam = c->v.r1_start != nullptr && (!ch || f->fetch_mode == FTK_FETCH_BAM_READ1);
    // (8192: this pass's own histogram limit, below kHistMaxBins)
    if ((rc = check_delfi_hist_outputs(ctx, short_out, long_out, hist_out, n_bins, 8192, overflow_out))) return rc;
    if (n_win <= 0 || win_start < 0 || win_len < kWpsTile + c->max_len || (int64_t)win_start + (int64_t)n_win * win_len > (1LL << 31))
        return fail(ctx, FTK_ERR_INVALID, "bins must be at least %d bp long (tile + longest fragment) and end below 2^31",
                    kWpsTile + c->max_len);
    if (start > 0 || stop < (int64_t)c->max_end || stop <= start)
        return fail(ctx, FTK_ERR_INVALID, "the WPS interval must cover every fragment of the contig (start <= 0, stop >= %d)",
                    c->max_end);
    if (start < -(1LL << 30) || stop > (1LL << 31)) return fail(ctx, FTK_ERR_INVALID, "interval out of range");
    if (bad_blacklist(n_bl, bl_start, bl_end) || is_device_ptr(bl_start))
        return fail(ctx, FTK_ERR_INVALID, "bad blacklist arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    FusedParams F{};
    F.win_start = win_start;
    F.win_len = win_len;
    F.n_win = n_win;
    F.bam = bam;
    if (ch) {
        F.ch_q = std::min(std::max(f->mapq_min, 0), 256);
        F.ch_min = f->min_len < 0 ? 0 : std::min(f->min_len, 1 << 30);
        F.ch_max = f->max_len < 0 ? (1 << 30) : std::min(f->max_len, 1 << 30);
    }
    F.do_cov = count_out != nullptr;
    F.do_hist = hist_out != nullptr;
    F.len_lo = len_lo;
    F.n_bins = n_bins;
    F.do_delfi = df;
    F.df_q = std::min(std::max(delfi_mapq_min, 0), 256);
    ftk_gaps g{};
    if ((rc = checked_gaps(ctx, gaps, -1, &g))) return rc;
    set_gap_constants(g, &F);
    if (df && n_bl > 0) {  // per-bin blacklist CSR, cached like ftk_delfi_counts' (same key: the bins' arrays)
        std::vector<int32_t> ws(n_win), we(n_win);
        for (int k = 0; k < n_win; ++k) { ws[k] = win_start + k * win_len; we[k] = ws[k] + win_len; }
        DelfiMeta* meta = nullptr;
        if ((rc = get_delfi_meta(ctx, contig_id, ws.data(), we.data(), n_win, bl_start, bl_end, n_bl, &meta))) return rc;
        if (meta->n_r) { F.bl_off = meta->d_off; F.bl_r0 = meta->d_r0; F.bl_pm = meta->d_pm; }
    }
    const int64_t n_pos = stop - start;
    const size_t hist_elems = hist_out ? (size_t)n_win * (size_t)n_bins : 0;
    int64_t* d_wps = nullptr;
    Scratch s(ctx);
    s.out(&d_wps, wps_out, n_pos);
    declare_feature_outputs(s, &F, n_win, hist_elems, hist_out != nullptr, count_out, hist_out, overflow_out, short_out, long_out);
    if ((rc = s.reserve())) return rc;
    // every feature output is accumulated with atomics: start from zero
    if (F.cov_out) HIPCHK(ctx, hipMemsetAsync(F.cov_out, 0, (size_t)n_win * 8, ctx->stream));
    if (F.hist_out) {
        HIPCHK(ctx, hipMemsetAsync(F.hist_out, 0, hist_elems * 4, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(F.over_out, 0, (size_t)n_win * 8, ctx->stream));
    }
    if (df) {
        HIPCHK(ctx, hipMemsetAsync(F.short_out, 0, (size_t)n_win * 8, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(F.long_out, 0, (size_t)n_win * 8, ctx->stream));
    }
    p.start = start;
    p.stop = stop;
    launch_wps_fused(ctx->stream, c->v, p, (n_pos + kWpsTile - 1) / kWpsTile, F, d_wps);
    HIPCHK(ctx, hipGetLastError());
    return s.finish();
}

int ftk_wps_batch(ftk_ctx* ctx, const int32_t* contig_ids, const int64_t* iv_start, const int64_t* iv_stop,
                  const int64_t* chrom_size, const int64_t* out_offset, int64_t n_iv, int32_t window_size,
                  int32_t min_len, int32_t max_len, int32_t mapq_min, int64_t* wps_out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (n_iv < 0 || n_iv > kBatchMaxItems) return fail(ctx, FTK_ERR_INVALID, "n_iv must be in [0, %d]", kBatchMaxItems);
    if (n_iv == 0) return FTK_OK;
    if (!contig_ids || !iv_start || !iv_stop || !chrom_size || !out_offset || !wps_out)
        return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    long long total_out = 0;
    std::vector<WpsItem> host;
    WpsParams p{};
    long long tiles = 0;
    for (int64_t i = 0; i < n_iv; ++i) {
        ContigData* c;
        int rc = get_contig(ctx, contig_ids[i], &c);
        if (rc) return rc;
        WpsParams pi{};
        if ((rc = wps_params(ctx, *c, chrom_size[i], window_size, min_len, max_len, mapq_min, &pi))) return rc;
        const long long len = iv_stop[i] - iv_start[i];
        if (len <= 0) continue;
        if (iv_start[i] < -(1LL << 30) || iv_stop[i] > (1LL << 31) || out_offset[i] < 0)
            return fail(ctx, FTK_ERR_INVALID, "interval %lld out of range", (long long)i);
        if (host.empty()) p = pi;
        if ((c->v.r1_start != nullptr) != (host.empty() ? c->v.r1_start != nullptr : host[0].cv.r1_start != nullptr))
            return fail(ctx, FTK_ERR_INVALID, "a batch cannot mix contigs with and without read1 columns");
        WpsItem it{};
        it.cv = c->v;
        it.start = iv_start[i];
        it.stop = iv_stop[i];
        it.chrom_size = chrom_size[i];
        it.out_off = out_offset[i];
        it.tile_base = tiles;
        it.lmax = pi.lmax;
        host.push_back(it);
        tiles += (len + kWpsTile - 1) / kWpsTile;
        total_out = std::max(total_out, (long long)out_offset[i] + len);
    }
    if (host.empty()) return FTK_OK;
    if (tiles > (long long)INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "too many tiles in one call");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    void* d_items = nullptr;
    int rc = upload_batch_descriptors(ctx, 1, host.data(), host.size() * sizeof(WpsItem), &d_items);
    if (rc) return rc;
    int64_t* d_out = nullptr;
    Scratch s(ctx);
    s.out(&d_out, wps_out, (size_t)total_out);
    if ((rc = s.reserve())) return rc;
    launch_wps_batch(ctx->stream, p, (const WpsItem*)d_items, (int)host.size(), tiles, d_out);
    HIPCHK(ctx, hipGetLastError());
    return s.finish();
}

int ftk_cleavage_intervals(ftk_ctx* ctx, int contig_id, const int64_t* iv_start, const int64_t* iv_stop, int64_t n_iv,
                           const int64_t* out_offset, int32_t min_len, int32_t max_len, int32_t mapq_min,
                           double* prop_out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    ContigData* c;
    int rc = get_contig(ctx, contig_id, &c);
    if (rc) return rc;
    Scratch s(ctx);
    TilePlan tp;
    double* d_out = nullptr;
    if ((rc = plan_interval_tiles(ctx, s, iv_start, iv_stop, n_iv, out_offset, 0, "tiles", prop_out, &d_out, &tp))) return rc;
    if (tp.n_tiles == 0) return FTK_OK;
    launch_cleavage(ctx->stream, c->v, cleave_params(*c, min_len, max_len, mapq_min), tp.n_tiles, tp.d_s, tp.d_e, tp.d_o, tp.d_ti,
                    tp.d_tk, d_out);
    HIPCHK(ctx, hipGetLastError());
    return s.finish(/*must_sync=*/true);  // (the plan's tile vectors are pageable staging)
}

int ftk_cleavage(ftk_ctx* ctx, int contig_id, int64_t start, int64_t stop, int32_t min_len, int32_t max_len,
                 int32_t mapq_min, double* prop_out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (stop <= start) return FTK_OK;
    ContigData* c;
    int rc = get_contig(ctx, contig_id, &c);
    if (rc) return rc;
    if (start < 0 || stop > (1LL << 31)) return fail(ctx, FTK_ERR_INVALID, "interval out of range");
    if (!prop_out) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // ONE interval: its tiles are numbered by the grid (no descriptor arrays to build and upload - for a whole contig
    // 60 000 tiles, half a megabyte of pageable staging and a stream synchronisation per call)
    CleaveParams p = cleave_params(*c, min_len, max_len, mapq_min);
    p.start = start;
    p.stop = stop;
    const int64_t n_pos = stop - start, n_tiles = (n_pos + kWpsTile - 1) / kWpsTile;
    double* d_out = nullptr;
    Scratch s(ctx);
    s.out(&d_out, prop_out, n_pos);
    if ((rc = s.reserve())) return rc;
    launch_cleavage(ctx->stream, c->v, p, n_tiles, nullptr, nullptr, nullptr, nullptr, nullptr, d_out);
    HIPCHK(ctx, hipGetLastError());
    return s.finish();
}

int ftk_wps_adjust(ftk_ctx* ctx, const double* scores, const int64_t* offsets, int64_t n_iv, int32_t median_window,
                   int use_mean, const double* edge_sub, int32_t savgol_window, const double* savgol_coef,
                   const double* savgol_edge, double* out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (n_iv < 0 || n_iv > INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "n_iv out of range");
    if (n_iv == 0) return FTK_OK;
    if (!scores || !offsets || !out) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    if (is_device_ptr(offsets) || is_device_ptr(edge_sub) || is_device_ptr(savgol_coef) ||
        is_device_ptr(savgol_edge))
        return fail(ctx, FTK_ERR_INVALID, "offsets / edge_sub / savgol arrays must be host arrays");
    const int W = median_window;
    if (W < 2 || (W & 1) || W > kAdjustMaxWindow)
        return fail(ctx, FTK_ERR_INVALID, "median_window must be even and in [2, %d]", kAdjustMaxWindow);
    const int sw = savgol_window;
    if (sw < 0 || (sw > 0 && (!(sw & 1) || !savgol_coef || !savgol_edge)))
        return fail(ctx, FTK_ERR_INVALID, "savgol_window must be odd and come with coef/edge arrays");
    // The tiles are counted here and BUILT on the device from the run offsets.  The device's half starts FIRST: the
    // offsets go into page-locked memory and the counting kernel out (it reads and writes nothing but its own arrays,
    // whatever the offsets hold), and the runs are checked on the host while it runs.
    const int64_t total_in = offsets[n_iv], total_out = total_in - n_iv * (int64_t)W;
    if (offsets[0] != 0 || total_out < 0)  // (some run is shorter than W, or the offsets do not start at 0: the loop below says which)
        for (int64_t i = 0; i < n_iv; ++i) {
            const int64_t len = offsets[i + 1] - offsets[i];
            if (offsets[i] < 0 || len < W)
                return fail(ctx, FTK_ERR_INVALID, "run %lld is shorter than median_window (%lld < %d)", (long long)i,
                            (long long)len, W);
        }
    if (total_out < 0 || total_in > (int64_t(1) << 40)) return fail(ctx, FTK_ERR_INVALID, "run offsets out of range");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool in_dev = is_device_ptr(scores);
    const int half = sw / 2;
    double *d_sub = nullptr, *d_coef = nullptr, *d_edge = nullptr, *d_staged = nullptr, *d_out = nullptr, *d_adj = nullptr;
    Scratch s(ctx);
    AdjustChain chain;
    chain.declare(s, n_iv, W, use_mean != 0, total_out);
    if (chain.tiles_ub(total_out) > INT32_MAX - 1024) return fail(ctx, FTK_ERR_INVALID, "too many tiles in one call");
    if (edge_sub) s.tmp(&d_sub, n_iv);
    if (sw) {
        s.tmp(&d_coef, sw);
        s.tmp(&d_edge, (size_t)2 * half * sw);
        s.tmp(&d_adj, total_out);
    }
    if (!in_dev) s.tmp(&d_staged, total_in);
    s.out(&d_out, out, total_out);
    int rc = s.reserve();
    if (rc) return rc;
    if (!sw) d_adj = d_out;
    {
        const size_t bytes = (size_t)(n_iv + 1) * 8;
        if (ctx->param_stage_bytes < bytes) {
            if (ctx->param_stage) (void)hipHostFree(ctx->param_stage);
            ctx->param_stage = nullptr;
            ctx->param_stage_bytes = 0;
            HIPCHK(ctx, hipHostMalloc(&ctx->param_stage, align_up(bytes + bytes / 2), hipHostMallocDefault));
            ctx->param_stage_bytes = align_up(bytes + bytes / 2);
        }
        memcpy(ctx->param_stage, offsets, bytes);  // (this call synchronises the stream before it returns)
        void* stage_dev = nullptr;  // the device's address of the page-locked block: the first kernel reads it in place
        HIPCHK(ctx, hipHostGetDevicePointer(&stage_dev, ctx->param_stage, 0));
        chain.counts(ctx->stream, (const int64_t*)stage_dev, n_iv);
    }
    int64_t n_tiles = 0, n_fast = 0;
    for (int64_t i = 0; i < n_iv; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        const int64_t m = len - W;
        const char* what = (offsets[i] < 0 || len < W) ? "shorter" : m > INT32_MAX ? "long" : (sw > 0 && m < sw) ? "savgol" : nullptr;
        if (what) {
            (void)hipStreamSynchronize(ctx->stream);  // (the counting kernel still reads the staged offsets)
            if (what[1] == 'h')
                return fail(ctx, FTK_ERR_INVALID, "run %lld is shorter than median_window (%lld < %d)", (long long)i,
                            (long long)len, W);
            if (what[0] == 'l') return fail(ctx, FTK_ERR_INVALID, "run %lld too long", (long long)i);
            return fail(ctx, FTK_ERR_INVALID, "run %lld: savgol_window (%d) exceeds the filtered length (%lld)",
                        (long long)i, sw, (long long)m);
        }
        chain.count(len, &n_tiles, &n_fast);
    }
    if (n_tiles == 0) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return FTK_OK;
    }
    const double* d_in = scores;
    if (!in_dev) {
        HIPCHK(ctx, hipMemcpyAsync(d_staged, scores, total_in * 8, hipMemcpyHostToDevice, ctx->stream));
        d_in = d_staged;
    }
    if (d_sub) HIPCHK(ctx, hipMemcpyAsync(d_sub, edge_sub, n_iv * 8, hipMemcpyHostToDevice, ctx->stream));
    if (sw) {
        HIPCHK(ctx, hipMemcpyAsync(d_coef, savgol_coef, (size_t)sw * 8, hipMemcpyHostToDevice, ctx->stream));
        if (half)
            HIPCHK(ctx, hipMemcpyAsync(d_edge, savgol_edge, (size_t)2 * half * sw * 8, hipMemcpyHostToDevice,
                                       ctx->stream));
    }
    chain.run(ctx->stream, n_iv, n_tiles, n_fast, d_in, d_sub, use_mean, d_adj, sw, d_coef, d_edge, d_out);
    HIPCHK(ctx, hipGetLastError());
    return s.finish(/*must_sync=*/true);  // (the coefficient arrays are pageable staging)
}
