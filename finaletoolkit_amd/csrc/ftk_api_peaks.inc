// Part of ftk_api.hip's translation unit (#included there behind the spectrum part) - nucleosome calls from float64 score
// runs (`ftk_track_peaks`) and from the adjusted WPS of intervals scored, adjusted and called in device scratch
// (`ftk_wps_peaks`) over the kernels of ftk_peaks.hip.  Both check their arguments, reserve room for the most regions
// and calls the runs can hold - so nothing waits for the device between the passes - and hand the calls back in library
// buffers (ftk_buffer_free); the fused call does so batch by batch of intervals, every batch in the same scratch.
#include "ftk_peaks.h"

namespace {

// The rule's side of one call: parameters, the mark pass's tiles of every batch, the device buffers, the way home.
struct PeaksCall {
    PeaksParams P{};
    PeaksBufs b{};
    std::vector<int32_t> tile_run, tile_k;  // batch after batch (pageable staging of the upload: finish() waits for the stream)
    std::vector<int64_t> batch_tile{0};
    int64_t reg_cap = 0, most_tiles = 0, n_runs = 0;
    int32_t *d_tile_run = nullptr, *d_tile_k = nullptr;

    int check(ftk_ctx* ctx, int64_t skip, int32_t max_gap, int32_t min_region, int32_t short_max, int32_t max_region) {
        if (skip < 0 || skip > INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "skip %lld out of range", (long long)skip);
        if (max_gap < 0 || max_gap > kPeaksMaxGap) return fail(ctx, FTK_ERR_INVALID, "max_gap %d out of range (0 .. %d)", max_gap, kPeaksMaxGap);
        if (!(1 <= min_region && min_region <= short_max && short_max <= max_region && max_region <= kPeaksMaxRegion))
            return fail(ctx, FTK_ERR_INVALID, "region lengths (%d, %d, %d) must satisfy 1 <= min_region <= short_max <= max_region <= %d",
                        min_region, short_max, max_region, kPeaksMaxRegion);
        P = PeaksParams{(int32_t)skip, max_gap, min_region, short_max, max_region};
        return FTK_OK;
    }
    // The next batch: n runs at rel[0 .. n] of its track.  Region starts lie max_gap + 2 apart and calls min_region + 1, which
    // bounds both by the runs' lengths.
    int add_batch(ftk_ctx* ctx, const int64_t* rel, int64_t n) {
        int64_t regions = 0;
        for (int64_t r = 0; r < n; ++r) {
            const int64_t len = rel[r + 1] - rel[r];
            for (int64_t k = 0; k < (len + kPeaksTile - 1) / kPeaksTile; ++k) {
                tile_run.push_back((int32_t)r);
                tile_k.push_back((int32_t)k);
            }
            regions += len / (P.max_gap + 2) + 1;
            b.out_cap += len / (P.min_region + 1) + 1;
        }
        const int64_t tiles = (int64_t)tile_run.size() - batch_tile.back();
        if (tiles > INT32_MAX - 1 || regions > INT32_MAX - 1 || b.out_cap > INT32_MAX - 1)
            return fail(ctx, FTK_ERR_INVALID, "too many positions in one call");
        batch_tile.push_back((int64_t)tile_run.size());
        reg_cap = std::max(reg_cap, regions);
        most_tiles = std::max(most_tiles, tiles);
        n_runs += n;
        return FTK_OK;
    }
    // stats: the caller's n_runs * 6 counters (host or device)
    void declare(Scratch& s, int64_t* stats) {
        b.reg_cap = reg_cap;
        s.tmp(&d_tile_run, tile_run.size());
        s.tmp(&d_tile_k, tile_k.size());
        s.tmp(&b.tile_cnt, (size_t)most_tiles + 1);
        s.tmp(&b.reg_start, (size_t)reg_cap);
        s.tmp(&b.reg_end, (size_t)reg_cap);
        s.tmp(&b.reg_run, (size_t)reg_cap);
        s.tmp(&b.reg_med, (size_t)reg_cap);
        s.tmp(&b.reg_cnt, (size_t)reg_cap + 1);
        s.out(&b.stats, stats, (size_t)n_runs * 6);
        s.tmp(&b.n_calls, 1);
        s.tmp(&b.bad, 1);
        s.tmp(&b.o_run, (size_t)b.out_cap);
        s.tmp(&b.o_start, (size_t)b.out_cap);
        s.tmp(&b.o_stop, (size_t)b.out_cap);
        s.tmp(&b.o_summit, (size_t)b.out_cap);
        s.tmp(&b.o_height, (size_t)b.out_cap);
        s.tmp(&b.o_area, (size_t)b.out_cap);
    }
    int upload(ftk_ctx* ctx) {
        HIPCHK(ctx, hipMemsetAsync(b.stats, 0, (size_t)n_runs * 6 * 8, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(b.n_calls, 0, 8, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(b.bad, 0, sizeof(int), ctx->stream));
        if (!tile_run.empty()) {
            HIPCHK(ctx, hipMemcpyAsync(d_tile_run, tile_run.data(), tile_run.size() * 4, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipMemcpyAsync(d_tile_k, tile_k.data(), tile_k.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        return FTK_OK;
    }
    // batch k: the n runs a[off[r], off[r + 1]) (device arrays), counted from run_base in the calls and the counters
    int launch(ftk_ctx* ctx, size_t k, const double* a, const int64_t* off, int64_t n, int64_t run_base) {
        PeaksBufs bk = b;
        bk.tile_run = d_tile_run + batch_tile[k];
        bk.tile_k = d_tile_k + batch_tile[k];
        launch_peaks(ctx->stream, a, off, (int)n, batch_tile[k + 1] - batch_tile[k], P, (int)run_base, bk);
        HIPCHK(ctx, hipGetLastError());
        return FTK_OK;
    }
    // Behind the last launch: waits for the stream, then carries the calls home in blocks of the library's.
    int finish(ftk_ctx* ctx, Scratch& s, int32_t** run, int64_t** start, int64_t** stop, int64_t** summit, double** height,
               double** area, int64_t* n_calls) {
        uint64_t n = 0;
        int bad = 0;
        HIPCHK(ctx, hipMemcpyAsync(&n, b.n_calls, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(&bad, b.bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        if (int rc = s.finish(true)) return rc;
        if (bad) return fail(ctx, FTK_ERR_INVALID, "a score is not finite");
        if (n > (uint64_t)b.out_cap) return fail(ctx, FTK_ERR_HIP, "the call count %llu is out of range", (unsigned long long)n);
        if (n == 0) return FTK_OK;
        static constexpr size_t kSize[6] = {4, 8, 8, 8, 8, 8};
        const void* dev[6] = {b.o_run, b.o_start, b.o_stop, b.o_summit, b.o_height, b.o_area};
        void** const out[6] = {(void**)run, (void**)start, (void**)stop, (void**)summit, (void**)height, (void**)area};
        HostCols<6> home{kSize};
        SyncOnExit wait{ctx};  // (always: copies into this frame's blocks may be in flight)
        if (!home.grow((int64_t)n)) return fail(ctx, FTK_ERR_OOM, "out of host memory");
        if (const hipError_t e = home.fetch(ctx->stream, dev, (int64_t)n)) {
            (void)hipGetLastError();
            return fail(ctx, FTK_ERR_HIP, "copy of the calls failed: %s", hipGetErrorString(e));
        }
        home.give(out, n_calls);
        return FTK_OK;
    }
};

int open_peaks_outputs(ftk_ctx* ctx, int32_t** run, int64_t** start, int64_t** stop, int64_t** summit, double** height,
                       double** area, int64_t* n_calls) {
    if (!run || !start || !stop || !summit || !height || !area || !n_calls) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    *run = nullptr;
    *start = *stop = *summit = nullptr;
    *height = *area = nullptr;
    *n_calls = 0;
    return FTK_OK;
}

}  // namespace

extern "C" {

int ftk_track_peaks(ftk_ctx* ctx, const double* scores, const int64_t* offsets, int64_t n_runs, int64_t skip, int32_t max_gap,
                    int32_t min_region, int32_t short_max, int32_t max_region, int32_t** run, int64_t** start, int64_t** stop,
                    int64_t** summit, double** height, double** area, int64_t* n_calls, int64_t* stats) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    int rc = open_peaks_outputs(ctx, run, start, stop, summit, height, area, n_calls);
    if (rc) return rc;
    PeaksCall pc;
    if ((rc = pc.check(ctx, skip, max_gap, min_region, short_max, max_region))) return rc;
    if (n_runs < 0 || n_runs > INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "n_runs out of range");
    if (n_runs == 0) return FTK_OK;
    if (!scores || !offsets || !stats) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    if (is_device_ptr(offsets)) return fail(ctx, FTK_ERR_INVALID, "offsets must be a host array");
    if (offsets[0] < 0) return fail(ctx, FTK_ERR_INVALID, "negative offset");
    std::vector<int64_t> rel((size_t)n_runs + 1);  // offsets from the first run's start (pageable staging)
    for (int64_t i = 0; i <= n_runs; ++i) {
        rel[i] = offsets[i] - offsets[0];
        if (i && offsets[i] < offsets[i - 1]) return fail(ctx, FTK_ERR_INVALID, "offsets decrease at run %lld", (long long)i - 1);
    }
    if ((rc = pc.add_batch(ctx, rel.data(), n_runs))) return rc;
    const size_t total = (size_t)rel[n_runs];
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool in_dev = is_device_ptr(scores);
    double* d_stage = nullptr;
    int64_t* d_rel = nullptr;
    Scratch s(ctx);
    if (!in_dev) s.tmp(&d_stage, total);
    s.tmp(&d_rel, (size_t)n_runs + 1);
    pc.declare(s, stats);
    if ((rc = s.reserve())) return rc;
    // From here on the stream may be reading this call's vectors: every way out waits for it first.
    auto enqueue = [&]() -> int {
        if (int e = pc.upload(ctx)) return e;
        HIPCHK(ctx, hipMemcpyAsync(d_rel, rel.data(), ((size_t)n_runs + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        const double* a = scores + offsets[0];
        if (!in_dev) {
            if (total) HIPCHK(ctx, hipMemcpyAsync(d_stage, a, total * 8, hipMemcpyHostToDevice, ctx->stream));
            a = d_stage;
        }
        return pc.launch(ctx, 0, a, d_rel, n_runs, 0);
    };
    if ((rc = enqueue()) || (rc = pc.finish(ctx, s, run, start, stop, summit, height, area, n_calls))) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

int ftk_wps_peaks(ftk_ctx* ctx, int contig_id, const int64_t* iv_start, const int64_t* iv_stop, int64_t n_iv, int64_t chrom_size,
                  int32_t window_size, int32_t min_len, int32_t max_len, int32_t mapq_min, int32_t median_window,
                  int32_t savgol_window, const double* savgol_coef, const double* savgol_edge, int32_t max_gap, int32_t min_region,
                  int32_t short_max, int32_t max_region, int64_t batch_bases, int32_t** run, int64_t** start, int64_t** stop,
                  int64_t** summit, double** height, double** area, int64_t* n_calls, int64_t* stats) {
    ContigData* c;
    WpsParams p{};
    int rc = open_wps_call(ctx, contig_id, chrom_size, window_size, min_len, max_len, mapq_min, &c, &p);
    if (rc) return rc;
    if ((rc = open_peaks_outputs(ctx, run, start, stop, summit, height, area, n_calls))) return rc;
    const int W = median_window, sw = savgol_window, half = sw / 2;
    if (W < 2 || (W & 1) || W > kAdjustMaxWindow)
        return fail(ctx, FTK_ERR_INVALID, "median_window must be even and in [2, %d]", kAdjustMaxWindow);
    if (sw < 0 || (sw > 0 && (!(sw & 1) || !savgol_coef || !savgol_edge)))
        return fail(ctx, FTK_ERR_INVALID, "savgol_window must be odd and come with coef/edge arrays");
    PeaksCall pc;
    if ((rc = pc.check(ctx, half, max_gap, min_region, short_max, max_region))) return rc;
    if (batch_bases < 0) return fail(ctx, FTK_ERR_INVALID, "negative batch_bases");
    if (n_iv < 0 || n_iv > INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "n_iv out of range");
    if (n_iv == 0) return FTK_OK;
    if (!iv_start || !iv_stop || !stats) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    if (is_device_ptr(iv_start) || is_device_ptr(iv_stop) || is_device_ptr(stats) || is_device_ptr(savgol_coef) || is_device_ptr(savgol_edge))
        return fail(ctx, FTK_ERR_INVALID, "interval, savgol and stats arrays must be host arrays");
    const int64_t limit = batch_bases ? batch_bases : kSpectrumBatchBases;
    // The intervals with a callable track, in consecutive batches of at most `limit` bases (a longer interval is a batch
    // of its own).  Interval j of a batch is scored at beg[j] of the scratch and adjusted to beg[j] - j * W; its WPS tiles
    // are those of ftk_wps_intervals.
    const int64_t need = (int64_t)W + std::max(sw, 1);
    std::vector<int64_t> orig, ks, ke, beg, a_off, p_off, batch_iv{0}, batch_tile{0};
    std::vector<int32_t> tile_iv, tile_k;
    int64_t fill = 0, most_in = 0, most_out = 0, most_iv = 0;
    auto close_batch = [&]() -> int {
        const int64_t i0 = batch_iv.back(), n = (int64_t)ks.size() - i0;
        const size_t at = a_off.size();
        for (int64_t j = 0; j < n; ++j) {
            a_off.push_back(beg[i0 + j]);
            p_off.push_back(beg[i0 + j] - j * W);
        }
        a_off.push_back(fill);
        p_off.push_back(fill - n * W);
        most_in = std::max(most_in, fill);
        most_out = std::max(most_out, fill - n * W);
        most_iv = std::max(most_iv, n);
        batch_iv.push_back((int64_t)ks.size());
        batch_tile.push_back((int64_t)tile_iv.size());
        fill = 0;
        return pc.add_batch(ctx, p_off.data() + at, n);
    };
    for (int64_t i = 0; i < n_iv; ++i) {
        const int64_t len = std::max<int64_t>(iv_stop[i] - iv_start[i], 0);
        if (len > 0 && (iv_start[i] < -(1LL << 30) || iv_stop[i] > (1LL << 31))) return fail(ctx, FTK_ERR_INVALID, "interval out of range");
        if (len - W > INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "interval %lld too long", (long long)i);
        if (len < need) continue;  // no callable track: zero calls, zero counters
        if (fill > 0 && fill + len > limit && (rc = close_batch())) return rc;
        const int64_t k = (int64_t)ks.size();
        orig.push_back(i);
        ks.push_back(iv_start[i]);
        ke.push_back(iv_stop[i]);
        beg.push_back(fill);
        fill += len;
        for (int64_t t = 0; t < (len + kWpsTile - 1) / kWpsTile; ++t) {
            tile_iv.push_back((int32_t)k);
            tile_k.push_back((int32_t)t);
        }
        if (tile_iv.size() > (size_t)INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "too many WPS tiles in one call");
    }
    const int64_t n_kept = (int64_t)ks.size();
    if (n_kept > 0 && (rc = close_batch())) return rc;
    memset(stats, 0, (size_t)n_iv * 6 * 8);  // (the arguments are good: an interval without a callable track keeps these zeros)
    if (n_kept == 0) return FTK_OK;
    const size_t n_tiles = tile_iv.size(), n_off = a_off.size();
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int64_t *d_scores = nullptr, *d_s = nullptr, *d_e = nullptr, *d_beg = nullptr, *d_aoff = nullptr, *d_poff = nullptr;
    int32_t *d_ti = nullptr, *d_tk = nullptr;
    double *d_coef = nullptr, *d_edge = nullptr, *d_adj = nullptr, *d_out = nullptr;
    std::vector<int64_t> kept_stats((size_t)n_kept * 6);
    Scratch s(ctx);
    AdjustChain chain;
    s.tmp(&d_scores, (size_t)most_in);  // int64 as scored, then the same values as float64 in place
    s.tmp(&d_out, (size_t)most_out);
    if (sw) {
        s.tmp(&d_adj, (size_t)most_out);
        s.tmp(&d_coef, (size_t)sw);
        s.tmp(&d_edge, (size_t)2 * half * sw);
    }
    s.tmp(&d_s, (size_t)n_kept);
    s.tmp(&d_e, (size_t)n_kept);
    s.tmp(&d_beg, (size_t)n_kept);
    s.tmp(&d_ti, n_tiles);
    s.tmp(&d_tk, n_tiles);
    s.tmp(&d_aoff, n_off);
    s.tmp(&d_poff, n_off);
    chain.declare(s, most_iv, W, false, most_out);
    if (chain.tiles_ub(most_out) > INT32_MAX - 1024) return fail(ctx, FTK_ERR_INVALID, "too many tiles in one batch");
    pc.declare(s, kept_stats.data());
    if ((rc = s.reserve())) return rc;
    if (!sw) d_adj = d_out;
    // From here on the stream may be reading this call's vectors: every way out waits for it first.
    auto enqueue = [&]() -> int {
        if (int e = pc.upload(ctx)) return e;
        HIPCHK(ctx, hipMemcpyAsync(d_s, ks.data(), (size_t)n_kept * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_e, ke.data(), (size_t)n_kept * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_beg, beg.data(), (size_t)n_kept * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_ti, tile_iv.data(), n_tiles * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_tk, tile_k.data(), n_tiles * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_aoff, a_off.data(), n_off * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_poff, p_off.data(), n_off * 8, hipMemcpyHostToDevice, ctx->stream));
        if (sw) {
            HIPCHK(ctx, hipMemcpyAsync(d_coef, savgol_coef, (size_t)sw * 8, hipMemcpyHostToDevice, ctx->stream));
            if (half) HIPCHK(ctx, hipMemcpyAsync(d_edge, savgol_edge, (size_t)2 * half * sw * 8, hipMemcpyHostToDevice, ctx->stream));
        }
        for (size_t b = 0; b + 1 < batch_iv.size(); ++b) {  // every batch is scored, adjusted and called in the same scratch
            const int64_t i0 = batch_iv[b], n = batch_iv[b + 1] - i0, t0 = batch_tile[b];
            const size_t at = (size_t)i0 + b;  // (one more offset than intervals per batch)
            int64_t adj_tiles = 0, adj_fast = 0;
            for (int64_t j = 0; j < n; ++j) chain.count(a_off[at + j + 1] - a_off[at + j], &adj_tiles, &adj_fast);
            launch_wps(ctx->stream, c->v, p, batch_tile[b + 1] - t0, d_s, d_e, d_beg, d_ti + t0, d_tk + t0, d_scores);
            launch_i64_to_f64(ctx->stream, d_scores, a_off[at + n]);
            chain.counts(ctx->stream, d_aoff + at, n);
            chain.run(ctx->stream, n, adj_tiles, adj_fast, (const double*)d_scores, nullptr, 0, d_adj, sw, d_coef, d_edge, d_out);
            HIPCHK(ctx, hipGetLastError());
            if (int e = pc.launch(ctx, b, d_out, d_poff + at, n, i0)) return e;
        }
        return FTK_OK;
    };
    if ((rc = enqueue()) || (rc = pc.finish(ctx, s, run, start, stop, summit, height, area, n_calls))) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    // home: the counters to their intervals' rows, runs to interval numbers, positions to contig coordinates
    for (int64_t k = 0; k < n_kept; ++k) memcpy(stats + orig[k] * 6, kept_stats.data() + k * 6, 6 * 8);
    for (int64_t i = 0; i < *n_calls; ++i) {
        const int32_t k = (*run)[i];
        const int64_t shift = ks[k] + W / 2;
        (*run)[i] = (int32_t)orig[k];
        (*start)[i] += shift;
        (*stop)[i] += shift;
        (*summit)[i] += shift;
    }
    return FTK_OK;
}

}  // extern "C"
