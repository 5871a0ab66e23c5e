// Part of ftk_api.hip's translation unit (#included there behind the V-plot part) - the periodogram of integer score
// runs (`ftk_track_spectrum`) and of the WPS of intervals scored into device scratch (`ftk_wps_spectrum`) over the
// kernels of ftk_spectrum.hip.  Both check their arguments, build the twiddle tables of the requested periods on the
// device and run the two passes (prep, fold) over the runs; the fused call does so batch by batch of intervals, every
// batch scoring into the same scratch.
#include "ftk_spectrum.h"

namespace {

// Intervals of one batch of ftk_wps_spectrum hold at most this many bases unless the caller says otherwise: 2 x 256 MiB
// of scratch (the int64 scores and the float64 x), enough for 3 000 gene bodies of 10 kb in one launch.
constexpr int64_t kSpectrumBatchBases = int64_t(1) << 25;

// The periods of one call: checked, then their tables on the device.
struct SpectrumPeriods {
    int n_per = 0;
    std::vector<int32_t> tab_off;  // pageable staging of the upload: the caller waits for the stream before it returns
    size_t entries = 0;
    int32_t *d_periods = nullptr, *d_off = nullptr;
    Twiddle* d_table = nullptr;
    int* d_bad = nullptr;

    int check(ftk_ctx* ctx, const int32_t* periods, int32_t n, double taper) {
        if (n < 0 || n > kSpectrumMaxPeriods) return fail(ctx, FTK_ERR_INVALID, "n_per %d out of range (0 .. %d)", n, kSpectrumMaxPeriods);
        if (!(taper >= 0.0 && taper <= 0.5)) return fail(ctx, FTK_ERR_INVALID, "taper %g out of range (0 .. 0.5)", taper);
        if (n > 0 && !periods) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
        if (is_device_ptr(periods)) return fail(ctx, FTK_ERR_INVALID, "periods must be a host array");
        n_per = n;
        tab_off.resize((size_t)n);
        for (int k = 0; k < n; ++k) {
            if (periods[k] < kSpectrumMinPeriod || periods[k] > kSpectrumMaxPeriod)
                return fail(ctx, FTK_ERR_INVALID, "period %d out of range (%d .. %d)", periods[k], kSpectrumMinPeriod, kSpectrumMaxPeriod);
            tab_off[k] = (int32_t)entries;  // (<= 1024 * 4096)
            entries += (size_t)periods[k];
        }
        return FTK_OK;
    }
    void declare(Scratch& s) {
        s.tmp(&d_periods, (size_t)n_per);
        s.tmp(&d_off, (size_t)n_per);
        s.tmp(&d_table, entries);
        s.tmp(&d_bad, 1);
    }
    int upload(ftk_ctx* ctx, const int32_t* periods) {
        HIPCHK(ctx, hipMemcpyAsync(d_periods, periods, (size_t)n_per * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_off, tab_off.data(), (size_t)n_per * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(d_bad, 0, sizeof(int), ctx->stream));
        launch_spectrum_twiddles(ctx->stream, d_periods, d_off, n_per, d_table);
        HIPCHK(ctx, hipGetLastError());
        return FTK_OK;
    }
    // the two passes over runs [0, n_runs) of v; d_out / d_ssw: the first run's row; h_beg / h_end: the host's copy of d_beg / d_end
    int transform(ftk_ctx* ctx, const int64_t* v, const int64_t* d_beg, const int64_t* d_end, const int64_t* h_beg, const int64_t* h_end,
                  int64_t n_runs, double taper, int detrend, double* d_x, double* d_out, double* d_ssw) const {
        // FTK_SPECTRUM_LDS=0: every run is folded from memory (an experiment switch; the results are the same bits)
        static const bool staging = !(getenv("FTK_SPECTRUM_LDS") && atoi(getenv("FTK_SPECTRUM_LDS")) == 0);
        if (staging && !ctx->spectrum_lds) HIPCHK(ctx, spectrum_lds_samples(ctx->device, &ctx->spectrum_lds));
        const int limit = staging ? ctx->spectrum_lds : -1;
        const int64_t chunks = spectrum_chunks(n_per, kSpectrumWaves), per_launch = kSpectrumMaxBlocks / chunks;
        for (int64_t r0 = 0; r0 < n_runs; r0 += per_launch) {
            const int64_t part = std::min(n_runs - r0, per_launch);
            int longest_staged = -1;
            bool any_longer = false;
            for (int64_t r = r0; r < r0 + part; ++r) {
                const int64_t len = h_end[r] - h_beg[r];
                if (len <= limit) longest_staged = std::max(longest_staged, (int)len);
                else any_longer = true;
            }
            launch_spectrum_prep(ctx->stream, v, d_beg + r0, d_end + r0, part, taper, detrend, d_x, d_ssw ? d_ssw + r0 : nullptr, d_bad);
            launch_spectrum_fold(ctx->stream, d_x, d_beg + r0, d_end + r0, part, d_periods, d_off, d_table, n_per, limit, longest_staged,
                                 any_longer, d_out + (size_t)r0 * (size_t)n_per * 2);
            HIPCHK(ctx, hipGetLastError());
        }
        return FTK_OK;
    }
    // behind the last transform: copies the range flag home with the outputs (waits for the stream)
    int finish(ftk_ctx* ctx, Scratch& s) const {
        int bad = 0;
        HIPCHK(ctx, hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        if (int rc = s.finish(true)) return rc;
        if (bad) return fail(ctx, FTK_ERR_INVALID, "a score is outside (-2^31, 2^31)");
        return FTK_OK;
    }
};

}  // namespace

extern "C" {

int ftk_track_spectrum(ftk_ctx* ctx, const int64_t* scores, const int64_t* offsets, int64_t n_iv, const int32_t* periods,
                       int32_t n_per, double taper, int detrend, double* out, double* ssw_out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    SpectrumPeriods sp;
    int rc = sp.check(ctx, periods, n_per, taper);
    if (rc) return rc;
    if (n_iv < 0 || n_iv > INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "n_iv out of range");
    if (n_iv == 0 || n_per == 0) return FTK_OK;
    if (!scores || !offsets || !out) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    if (is_device_ptr(offsets)) return fail(ctx, FTK_ERR_INVALID, "offsets must be a host array");
    if (offsets[0] < 0) return fail(ctx, FTK_ERR_INVALID, "negative offset");
    std::vector<int64_t> rel((size_t)n_iv + 1);  // offsets from the first run's start (pageable staging)
    for (int64_t i = 0; i <= n_iv; ++i) {
        rel[i] = offsets[i] - offsets[0];
        if (i && offsets[i] < offsets[i - 1]) return fail(ctx, FTK_ERR_INVALID, "offsets decrease at run %lld", (long long)i - 1);
        if (i && offsets[i] - offsets[i - 1] > kSpectrumMaxRun)
            return fail(ctx, FTK_ERR_INVALID, "run %lld is longer than %lld", (long long)i - 1, kSpectrumMaxRun);
    }
    const size_t total = (size_t)rel[n_iv];
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool in_dev = is_device_ptr(scores);
    int64_t *d_stage = nullptr, *d_rel = nullptr;
    double *d_x = nullptr, *d_out = nullptr, *d_ssw = nullptr;
    Scratch s(ctx);
    if (!in_dev) s.tmp(&d_stage, total);
    s.tmp(&d_x, total);
    s.tmp(&d_rel, (size_t)n_iv + 1);
    sp.declare(s);
    s.out(&d_out, out, (size_t)n_iv * (size_t)n_per * 2);
    if (ssw_out) s.out(&d_ssw, ssw_out, (size_t)n_iv);
    if ((rc = s.reserve())) return rc;
    // From here on the stream may be reading this call's vectors: every way out waits for it first.
    auto enqueue = [&]() -> int {
        if (int e = sp.upload(ctx, periods)) return e;
        HIPCHK(ctx, hipMemcpyAsync(d_rel, rel.data(), ((size_t)n_iv + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        const int64_t* v = scores + offsets[0];
        if (!in_dev) {
            if (total) HIPCHK(ctx, hipMemcpyAsync(d_stage, v, total * 8, hipMemcpyHostToDevice, ctx->stream));
            v = d_stage;
        }
        return sp.transform(ctx, v, d_rel, d_rel + 1, rel.data(), rel.data() + 1, n_iv, taper, detrend != 0, d_x, d_out, d_ssw);
    };
    if ((rc = enqueue()) || (rc = sp.finish(ctx, s))) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

int ftk_wps_spectrum(ftk_ctx* ctx, int contig_id, const int64_t* iv_start, const int64_t* iv_stop, int64_t n_iv, int64_t chrom_size,
                     int32_t window_size, int32_t min_len, int32_t max_len, int32_t mapq_min, const int32_t* periods,
                     int32_t n_per, double taper, int detrend, int64_t batch_bases, double* out, double* ssw_out) {
    ContigData* c;
    WpsParams p{};
    int rc = open_wps_call(ctx, contig_id, chrom_size, window_size, min_len, max_len, mapq_min, &c, &p);
    if (rc) return rc;
    SpectrumPeriods sp;
    if ((rc = sp.check(ctx, periods, n_per, taper))) return rc;
    if (batch_bases < 0) return fail(ctx, FTK_ERR_INVALID, "negative batch_bases");
    if (n_iv < 0 || n_iv > INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "n_iv out of range");
    if (n_iv == 0 || n_per == 0) return FTK_OK;
    if (!iv_start || !iv_stop || !out) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    if (is_device_ptr(iv_start) || is_device_ptr(iv_stop)) return fail(ctx, FTK_ERR_INVALID, "interval arrays must be host arrays");
    const int64_t limit = batch_bases ? batch_bases : kSpectrumBatchBases;
    // Consecutive batches of at most `limit` bases (an interval longer than that is a batch of its own); an interval's
    // scores start at beg[i] of its batch's scratch and its tiles are those of ftk_wps_intervals.
    std::vector<int64_t> beg((size_t)n_iv), end((size_t)n_iv), batch_iv{0}, batch_tile{0};
    std::vector<int32_t> tile_iv, tile_k;
    int64_t fill = 0, most = 0;
    for (int64_t i = 0; i < n_iv; ++i) {
        const int64_t len = std::max<int64_t>(iv_stop[i] - iv_start[i], 0);  // a degenerate interval: an empty run
        if (len > 0 && (iv_start[i] < -(1LL << 30) || iv_stop[i] > (1LL << 31))) return fail(ctx, FTK_ERR_INVALID, "interval out of range");
        if (len > kSpectrumMaxRun) return fail(ctx, FTK_ERR_INVALID, "interval %lld is longer than %lld", (long long)i, kSpectrumMaxRun);
        if (fill > 0 && fill + len > limit) {
            batch_iv.push_back(i);
            batch_tile.push_back((int64_t)tile_iv.size());
            fill = 0;
        }
        beg[i] = fill;
        end[i] = fill += len;
        most = std::max(most, fill);
        for (int64_t k = 0; k < (len + kWpsTile - 1) / kWpsTile; ++k) {
            tile_iv.push_back((int32_t)i);
            tile_k.push_back((int32_t)k);
        }
        if (tile_iv.size() > (size_t)INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "too many WPS tiles in one call");
    }
    batch_iv.push_back(n_iv);
    batch_tile.push_back((int64_t)tile_iv.size());
    const size_t n_tiles = tile_iv.size();
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int64_t *d_scores = nullptr, *d_s = nullptr, *d_e = nullptr, *d_beg = nullptr, *d_end = nullptr;
    int32_t *d_ti = nullptr, *d_tk = nullptr;
    double *d_x = nullptr, *d_out = nullptr, *d_ssw = nullptr;
    Scratch s(ctx);
    s.tmp(&d_scores, (size_t)most);
    s.tmp(&d_x, (size_t)most);
    s.tmp(&d_s, (size_t)n_iv);
    s.tmp(&d_e, (size_t)n_iv);
    s.tmp(&d_beg, (size_t)n_iv);
    s.tmp(&d_end, (size_t)n_iv);
    s.tmp(&d_ti, n_tiles);
    s.tmp(&d_tk, n_tiles);
    sp.declare(s);
    s.out(&d_out, out, (size_t)n_iv * (size_t)n_per * 2);
    if (ssw_out) s.out(&d_ssw, ssw_out, (size_t)n_iv);
    if ((rc = s.reserve())) return rc;
    // From here on the stream may be reading this call's vectors: every way out waits for it first.
    auto enqueue = [&]() -> int {
        if (int e = sp.upload(ctx, periods)) return e;
        HIPCHK(ctx, hipMemcpyAsync(d_s, iv_start, (size_t)n_iv * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_e, iv_stop, (size_t)n_iv * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_beg, beg.data(), (size_t)n_iv * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_end, end.data(), (size_t)n_iv * 8, hipMemcpyHostToDevice, ctx->stream));
        if (n_tiles) {
            HIPCHK(ctx, hipMemcpyAsync(d_ti, tile_iv.data(), n_tiles * 4, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipMemcpyAsync(d_tk, tile_k.data(), n_tiles * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        for (size_t b = 0; b + 1 < batch_iv.size(); ++b) {  // every batch scores into, and transforms, the same scratch
            const int64_t i0 = batch_iv[b], t0 = batch_tile[b];
            launch_wps(ctx->stream, c->v, p, batch_tile[b + 1] - t0, d_s, d_e, d_beg, d_ti + t0, d_tk + t0, d_scores);
            HIPCHK(ctx, hipGetLastError());
            if (int e = sp.transform(ctx, d_scores, d_beg + i0, d_end + i0, beg.data() + i0, end.data() + i0, batch_iv[b + 1] - i0, taper, detrend != 0, d_x,
                                     d_out + (size_t)i0 * (size_t)n_per * 2, d_ssw ? d_ssw + i0 : nullptr))
                return e;
        }
        return FTK_OK;
    };
    if ((rc = enqueue()) || (rc = sp.finish(ctx, s))) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

}  // extern "C"
