// Part of ftk_api.hip's translation unit (#included there behind the peaks part) - preferred fragment ends:
// `ftk_preferred_ends` over the kernels of ftk_prefends.hip.  The call checks its arguments, then walks the intervals'
// tiles in batches of kPrefBatchTiles: count pass and scan, ONE read-back (the tiles' counters and the batch's calls),
// room for exactly those calls, write pass, the calls home into host blocks of the library's that grow batch by batch.
// The plan of a batch has one size, so the scratch a whole chromosome takes is that of its fullest batch.  The
// per-interval counters are summed on the host from the tiles' counters: a count pass that has to run again, because the
// scratch moved when the calls' room was reserved, counts nothing twice.
#include "ftk_prefends.h"

namespace {

// May the call read lq instead of end and mapq?  (FTK_PACKED=0 keeps every launch on the wide columns, as in ftk_kernels.hip.)
bool prefends_packed(const ContigView& cv, const PrefParams& p) {
    static const int allow = getenv("FTK_PACKED") ? atoi(getenv("FTK_PACKED")) : 1;
    PackedCall c;
    c.has_lq = cv.lq != nullptr;
    c.wps = true;  // one mapq cut and one pair of length bounds, as a WPS launch has
    c.wps_q = p.mapq_min;
    c.wps_min = p.min_len;
    c.wps_max = p.max_len;
    return allow != 0 && packed_call_ok(c);
}

// the calls on their way home: six growing host blocks, the caller's once the call has succeeded
struct PrefHostCols {
    static constexpr size_t kSize[6] = {4, 8, 4, 4, 8, 4};  // run, pos, kind, count, total, n_w
    void* p[6] = {};
    int64_t n = 0;
    ~PrefHostCols() { for (void* q : p) free(q); }
    bool grow(int64_t more) {
        for (int k = 0; k < 6; ++k) {
            void* q = realloc(p[k], (size_t)(n + more) * kSize[k]);
            if (!q) return false;
            p[k] = q;
        }
        return true;
    }
};

struct PrefSyncOnExit {  // pageable staging of this frame may be in flight on any way out
    ftk_ctx* ctx;
    ~PrefSyncOnExit() { (void)hipStreamSynchronize(ctx->stream); }
};

}  // namespace

extern "C" {

int ftk_preferred_ends(ftk_ctx* ctx, int contig_id, const int64_t* iv_start, const int64_t* iv_stop, int64_t n_iv, int64_t chrom_size,
                       int32_t half, int32_t mode, int32_t min_count, const uint64_t* thr, int32_t n_thr, int32_t min_len,
                       int32_t max_len, int32_t mapq_min, int32_t** run, int64_t** pos, int32_t** kind, int32_t** count,
                       int64_t** total, int32_t** n_w, int64_t* n_calls, int64_t* stats) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (!run || !pos || !kind || !count || !total || !n_w || !n_calls) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    *run = *kind = *count = *n_w = nullptr;
    *pos = *total = nullptr;
    *n_calls = 0;
    if (chrom_size < 0 || chrom_size >= (1LL << 30)) return fail(ctx, FTK_ERR_INVALID, "chrom_size %lld outside [0, 2^30)", (long long)chrom_size);
    if (half < 1 || half > FTK_PREFENDS_MAX_HALF) return fail(ctx, FTK_ERR_INVALID, "half %d outside [1, %d]", half, FTK_PREFENDS_MAX_HALF);
    if (mode != FTK_PREFENDS_COMBINED && mode != FTK_PREFENDS_SPLIT) return fail(ctx, FTK_ERR_INVALID, "mode %d is neither 0 nor 1", mode);
    if (min_count < 1) return fail(ctx, FTK_ERR_INVALID, "min_count %d below 1", min_count);
    if (n_thr < 2 || n_thr > FTK_PREFENDS_MAX_THR) return fail(ctx, FTK_ERR_INVALID, "n_thr %d outside [2, %d]", n_thr, FTK_PREFENDS_MAX_THR);
    if (n_iv < 0 || n_iv > INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "n_iv out of range");
    if (!thr || (n_iv > 0 && (!iv_start || !iv_stop || !stats))) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    if (is_device_ptr(thr) || is_device_ptr(iv_start) || is_device_ptr(iv_stop) || is_device_ptr(stats))
        return fail(ctx, FTK_ERR_INVALID, "interval, threshold and stats arrays must be host arrays");
    for (int k = 0; k < n_thr; ++k)
        if (thr[k] >= (1ULL << 40)) return fail(ctx, FTK_ERR_INVALID, "threshold %d reaches 2^40", k);
    for (int64_t i = 0; i < n_iv; ++i)
        if (iv_start[i] < 0 || iv_stop[i] < iv_start[i] || iv_stop[i] > chrom_size)
            return fail(ctx, FTK_ERR_INVALID, "interval %lld [%lld, %lld) does not lie in [0, %lld)", (long long)i, (long long)iv_start[i],
                        (long long)iv_stop[i], (long long)chrom_size);
    ContigData* c;
    int rc = get_contig(ctx, contig_id, &c);
    if (rc) return rc;
    const CleaveParams cp = cleave_params(*c, min_len, max_len, mapq_min);
    PrefParams p{};
    p.chrom = (int)chrom_size;
    p.half = half;
    p.split = mode == FTK_PREFENDS_SPLIT;
    p.min_count = (unsigned)min_count;
    p.n_thr = n_thr;
    p.min_len = cp.min_len;
    p.max_len = cp.max_len;
    p.mapq_min = cp.mapq_min;
    p.lmax = cp.lmax;
    p.packed = prefends_packed(c->v, p);
    HIPCHK(ctx, hipSetDevice(ctx->device));

    constexpr size_t B = kPrefBatchTiles;
    const size_t plan_bytes = align_up((size_t)n_thr * 8) + 4 * align_up(B * 4) + align_up(B * kPrefStats * 4) + align_up(8);
    std::vector<int32_t> t0, tlen, trun;  // the batch's tiles (pageable staging: every way out waits for the stream)
    std::vector<uint32_t> tstats;
    std::vector<int64_t> sums((size_t)n_iv * kPrefStats, 0);
    PrefHostCols home;
    PrefSyncOnExit wait{ctx};
    PrefPlan pl{};
    // the batch's plan at the scratch base, the count pass and the scan
    auto count_pass = [&](Arena& a) -> int {
        const size_t nt = t0.size();
        uint64_t* d_thr = a.take<uint64_t>((size_t)n_thr);
        int32_t* d_t0 = a.take<int32_t>(B);
        int32_t* d_len = a.take<int32_t>(B);
        int32_t* d_run = a.take<int32_t>(B);
        pl.off = a.take<int32_t>(B);
        pl.stats = a.take<uint32_t>(B * kPrefStats);
        pl.total = a.take<int64_t>(1);
        pl.tile_t0 = d_t0;
        pl.tile_len = d_len;
        pl.tile_run = d_run;
        p.thr = reinterpret_cast<const unsigned long long*>(d_thr);
        HIPCHK(ctx, hipMemcpyAsync(d_thr, thr, (size_t)n_thr * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_t0, t0.data(), nt * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_len, tlen.data(), nt * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_run, trun.data(), nt * 4, hipMemcpyHostToDevice, ctx->stream));
        launch_prefends_count(ctx->stream, c->v, p, (int)nt, pl);
        HIPCHK(ctx, hipGetLastError());
        return FTK_OK;
    };
    auto run_batch = [&]() -> int {
        const size_t nt = t0.size();
        if (int e = reserve_scratch(ctx, plan_bytes)) return e;
        {
            Arena a(ctx);
            if (int e = count_pass(a)) return e;
        }
        int64_t n = 0;
        tstats.resize(nt * kPrefStats);
        HIPCHK(ctx, hipMemcpyAsync(tstats.data(), pl.stats, nt * kPrefStats * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(&n, pl.total, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        int64_t seen = 0;
        for (size_t t = 0; t < nt; ++t) {
            for (int k = 0; k < kPrefStats; ++k) sums[(size_t)trun[t] * kPrefStats + k] += tstats[t * kPrefStats + k];
            seen += (int64_t)tstats[t * kPrefStats + 4] + tstats[t * kPrefStats + 5];
        }
        if (n != seen || n > (int64_t)nt * kPrefTile * 2) return fail(ctx, FTK_ERR_HIP, "the call count %lld is out of range", (long long)n);
        if (n == 0) return FTK_OK;
        const void* before = ctx->scratch;
        if (int e = reserve_scratch(ctx, plan_bytes + 4 * align_up((size_t)n * 4) + 2 * align_up((size_t)n * 8))) return e;
        Arena a(ctx);
        if (ctx->scratch != before) {  // the scratch moved: the plan went with the old block
            if (int e = count_pass(a)) return e;
        } else {
            a.off = plan_bytes;
        }
        PrefOut o{};
        o.run = a.take<int32_t>((size_t)n);
        o.pos = a.take<int64_t>((size_t)n);
        o.kind = a.take<int32_t>((size_t)n);
        o.count = a.take<int32_t>((size_t)n);
        o.total = a.take<int64_t>((size_t)n);
        o.n_w = a.take<int32_t>((size_t)n);
        launch_prefends_write(ctx->stream, c->v, p, (int)nt, pl, o);
        HIPCHK(ctx, hipGetLastError());
        if (!home.grow(n)) return fail(ctx, FTK_ERR_OOM, "out of host memory");
        const void* dev[6] = {o.run, o.pos, o.kind, o.count, o.total, o.n_w};
        for (int k = 0; k < 6; ++k) {
            const size_t sz = PrefHostCols::kSize[k];
            HIPCHK(ctx, hipMemcpyAsync((char*)home.p[k] + (size_t)home.n * sz, dev[k], (size_t)n * sz, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        home.n += n;
        return FTK_OK;
    };
    for (int64_t i = 0; i < n_iv; ++i)
        for (int64_t a = iv_start[i]; a < iv_stop[i]; a += kPrefTile) {
            t0.push_back((int32_t)a);
            tlen.push_back((int32_t)std::min<int64_t>(iv_stop[i] - a, kPrefTile));
            trun.push_back((int32_t)i);
            if (t0.size() == B) {
                if ((rc = run_batch())) return rc;
                t0.clear();
                tlen.clear();
                trun.clear();
            }
        }
    if (!t0.empty() && (rc = run_batch())) return rc;
    if (n_iv > 0) memcpy(stats, sums.data(), sums.size() * 8);
    if (home.n > 0) {
        *run = (int32_t*)home.p[0];
        *pos = (int64_t*)home.p[1];
        *kind = (int32_t*)home.p[2];
        *count = (int32_t*)home.p[3];
        *total = (int64_t*)home.p[4];
        *n_w = (int32_t*)home.p[5];
        *n_calls = home.n;
        for (void*& q : home.p) q = nullptr;
    }
    return FTK_OK;
}

}  // extern "C"
