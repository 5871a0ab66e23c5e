// Part of ftk_api.hip's translation unit (#included there behind the peaks part) - preferred fragment ends:
// `ftk_preferred_ends` over the kernels of ftk_prefends.hip.  The call checks its arguments and hands its rule's pieces
// to run_tile_call, which walks the intervals' tiles in batches; the per-interval counters are the sums of the tiles'.
#include "ftk_prefends.h"

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
    ContigData* c;
    int rc = check_intervals_in_contig(ctx, iv_start, iv_stop, n_iv, chrom_size);
    if (rc || (rc = get_contig(ctx, contig_id, &c))) return rc;
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
    p.packed = call_reads_packed(c->v, p.mapq_min, p.min_len, p.max_len);
    HIPCHK(ctx, hipSetDevice(ctx->device));

    static constexpr size_t kSize[6] = {4, 8, 4, 4, 8, 4};  // run, pos, kind, count, total, n_w
    std::vector<int64_t> sums((size_t)n_iv * kPrefStats, 0);
    HostCols<6> home{kSize};
    rc = run_tile_call(
        ctx, thr, (size_t)n_thr * 8, kPrefStats, 2, home,
        [&](const void* d_thr, int nt, const TileCallPlan& pl) {
            p.thr = static_cast<const unsigned long long*>(d_thr);
            launch_prefends_count(ctx->stream, c->v, p, nt, pl);
        },
        [&](int nt, const TileCallPlan& pl, void* const* col) {
            const PrefOut o{(int32_t*)col[0], (int64_t*)col[1], (int32_t*)col[2], (int32_t*)col[3], (int64_t*)col[4], (int32_t*)col[5]};
            launch_prefends_write(ctx->stream, c->v, p, nt, pl, o);
        },
        [&](int32_t iv, int32_t, const uint32_t* ts) {
            for (int k = 0; k < kPrefStats; ++k) sums[(size_t)iv * kPrefStats + k] += ts[k];
            return (int64_t)ts[4] + ts[5];
        },
        [](int64_t, int64_t) { return true; },
        [&](auto&& push_tile) {
            for (int64_t i = 0; i < n_iv; ++i)
                for (int64_t a = iv_start[i]; a < iv_stop[i]; a += kCallTile)
                    if (int e = push_tile(a, std::min<int64_t>(iv_stop[i] - a, kCallTile), i)) return e;
            return (int)FTK_OK;
        });
    if (rc) return rc;
    if (n_iv > 0) memcpy(stats, sums.data(), sums.size() * 8);
    void** const out[6] = {(void**)run, (void**)pos, (void**)kind, (void**)count, (void**)total, (void**)n_w};
    home.give(out, n_calls);
    return FTK_OK;
}

}  // extern "C"
