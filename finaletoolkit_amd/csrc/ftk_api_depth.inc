// Part of ftk_api.hip's translation unit (#included there behind the export part) - the per-base depth track:
// `ftk_depth` (one value per base) and `ftk_depth_runs` (its run-length encoding) over the kernels of ftk_depth.hip.
#include "ftk_depth.h"

namespace {

// The shared front of both calls: arguments, contig, parameters.  *n_tiles == 0: an empty region, nothing to launch.
int open_depth_call(ftk_ctx* ctx, int contig_id, int64_t start, int64_t stop, int32_t min_len, int32_t max_len,
                    int32_t mapq_min, ContigData** c, DepthParams* p, int64_t* n_tiles) {
    if (start < 0 || stop < start) return fail(ctx, FTK_ERR_INVALID, "region [%lld, %lld) is not an interval", (long long)start, (long long)stop);
    if (stop >= (1LL << 30)) return fail(ctx, FTK_ERR_INVALID, "stop %lld reaches 2^30, the coordinate bound", (long long)stop);
    int rc = get_contig(ctx, contig_id, c);
    if (rc) return rc;
    const CleaveParams cp = cleave_params(**c, min_len, max_len, mapq_min);
    *p = DepthParams{start, stop, cp.min_len, cp.max_len, cp.mapq_min, cp.lmax, 0};
    *n_tiles = (stop - start + kWpsTile - 1) / kWpsTile;
    return FTK_OK;
}

}  // namespace

extern "C" {

int ftk_depth(ftk_ctx* ctx, int contig_id, int64_t start, int64_t stop, int32_t min_len, int32_t max_len, int32_t mapq_min,
              int32_t* depth_out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (!depth_out) return fail(ctx, FTK_ERR_INVALID, "depth_out is NULL");
    ContigData* c;
    DepthParams p;
    int64_t n_tiles;
    int rc = open_depth_call(ctx, contig_id, start, stop, min_len, max_len, mapq_min, &c, &p, &n_tiles);
    if (rc || n_tiles == 0) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t* d_out = nullptr;
    Scratch s(ctx);
    s.out(&d_out, depth_out, (size_t)(stop - start));
    if ((rc = s.reserve())) return rc;
    launch_depth(ctx->stream, c->v, p, n_tiles, d_out);
    HIPCHK(ctx, hipGetLastError());
    return s.finish();
}

int ftk_depth_runs(ftk_ctx* ctx, int contig_id, int64_t start, int64_t stop, int32_t min_len, int32_t max_len,
                   int32_t mapq_min, int include_zero, int32_t** run_start, int32_t** run_end, int32_t** run_depth,
                   int64_t* n_runs) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (!run_start || !run_end || !run_depth || !n_runs) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    *run_start = *run_end = *run_depth = nullptr;
    *n_runs = 0;
    ContigData* c;
    DepthParams p;
    int64_t n_tiles;
    int rc = open_depth_call(ctx, contig_id, start, stop, min_len, max_len, mapq_min, &c, &p, &n_tiles);
    if (rc || n_tiles == 0) return rc;
    p.include_zero = include_zero != 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t plan_bytes = 4 * align_up((size_t)n_tiles * 4) + align_up(8);
    if ((rc = reserve_scratch(ctx, plan_bytes))) return rc;
    DepthRunPlan rp{};
    auto carve = [&](Arena& a) {
        rp.cnt = a.take<int32_t>((size_t)n_tiles);
        rp.first = a.take<int32_t>((size_t)n_tiles);
        rp.off = a.take<int32_t>((size_t)n_tiles);
        rp.next = a.take<int32_t>((size_t)n_tiles);
        rp.total = a.take<int64_t>(1);
    };
    auto pass1 = [&]() -> int {
        Arena a(ctx);
        carve(a);
        launch_depth_count(ctx->stream, c->v, p, n_tiles, rp);
        HIPCHK(ctx, hipGetLastError());
        return FTK_OK;
    };
    if ((rc = pass1())) return rc;
    int64_t total = 0;
    HIPCHK(ctx, hipMemcpyAsync(&total, rp.total, sizeof(total), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (total < 0 || total > stop - start) return fail(ctx, FTK_ERR_HIP, "the run count %lld is out of range", (long long)total);
    if (total == 0) return FTK_OK;
    const size_t col = align_up((size_t)total * 4);
    const void* before = ctx->scratch;
    if ((rc = reserve_scratch(ctx, plan_bytes + 3 * col))) return rc;
    if (ctx->scratch != before && (rc = pass1())) return rc;  // the scratch moved: the tile plan went with the old block
    Arena a(ctx);
    carve(a);
    int32_t* d_run[3];
    for (auto& d : d_run) d = a.take<int32_t>((size_t)total);
    launch_depth_write(ctx->stream, c->v, p, n_tiles, rp, d_run[0], d_run[1], d_run[2]);
    HIPCHK(ctx, hipGetLastError());
    static constexpr size_t kSize[3] = {4, 4, 4};
    void** const out[3] = {(void**)run_start, (void**)run_end, (void**)run_depth};
    HostCols<3> home{kSize};
    SyncOnExit wait{ctx};  // (always: copies into this frame's blocks may be in flight)
    if (!home.grow(total)) return fail(ctx, FTK_ERR_OOM, "out of host memory");
    const void* dev[3] = {d_run[0], d_run[1], d_run[2]};
    if (const hipError_t e = home.fetch(ctx->stream, dev, total)) {
        (void)hipGetLastError();
        return fail(ctx, FTK_ERR_HIP, "copy of the runs failed: %s", hipGetErrorString(e));
    }
    home.give(out, n_runs);
    return FTK_OK;
}

}  // extern "C"
