// Part of ftk_api.hip's translation unit (#included there behind the depth part) - the fragment length x GC tables:
// `ftk_frag_gc` (gc per fragment), `ftk_frag_gc_table` (observed) and `ftk_ref_gc_table` (expected) over the kernels of
// ftk_gcbias.hip.
#include "ftk_gcbias.h"

namespace {

// The reference half of the three calls: the image's view, its coordinates below the bound the kernels' int arithmetic needs.
int open_gc_view(ftk_ctx* ctx, int ref_id, RefView* im) {
    const int rc = open_ref_view(ctx, ref_id, im);
    if (rc) return rc;
    if (im->chrom_len >= (1 << 30)) return fail(ctx, FTK_ERR_INVALID, "chrom_len %lld reaches 2^30, the coordinate bound", (long long)im->chrom_len);
    return FTK_OK;
}

int check_gc_lengths(ftk_ctx* ctx, int32_t len_lo, int32_t len_hi) {
    if (len_lo < 1 || len_hi < len_lo || len_hi > FTK_GC_MAX_LEN)
        return fail(ctx, FTK_ERR_INVALID, "lengths [%d, %d] are not within [1, %d]", len_lo, len_hi, FTK_GC_MAX_LEN);
    return FTK_OK;
}

// A reference call's positions [pos_lo, pos_hi) must be a range; *hi: its end clamped to the contig's (nothing is defined
// at or behind the contig's end), so the call launches when pos_lo < *hi.
int check_ref_range(ftk_ctx* ctx, const RefView& im, int64_t pos_lo, int64_t pos_hi, int64_t* hi) {
    *hi = std::min<int64_t>(pos_hi, im.chrom_len);
    if (pos_lo >= 0 && pos_hi >= pos_lo) return FTK_OK;
    return fail(ctx, FTK_ERR_INVALID, "positions [%lld, %lld) are not a range", (long long)pos_lo, (long long)pos_hi);
}

size_t gc_table_cells(int32_t len_lo, int32_t len_hi) { return (size_t)(len_hi - len_lo + 1) * (size_t)(len_hi + 1); }

}  // namespace

extern "C" {

int ftk_frag_gc(ftk_ctx* ctx, int contig_id, int ref_id, int32_t min_len, int32_t max_len, int32_t mapq_min, int16_t* gc_out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (!gc_out) return fail(ctx, FTK_ERR_INVALID, "gc_out is NULL");
    ContigData* c;
    RefView im;
    int rc = get_contig(ctx, contig_id, &c);
    if (rc || (rc = open_gc_view(ctx, ref_id, &im))) return rc;
    if (c->n == 0) return FTK_OK;
    // (gc is undefined below 1 and above FTK_GC_MAX_LEN bases: the open bounds close there)
    FragGcParams p{};
    p.min_len = min_len < 1 ? 1 : min_len;
    p.max_len = max_len < 0 || max_len > FTK_GC_MAX_LEN ? FTK_GC_MAX_LEN : max_len;
    p.mapq_min = mapq_min;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int16_t* d_out = nullptr;
    Scratch s(ctx);
    s.out(&d_out, gc_out, (size_t)c->n);  // (every row is written: nothing to zero)
    return run_table_call(ctx, s, {}, [&] {
        launch_frag_gc(ctx->stream, ctx->n_cu, c->v, im, p, d_out, nullptr, nullptr);
        return FTK_OK;
    });
}

int ftk_frag_gc_table(ftk_ctx* ctx, int contig_id, int ref_id, int32_t len_lo, int32_t len_hi, int32_t mapq_min,
                      int64_t* table_out, int64_t* n_skipped) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (!table_out || !n_skipped) return fail(ctx, FTK_ERR_INVALID, "NULL output pointer");
    ContigData* c;
    RefView im;
    int rc = get_contig(ctx, contig_id, &c);
    if (rc || (rc = open_gc_view(ctx, ref_id, &im)) || (rc = check_gc_lengths(ctx, len_lo, len_hi))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int64_t *d_table = nullptr, *d_skipped = nullptr;
    Scratch s(ctx);
    return run_table_call(ctx, s, {{&d_table, table_out, gc_table_cells(len_lo, len_hi)}, {&d_skipped, n_skipped, 1}}, [&] {
        FragGcParams p{len_lo, len_hi, mapq_min, len_lo, len_hi, len_lo};
        launch_frag_gc(ctx->stream, ctx->n_cu, c->v, im, p, nullptr, (unsigned long long*)d_table, (unsigned long long*)d_skipped);
        return FTK_OK;
    });
}

int ftk_ref_gc_table(ftk_ctx* ctx, int ref_id, int64_t pos_lo, int64_t pos_hi, int32_t len_lo, int32_t len_hi, int64_t stride,
                     int64_t* table_out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (!table_out) return fail(ctx, FTK_ERR_INVALID, "table_out is NULL");
    RefView im;
    int rc = open_gc_view(ctx, ref_id, &im);
    if (rc || (rc = check_gc_lengths(ctx, len_lo, len_hi))) return rc;
    if (stride < 1) return fail(ctx, FTK_ERR_INVALID, "stride %lld is below 1", (long long)stride);
    int64_t hi;
    if ((rc = check_ref_range(ctx, im, pos_lo, pos_hi, &hi))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int64_t* d_table = nullptr;
    Scratch s(ctx);
    return run_table_call(ctx, s, {{&d_table, table_out, gc_table_cells(len_lo, len_hi)}}, [&] {
        // (of the multiples of a stride of 2^30 or more only position 0 lies below the coordinate bound)
        if (pos_lo < hi)
            launch_ref_gc_table(ctx->stream, ctx->n_cu, im, (int)pos_lo, (int)hi, len_lo, len_hi, std::min<int64_t>(stride, 1LL << 30),
                                (unsigned long long*)d_table);
        return FTK_OK;
    });
}

}  // extern "C"
