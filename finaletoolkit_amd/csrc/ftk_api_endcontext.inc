// Part of ftk_api.hip's translation unit (#included there behind the hotspots part) - the end-context tables:
// `ftk_end_context` (nucleotide / dinucleotide profiles around fragment ends or centres, per length class),
// `ftk_ref_context` (the background) and `ftk_end_context_lds_classes` over the kernels of ftk_endcontext.hip.
#include "ftk_endcontext.h"

namespace {

// which LDS arrangement ftk_end_context launches: lanes are fragments, the faster one as measured (docs/experiments.md),
// unless FTK_CONTEXT_ARRANGE=0 asks for lanes as offsets (tools/kbench.py times both; read at every call)
int end_context_arrangement() {
    const char* e = getenv("FTK_CONTEXT_ARRANGE");
    return e && atoi(e) == kCtxLanesAreOffsets ? kCtxLanesAreOffsets : kCtxLanesAreFragments;
}

}  // namespace

extern "C" {

int ftk_end_context_lds_classes(int32_t half_width) {
    return half_width < 1 || half_width > FTK_CONTEXT_MAX_HALF ? 0 : ctx_lds_classes(half_width);
}

int ftk_end_context(ftk_ctx* ctx, int contig_id, int ref_id, int32_t half_width, const int32_t* len_edges, int32_t n_classes,
                    int32_t mapq_min, int32_t anchor, int64_t* out, int64_t* n_kept_out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (!out || !n_kept_out || !len_edges) return fail(ctx, FTK_ERR_INVALID, "NULL pointer argument");
    ContigData* c;
    RefView im;
    int rc = get_contig(ctx, contig_id, &c);
    if (rc || (rc = open_gc_view(ctx, ref_id, &im))) return rc;
    if (half_width < 1 || half_width > FTK_CONTEXT_MAX_HALF)
        return fail(ctx, FTK_ERR_INVALID, "half_width %d outside [1, %d]", half_width, FTK_CONTEXT_MAX_HALF);
    if (n_classes < 1 || n_classes > FTK_CONTEXT_MAX_CLASSES)
        return fail(ctx, FTK_ERR_INVALID, "n_classes %d outside [1, %d]", n_classes, FTK_CONTEXT_MAX_CLASSES);
    if (anchor != FTK_CONTEXT_ENDS && anchor != FTK_CONTEXT_CENTRE) return fail(ctx, FTK_ERR_INVALID, "unknown anchor %d", anchor);
    EndContextParams p{};
    for (int k = 0; k <= n_classes; ++k) {
        if (len_edges[k] < 1 || len_edges[k] > (1 << 30) || (k && len_edges[k] <= len_edges[k - 1]))
            return fail(ctx, FTK_ERR_INVALID, "len_edges[%d] = %d: edges ascend strictly within [1, 2^30]", k, len_edges[k]);
        p.edges[k] = len_edges[k];
    }
    p.n_classes = n_classes;
    p.half = half_width;
    p.mapq_min = mapq_min;
    p.anchor = anchor;
    const size_t cells = (size_t)n_classes * (size_t)ctx_class_cells(half_width);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int64_t *d_out = nullptr, *d_kept = nullptr;
    Scratch s(ctx);
    return run_table_call(ctx, s, {{&d_out, out, cells}, {&d_kept, n_kept_out, (size_t)n_classes}}, [&] {
        launch_end_context(ctx->stream, ctx->n_cu, c->v, im, p, end_context_arrangement(), (unsigned long long*)d_out,
                           (unsigned long long*)d_kept);
        return FTK_OK;
    });
}

int ftk_ref_context(ftk_ctx* ctx, int ref_id, int64_t pos_lo, int64_t pos_hi, int64_t* out25) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (!out25) return fail(ctx, FTK_ERR_INVALID, "out25 is NULL");
    RefView im;
    int64_t hi;
    int rc = open_gc_view(ctx, ref_id, &im);
    if (rc || (rc = check_ref_range(ctx, im, pos_lo, pos_hi, &hi))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int64_t* d_out = nullptr;
    Scratch s(ctx);
    return run_table_call(ctx, s, {{&d_out, out25, (size_t)kCtxCellsPerRow}}, [&] {
        if (pos_lo < hi) launch_ref_context(ctx->stream, ctx->n_cu, im, (int)pos_lo, (int)hi, (unsigned long long*)d_out);
        return FTK_OK;
    });
}

}  // extern "C"
