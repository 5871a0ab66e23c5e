// Part of ftk_api.hip's translation unit (#included there behind the co-fragmentation part) - the end-motif x fragment-length
// table: `ftk_motif_length_table` and `ftk_motif_length_lds_rows` over the kernels of ftk_motiflen.hip.
#include "ftk_motiflen.h"

extern "C" {

int ftk_motif_length_lds_rows(int32_t k) { return k < 1 || k > FTK_MOTIFLEN_MAX_K ? 0 : motiflen_lds_rows(k); }

int ftk_motif_length_table(ftk_ctx* ctx, int contig_id, int ref_id, int32_t k, int32_t shift, int32_t len_lo, int32_t len_hi,
                           int32_t len_bin, int32_t mapq_min, int64_t* table_out, int64_t* n_kept_out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (!table_out || !n_kept_out) return fail(ctx, FTK_ERR_INVALID, "NULL pointer argument");
    ContigData* c;
    RefView im;
    int rc = get_contig(ctx, contig_id, &c);
    if (rc || (rc = open_gc_view(ctx, ref_id, &im))) return rc;
    if (k < 1 || k > FTK_MOTIFLEN_MAX_K) return fail(ctx, FTK_ERR_INVALID, "k %d outside [1, %d]", k, FTK_MOTIFLEN_MAX_K);
    if (shift < -4 || shift > 4) return fail(ctx, FTK_ERR_INVALID, "shift %d outside [-4, 4]", shift);
    if (len_lo < 1 || len_hi < len_lo || len_hi > (1 << 30))
        return fail(ctx, FTK_ERR_INVALID, "lengths [%d, %d] are not within [1, 2^30]", len_lo, len_hi);
    if (len_bin < 1) return fail(ctx, FTK_ERR_INVALID, "len_bin %d must be >= 1", len_bin);
    const int64_t n_rows = (int64_t)(len_hi - len_lo) / len_bin + 1;
    if (n_rows > FTK_MOTIFLEN_MAX_ROWS)
        return fail(ctx, FTK_ERR_INVALID, "%lld length rows, more than %d", (long long)n_rows, FTK_MOTIFLEN_MAX_ROWS);
    MotifLenParams p{};
    p.k = k;
    p.shift = shift;
    p.len_lo = len_lo;
    p.len_hi = len_hi;
    p.len_bin = len_bin;
    p.n_rows = (int)n_rows;
    p.mapq_min = mapq_min;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int64_t *d_out = nullptr, *d_kept = nullptr;
    Scratch s(ctx);
    return run_table_call(ctx, s, {{&d_out, table_out, (size_t)2 * (size_t)n_rows * (size_t)motiflen_cols(k)}, {&d_kept, n_kept_out, (size_t)n_rows}},
                          [&] {
                              launch_motif_length(ctx->stream, ctx->n_cu, c->v, im, p, (unsigned long long*)d_out,
                                                  (unsigned long long*)d_kept);
                              return FTK_OK;
                          });
}

}  // extern "C"
