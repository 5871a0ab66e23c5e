// Part of ftk_api.hip's translation unit (#included there behind the gcbias part) - the per-fragment weight column of a
// resident contig (`ftk_frags_set_weights`, `ftk_frags_weights`, `ftk_frags_set_gc_weights`) and its sums per window
// (`ftk_weighted_window_sums`) over the kernels of ftk_weights.hip.  The column is an optional allocation of ContigData,
// like r1 and order: free_contig releases it, so it goes with ftk_frags_release and when the contig id is loaded again.
#include "ftk_weights.h"

namespace {

// The contig's column, allocated on first use (n is fixed for the life of a resident contig).
int ensure_weights(ftk_ctx* ctx, ContigData* c) {
    if (c->weights) return FTK_OK;
    HIPCHK(ctx, hipMalloc((void**)&c->weights, align_up((size_t)c->n * 4 + 16)));
    return FTK_OK;
}

int no_weights(ftk_ctx* ctx, int contig_id) {
    return fail(ctx, FTK_ERR_INVALID, "contig %d has no weights column (ftk_frags_set_weights / ftk_frags_set_gc_weights)", contig_id);
}

}  // namespace

extern "C" {

int ftk_frags_set_weights(ftk_ctx* ctx, int contig_id, const uint32_t* w, int64_t n) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    ContigData* c;
    int rc = get_contig(ctx, contig_id, &c);
    if (rc) return rc;
    if (n != c->n) return fail(ctx, FTK_ERR_INVALID, "weights column has %lld rows, contig has %lld", (long long)n, (long long)c->n);
    if (n > 0 && !w) return fail(ctx, FTK_ERR_INVALID, "weights pointer is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure_weights(ctx, c))) return rc;
    if (n > 0) {
        const bool dev = is_device_ptr(w);
        HIPCHK(ctx, hipMemcpyAsync(c->weights, w, (size_t)n * 4, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
        if (!dev) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // the caller's array is free again
    }
    return FTK_OK;
}

int ftk_frags_weights(ftk_ctx* ctx, int contig_id, uint32_t* w_out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    ContigData* c;
    int rc = get_contig(ctx, contig_id, &c);
    if (rc) return rc;
    if (!w_out) return fail(ctx, FTK_ERR_INVALID, "w_out is NULL");
    if (!c->weights) return no_weights(ctx, contig_id);
    if (c->n == 0) return FTK_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool dev = is_device_ptr(w_out);
    HIPCHK(ctx, hipMemcpyAsync(w_out, c->weights, (size_t)c->n * 4, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    if (!dev) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return FTK_OK;
}

int ftk_frags_set_gc_weights(ftk_ctx* ctx, int contig_id, int ref_id, int32_t len_lo, int32_t len_hi, int32_t mapq_min,
                             const uint32_t* table, int64_t* n_zero_out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (!table || !n_zero_out) return fail(ctx, FTK_ERR_INVALID, "NULL table or output pointer");
    ContigData* c;
    RefView im;
    int rc = get_contig(ctx, contig_id, &c);
    if (rc || (rc = open_gc_view(ctx, ref_id, &im)) || (rc = check_gc_lengths(ctx, len_lo, len_hi))) return rc;
    if (is_device_ptr(table)) return fail(ctx, FTK_ERR_INVALID, "the weight table must be a host array");
    // rows L = len_lo .. len_hi of the (len_hi - len_lo + 1) x (len_hi + 1) table, cells g = 0 .. L of each: packed
    const size_t cells = (size_t)gc_weight_cells(len_lo, len_hi), pitch = (size_t)len_hi + 1;
    std::vector<uint32_t> packed(cells);
    size_t at = 0;
    for (int L = len_lo; L <= len_hi; ++L) {
        memcpy(packed.data() + at, table + (size_t)(L - len_lo) * pitch, ((size_t)L + 1) * 4);
        at += (size_t)L + 1;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    uint32_t* d_packed = nullptr;
    int64_t* d_zero = nullptr;
    Scratch s(ctx);
    s.tmp(&d_packed, cells);
    return run_table_call(ctx, s, {{&d_zero, n_zero_out, 1}}, [&]() -> int {
        if (const int e = ensure_weights(ctx, c)) return e;
        if (c->n > 0) {
            HIPCHK(ctx, hipMemcpyAsync(d_packed, packed.data(), cells * 4, hipMemcpyHostToDevice, ctx->stream));
            GcWeightParams p{len_lo, len_hi, mapq_min, 0, 0};
            launch_frag_gc_weights(ctx->stream, ctx->n_cu, c->v, im, p, d_packed, c->weights, (unsigned long long*)d_zero);
        }
        return FTK_OK;
    }, true);  // (`packed` is pageable staging of this call)
}

int ftk_weighted_window_sums(ftk_ctx* ctx, int contig_id, const int32_t* w_start, const int32_t* w_end, int64_t n_win,
                             const ftk_filter* f, int64_t* sum_out, int64_t* n_weighted_out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    ContigData* c;
    int rc = get_contig(ctx, contig_id, &c);
    if (rc || (rc = check_filter(ctx, f, *c, true))) return rc;
    if (!c->weights) return no_weights(ctx, contig_id);
    if (n_win < 0 || n_win > (1 << 30)) return fail(ctx, FTK_ERR_INVALID, "n_win out of range");
    if (n_win == 0) return FTK_OK;
    if (!w_start || !w_end) return fail(ctx, FTK_ERR_INVALID, "NULL window pointer");
    if (!sum_out) return fail(ctx, FTK_ERR_INVALID, "sum_out is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int64_t *d_sum = nullptr, *d_cnt = nullptr;
    WindowCall wc;
    Scratch s(ctx);
    s.out(&d_sum, sum_out, (size_t)n_win);
    if (n_weighted_out) s.out(&d_cnt, n_weighted_out, (size_t)n_win);
    s.tmp(&wc.b_ws, (size_t)n_win);
    s.tmp(&wc.b_we, (size_t)n_win);
    if ((rc = s.reserve())) return rc;
    HIPCHK(ctx, hipMemsetAsync(d_sum, 0, (size_t)n_win * 8, ctx->stream));
    if (d_cnt) HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, (size_t)n_win * 8, ctx->stream));
    if (c->n > 0) {
        const int lmax = eff_lmax(f, *c);  // (the lmax of cleave_params)
        if ((rc = window_prepare(ctx, c, w_start, w_end, n_win, lmax, -1, &wc, nullptr, false))) return rc;
        const WeightedWinParams p{f->mapq_min, f->min_len < 0 ? INT32_MIN : f->min_len, f->max_len < 0 ? INT32_MAX : f->max_len,
                                  f->policy, c->v.r1_start != nullptr && f->fetch_mode == FTK_FETCH_BAM_READ1, lmax};
        launch_weighted_windows(ctx->stream, c->v, c->weights, wc.d_ws, wc.d_we, (int)n_win,
                                weighted_window_slices(ctx->n_cu, n_win, c->n), p, (unsigned long long*)d_sum,
                                (unsigned long long*)d_cnt);
        HIPCHK(ctx, hipGetLastError());
    }
    return s.finish();
}

}  // extern "C"
