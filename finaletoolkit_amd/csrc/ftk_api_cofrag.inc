// Part of ftk_api.hip's translation unit (#included there behind the end-context part) - the co-fragmentation calls:
// `ftk_hist_ks` (pairwise KS numerators of histogram rows), `ftk_cofrag` (the same over the length histograms of a
// resident contig's windows, which never leave the device) and `ftk_hist_ks_shape` over the kernels of ftk_cofrag.hip.
#include "ftk_cofrag.h"

namespace {

// which pair kernel the calls launch: the tiled one, the faster as measured (docs/experiments.md), unless
// FTK_COFRAG_ARRANGE=0 asks for a thread per pair (tools/kbench.py times both; read at every call)
int cofrag_arrangement() {
    const char* e = getenv("FTK_COFRAG_ARRANGE");
    return e && atoi(e) == kKsPairThreads ? kKsPairThreads : kKsTiles;
}

// What both calls keep at the base of the scratch: the histogram rows (staged from the host, or built there by the
// window pass), their prefix image, the row totals and the flag of the row pass.
struct KsFront {
    uint32_t* b_hist = nullptr;
    uint32_t* prefix = nullptr;
    uint32_t* n32 = nullptr;
    int32_t* bad_row = nullptr;
    void declare(Scratch& s, bool hist_buf, int64_t n_rows, int32_t n_bins) {
        if (hist_buf) s.tmp(&b_hist, (size_t)n_rows * (size_t)n_bins);
        s.tmp(&prefix, (size_t)n_bins * (size_t)ks_pitch((int)n_rows));
        s.tmp(&n32, (size_t)ks_pitch((int)n_rows));
        s.tmp(&bad_row, 1);
    }
};

// the most the three outputs take behind the front when all of them are host arrays
size_t ks_outputs_room(int64_t n_rows) {
    const size_t cells = (size_t)n_rows * (size_t)n_rows;
    return align_up(cells * 8) + align_up(cells * 4) + align_up((size_t)n_rows * 8);
}

int check_ks_arguments(ftk_ctx* ctx, const void* in, int64_t n_rows, int32_t n_bins, const int64_t* k_out, const int64_t* n_out) {
    if (!in || !k_out || !n_out) return fail(ctx, FTK_ERR_INVALID, "NULL pointer argument");
    if (n_rows < 1 || n_rows > FTK_COFRAG_MAX_BINS)
        return fail(ctx, FTK_ERR_INVALID, "%lld histogram rows: 1 .. %d are supported", (long long)n_rows, FTK_COFRAG_MAX_BINS);
    if (n_bins < 1 || n_bins > FTK_COFRAG_MAX_LEN_BINS)
        return fail(ctx, FTK_ERR_INVALID, "n_bins %d outside [1, %d]", n_bins, FTK_COFRAG_MAX_LEN_BINS);
    return FTK_OK;
}

// The row pass over d_hist (device), the host's look at its flag - nothing has been written to an output by then - and
// the pair kernel into the outputs, which get their place behind the front's `front_bytes`.
int ks_rows_then_pairs(ftk_ctx* ctx, const KsFront& k, size_t front_bytes, const uint32_t* d_hist, int64_t n_rows, int32_t n_bins,
                       int64_t* k_out, int32_t* at_out, int64_t* n_out) {
    HIPCHK(ctx, hipMemsetAsync(k.bad_row, 0x7f, 4, ctx->stream));
    launch_ks_rows(ctx->stream, d_hist, (int)n_rows, n_bins, k.prefix, k.n32, k.bad_row);
    HIPCHK(ctx, hipGetLastError());
    int32_t bad = kKsNoRow;
    HIPCHK(ctx, hipMemcpyAsync(&bad, k.bad_row, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (bad != kKsNoRow) return fail(ctx, FTK_ERR_INVALID, "histogram row %d sums to 2^31 or more", bad);
    int64_t *d_k = nullptr, *d_n = nullptr;
    int32_t* d_at = nullptr;
    Scratch s(ctx, front_bytes);
    if (at_out) s.out(&d_at, at_out, (size_t)n_rows * (size_t)n_rows);
    const int arrangement = cofrag_arrangement();
    return run_table_call(ctx, s, {{&d_k, k_out, (size_t)n_rows * (size_t)n_rows}, {&d_n, n_out, (size_t)n_rows}}, [&] {
        launch_ks_pairs(ctx->stream, arrangement, k.prefix, k.n32, (int)n_rows, n_bins, (long long*)d_k, d_at, (long long*)d_n);
        return FTK_OK;
    });
}

}  // namespace

extern "C" {

int ftk_hist_ks_shape(int32_t* tile_out, int32_t* chunk_out) {
    if (!tile_out || !chunk_out) return fail(nullptr, FTK_ERR_INVALID, "NULL pointer argument");
    *tile_out = kKsTile;
    *chunk_out = kKsChunk;
    return FTK_OK;
}

int ftk_hist_ks(ftk_ctx* ctx, const uint32_t* hist, int64_t n_rows, int32_t n_bins, int64_t* k_out, int32_t* at_out, int64_t* n_out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    int rc = check_ks_arguments(ctx, hist, n_rows, n_bins, k_out, n_out);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool hist_dev = is_device_ptr(hist);
    KsFront k;
    Scratch front(ctx);
    k.declare(front, !hist_dev, n_rows, n_bins);
    // the whole call's room at once: the block must not move between the row pass and the pair kernel
    if ((rc = reserve_scratch(ctx, front.bytes() + ks_outputs_room(n_rows))) || (rc = front.place())) return rc;
    const uint32_t* d_hist = nullptr;
    if ((rc = stage_in(ctx, hist, (size_t)n_rows * (size_t)n_bins, k.b_hist, &d_hist))) return rc;
    return ks_rows_then_pairs(ctx, k, front.bytes(), d_hist, n_rows, n_bins, k_out, at_out, n_out);
}

int ftk_cofrag(ftk_ctx* ctx, int contig_id, const int32_t* w_start, const int32_t* w_end, int64_t n_win, const ftk_filter* f,
               int32_t len_lo, int32_t n_bins, int64_t* k_out, int32_t* at_out, int64_t* n_out, int64_t* overflow_out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    int rc = check_ks_arguments(ctx, w_start, n_win, n_bins, k_out, n_out);
    if (rc) return rc;
    if (!w_end || !overflow_out) return fail(ctx, FTK_ERR_INVALID, "NULL pointer argument");
    ContigData* c;
    if ((rc = get_contig(ctx, contig_id, &c)) || (rc = check_filter(ctx, f, *c))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    KsFront k;
    Scratch front(ctx);
    k.declare(front, true, n_win, n_bins);
    // Behind the front the window pass keeps its own buffers (the plan of up to 4096 windows and the overflow column:
    // well under the MiB allowed for here), then the outputs take that place: reserved at once, so that the block holding
    // the rows does not move under either.
    if ((rc = reserve_scratch(ctx, front.bytes() + std::max<size_t>(ks_outputs_room(n_win), (size_t)1 << 20))) || (rc = front.place()))
        return rc;
    const void* block = ctx->scratch;
    FeatCall fc;
    fc.f = f;
    fc.hist_out = k.b_hist;  // device memory: the window pass writes the rows where they are
    fc.overflow_out = overflow_out;
    fc.len_lo = len_lo;
    fc.n_bins = n_bins;
    if ((rc = features_common(ctx, contig_id, w_start, w_end, n_win, fc, nullptr, nullptr, front.bytes()))) return rc;
    if (ctx->scratch != block) return fail(ctx, FTK_ERR_HIP, "the scratch block moved under the histogram rows");
    return ks_rows_then_pairs(ctx, k, front.bytes(), k.b_hist, n_win, n_bins, k_out, at_out, n_out);
}

}  // extern "C"
