// Part of ftk_api.hip's translation unit (#included there behind the site-profile part) - the fragment length x
// midpoint offset map of a resident contig around sites (`ftk_site_vplot`) over the kernel of ftk_vplot.hip: the call
// checks its arguments, plans the sites as ftk_site_profile does (SitePlan), splits the rows into the tiles the LDS
// budget holds and launches one workgroup per (run, tile).
#include "ftk_vplot.h"

extern "C" {

int ftk_site_vplot(ftk_ctx* ctx, int contig_id, const int32_t* centre, const uint8_t* flip, const int32_t* group, int64_t n_sites,
                   int32_t n_groups, int32_t half_width, int32_t bin_size, int32_t len_lo, int32_t len_hi, int32_t len_bin,
                   int32_t mapq_min, int use_weights, int64_t* sum_out, int64_t* count_out) {
    int n_bins = 0;
    int rc = check_site_axis(ctx, n_sites, centre, sum_out, half_width, bin_size, &n_bins);
    if (rc) return rc;
    if (len_lo < 0 || len_hi < len_lo || len_hi > kVplotMaxLen)
        return fail(ctx, FTK_ERR_INVALID, "len_lo %d, len_hi %d out of range (0 <= len_lo <= len_hi <= %d)", len_lo, len_hi, kVplotMaxLen);
    if (len_bin < 1 || (len_hi - len_lo + 1) % len_bin != 0)
        return fail(ctx, FTK_ERR_INVALID, "len_bin %d does not divide len_hi - len_lo + 1 = %d", len_bin, len_hi - len_lo + 1);
    const int n_rows = (len_hi - len_lo + 1) / len_bin;
    if (n_rows > kVplotMaxRows) return fail(ctx, FTK_ERR_INVALID, "%d rows: at most %d", n_rows, kVplotMaxRows);
    if (n_groups < 1 || (int64_t)n_groups * n_rows * n_bins > (1 << 28))
        return fail(ctx, FTK_ERR_INVALID, "n_groups %d out of range (n_groups * n_rows * n_bins <= 2^28)", n_groups);
    if (is_device_ptr(centre) || is_device_ptr(flip) || is_device_ptr(group))
        return fail(ctx, FTK_ERR_INVALID, "the sites must be host arrays");
    ContigData* c;
    if ((rc = get_contig(ctx, contig_id, &c))) return rc;
    if (use_weights && !c->weights) return no_weights(ctx, contig_id);
    SitePlan plan;
    if ((rc = plan.sort(ctx, centre, flip, group, n_sites, n_groups))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!ctx->vplot_lds) HIPCHK(ctx, vplot_lds_budget(ctx->device, &ctx->vplot_lds));
    VplotParams p{half_width, bin_size, n_bins, len_lo, len_hi, len_bin, n_rows, 0, mapq_min, std::max(c->max_len, 0), use_weights != 0};
    p.tile_rows = vplot_tile_rows(ctx->vplot_lds, n_rows, n_bins, use_weights != 0);
    plan.cut(n_sites > 0 && c->n > 0 ? vplot_run_sites(ctx->n_cu, n_sites, c->n, c->max_end, p) : 0);
    const size_t cells = (size_t)n_groups * (size_t)n_rows * (size_t)n_bins;
    int64_t *d_sum = nullptr, *d_cnt = nullptr;
    // (a run is one workgroup per tile)
    return run_site_call(ctx, plan, {{&d_sum, sum_out, cells}, {&d_cnt, count_out, cells}}, (size_t)vplot_tiles(p),
                         [&](size_t r0, int part) {
                             launch_site_vplot(ctx->stream, c->v, c->weights, plan.d_words, plan.d_off + r0, plan.d_group + r0, part, p,
                                               (unsigned long long*)d_sum, (unsigned long long*)d_cnt);
                         });
}

}  // extern "C"
