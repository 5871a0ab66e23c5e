// Part of ftk_api.hip's translation unit (#included there behind the V-plot part) - the fragment-end profiles of a
// resident contig around sites, and the per-site window sums the OCF score is made of (`ftk_site_ends`), over the kernel
// of ftk_siteends.hip: the call checks its arguments, plans the sites as ftk_site_profile does (SitePlan, here with the
// caller's index of every sorted site), decides whether a run's two tracks share one workgroup, and launches one workgroup
// per run, or per (run, track).
#include "ftk_siteends.h"

extern "C" {

int ftk_site_ends(ftk_ctx* ctx, int contig_id, const int32_t* centre, const uint8_t* flip, const int32_t* group, int64_t n_sites,
                  int32_t n_groups, int32_t half_width, int32_t bin_size, int32_t mapq_min, int32_t min_len, int32_t max_len,
                  int use_weights, int32_t peak, int32_t flank, int64_t* sum_out, int64_t* count_out, int64_t* site_sum_out,
                  int64_t* site_count_out) {
    int n_bins = 0;
    int rc = check_site_axis(ctx, n_sites, centre, sum_out, half_width, bin_size, &n_bins);
    if (rc) return rc;
    if (n_groups < 1 || (int64_t)n_groups * 2 * n_bins > (1 << 28))
        return fail(ctx, FTK_ERR_INVALID, "n_groups %d out of range (n_groups * 2 * n_bins <= 2^28)", n_groups);
    const bool per_site = site_sum_out != nullptr;
    if (per_site) {
        if (peak < 1) return fail(ctx, FTK_ERR_INVALID, "peak %d out of range: at least 1", peak);
        if (flank < 0 || flank >= peak) return fail(ctx, FTK_ERR_INVALID, "flank %d out of range [0, peak = %d)", flank, peak);
        if ((int64_t)peak + flank >= half_width)
            return fail(ctx, FTK_ERR_INVALID, "peak + flank = %lld: below half_width = %d", (long long)peak + flank, half_width);
    }
    if (is_device_ptr(centre) || is_device_ptr(flip) || is_device_ptr(group))
        return fail(ctx, FTK_ERR_INVALID, "the sites must be host arrays");
    ContigData* c;
    if ((rc = get_contig(ctx, contig_id, &c))) return rc;
    if (use_weights && !c->weights) return no_weights(ctx, contig_id);
    SitePlan plan;
    if ((rc = plan.sort(ctx, centre, flip, group, n_sites, n_groups, per_site))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!ctx->siteends_lds) HIPCHK(ctx, siteends_lds_most(ctx->device, &ctx->siteends_lds));
    const ftk_filter f{mapq_min, min_len, max_len, FTK_POLICY_MIDPOINT, FTK_FETCH_TABIX};
    SiteEndsParams p{half_width, bin_size, n_bins, mapq_min, min_len < 0 ? INT32_MIN : min_len, max_len < 0 ? INT32_MAX : max_len,
                     eff_lmax(&f, *c), use_weights != 0, 0, per_site ? peak : 1, per_site ? flank : 0};
    // One workgroup per run up to the threshold, one per (run, track) above it.  FTK_SITE_ENDS_SPLIT=1 / =0 asks for the
    // split / the whole arrangement wherever the device can hold it - for tests of both, and for measuring one against the
    // other without a second build (docs/experiments.md, "site ends").
    const int whole = siteends_whole_bytes(n_bins, use_weights != 0);
    p.split = whole > kSiteEndsLdsBytes;
    if (const char* env = getenv("FTK_SITE_ENDS_SPLIT")) {
        if (env[0] == '1') p.split = 1;
        if (env[0] == '0') p.split = 0;
    }
    if (whole > ctx->siteends_lds) p.split = 1;
    plan.cut(n_sites > 0 && c->n > 0 ? siteends_run_sites(ctx->n_cu, n_sites, c->n, c->max_end, p) : 0);
    const size_t cells = (size_t)n_groups * 2 * (size_t)n_bins, site_cells = (size_t)n_sites * 4;
    int64_t *d_sum = nullptr, *d_cnt = nullptr, *d_ssum = nullptr, *d_scnt = nullptr;
    // (the kernel writes every site's row; the zeros of the per-site outputs are what a call without runs - an empty
    // contig - returns.  A split run is two workgroups.)
    return run_site_call(ctx, plan,
                         {{&d_sum, sum_out, cells},
                          {&d_cnt, count_out, cells},
                          {&d_ssum, site_sum_out, site_cells},
                          {&d_scnt, per_site ? site_count_out : nullptr, site_cells}},
                         p.split ? 2 : 1, [&](size_t r0, int part) {
                             launch_site_ends(ctx->stream, c->v, c->weights, plan.d_words, plan.d_order, plan.d_off + r0,
                                              plan.d_group + r0, part, p, (unsigned long long*)d_sum, (unsigned long long*)d_cnt,
                                              (unsigned long long*)d_ssum, (unsigned long long*)d_scnt);
                         });
}

}  // extern "C"
