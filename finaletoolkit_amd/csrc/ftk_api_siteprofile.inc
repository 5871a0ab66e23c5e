// Part of ftk_api.hip's translation unit (#included there behind the weights part) - the site-aggregated midpoint
// profile of a resident contig (`ftk_site_profile`) over the kernel of ftk_siteprofile.hip: the call checks its
// arguments, sorts the sites by (group, centre), cuts them into runs of one group each and launches one workgroup per run.
// The checks of the site list and of the offset axis, the plan of runs and the call's tail are shared with ftk_site_vplot
// (ftk_api_vplot.inc) and ftk_site_ends (ftk_api_siteends.inc).
#include "ftk_siteprofile.h"

namespace {

// The checks every site call starts with, in this order: the context, the site count, the pointers, the offset axis.
int check_site_axis(ftk_ctx* ctx, int64_t n_sites, const int32_t* centre, const int64_t* sum_out, int32_t half_width,
                    int32_t bin_size, int* n_bins) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (n_sites < 0 || n_sites > INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "n_sites out of range");
    if (n_sites > 0 && !centre) return fail(ctx, FTK_ERR_INVALID, "NULL centre pointer");
    if (!sum_out) return fail(ctx, FTK_ERR_INVALID, "sum_out is NULL");
    if (half_width < 1 || half_width > kSiteMaxHalfWidth)
        return fail(ctx, FTK_ERR_INVALID, "half_width %d out of range [1, %d]", half_width, kSiteMaxHalfWidth);
    if (bin_size < 1 || (2 * half_width) % bin_size != 0)
        return fail(ctx, FTK_ERR_INVALID, "bin_size %d does not divide 2 * half_width = %d", bin_size, 2 * half_width);
    *n_bins = 2 * half_width / bin_size;
    if (*n_bins > kSiteMaxBins) return fail(ctx, FTK_ERR_INVALID, "%d bins: at most %d", *n_bins, kSiteMaxBins);
    return FTK_OK;
}

// The sites of one call as the kernels take them: 32-bit words sorted by (group, centre), cut into runs that stay inside
// one group; and their temporaries in the call's scratch.
struct SitePlan {
    std::vector<uint64_t> keys;   // group, then centre, then the flip flag (which takes no part in the order that matters)
    std::vector<uint32_t> words;  // the centre with the flip flag on top (kSiteFlipBit), in key order
    std::vector<int32_t> run_off, run_group;
    std::vector<int32_t> order;   // optional (sort's keep_order): the caller's index of every sorted site; else empty
    uint32_t* d_words = nullptr;
    int32_t *d_off = nullptr, *d_group = nullptr, *d_order = nullptr;
    size_t n_runs() const { return run_group.size(); }

    // checks every site and sorts them; keep_order: `order` is filled too (equal keys in the caller's order)
    int sort(ftk_ctx* ctx, const int32_t* centre, const uint8_t* flip, const int32_t* group, int64_t n_sites, int32_t n_groups,
             bool keep_order = false) {
        keys.resize((size_t)n_sites);
        for (int64_t i = 0; i < n_sites; ++i) {
            const int32_t g = group ? group[i] : 0;
            if (centre[i] < 0 || centre[i] >= kPadCoord)
                return fail(ctx, FTK_ERR_INVALID, "site %lld: centre %d outside [0, 2^30)", (long long)i, centre[i]);
            if (g < 0 || g >= n_groups)
                return fail(ctx, FTK_ERR_INVALID, "site %lld: group %d outside [0, %d)", (long long)i, g, n_groups);
            keys[(size_t)i] = (uint64_t)g << 32 | (uint64_t)centre[i] << 1 | (uint64_t)(flip && flip[i]);
        }
        if (keep_order) {
            const std::vector<uint64_t> given = keys;
            order.resize((size_t)n_sites);
            for (int64_t i = 0; i < n_sites; ++i) order[(size_t)i] = (int32_t)i;
            std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return given[(size_t)a] < given[(size_t)b]; });
            for (int64_t i = 0; i < n_sites; ++i) keys[(size_t)i] = given[(size_t)order[(size_t)i]];
            return FTK_OK;
        }
        std::sort(keys.begin(), keys.end());
        return FTK_OK;
    }
    // runs: at most per_run sites, never across a group's end (per_run <= 0: no runs - an empty contig)
    void cut(long long per_run) {
        const int64_t n_sites = (int64_t)keys.size();
        words.resize(keys.size());
        if (n_sites == 0 || per_run <= 0) return;
        for (int64_t i = 0; i < n_sites; ++i) {
            const int32_t g = (int32_t)(keys[(size_t)i] >> 32);
            if (run_group.empty() || g != run_group.back() || i - run_off.back() >= per_run) {
                run_off.push_back((int32_t)i);
                run_group.push_back(g);
            }
            const uint32_t low = (uint32_t)keys[(size_t)i];
            words[(size_t)i] = low >> 1 | ((low & 1u) ? kSiteFlipBit : 0u);
        }
        run_off.push_back((int32_t)n_sites);
    }
    // (in front of the call's outputs; the plan must not move between this and Scratch::reserve)
    void declare(Scratch& s) {
        if (!n_runs()) return;
        s.tmp(&d_words, words.size());
        s.tmp(&d_off, n_runs() + 1);
        s.tmp(&d_group, n_runs());
        if (!order.empty()) s.tmp(&d_order, order.size());
    }
    // the uploads read the vectors above (pageable): the caller waits for the stream on every way out
    int upload(ftk_ctx* ctx) {
        HIPCHK(ctx, hipMemcpyAsync(d_words, words.data(), words.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_off, run_off.data(), (n_runs() + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_group, run_group.data(), n_runs() * 4, hipMemcpyHostToDevice, ctx->stream));
        if (d_order) HIPCHK(ctx, hipMemcpyAsync(d_order, order.data(), order.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        return FTK_OK;
    }
};

// The tail every site call ends with: the outputs and the plan get their place in the scratch, the outputs are zeroed,
// the plan goes up, and launch(r0, part) is called for runs [r0, r0 + part) - at most kSiteMaxRunsPerLaunch workgroups
// per launch, a run being groups_per_run of them, so that a grid of any workgroup size stays below 2^32 threads.
template <class Launch>
int run_site_call(ftk_ctx* ctx, SitePlan& plan, std::initializer_list<CellsOut> outs, size_t groups_per_run, Launch&& launch) {
    Scratch s(ctx);
    plan.declare(s);
    int rc;
    if ((rc = s.reserve_zeroed(outs))) return rc;
    // From here on the stream may be reading the plan's vectors (pageable staging of this call): every way out, an
    // error's included, waits for the stream first.
    auto enqueue = [&]() -> int {
        const size_t n_runs = plan.n_runs();
        if (!n_runs) return FTK_OK;
        if (int e = plan.upload(ctx)) return e;
        const size_t per_launch = std::max<size_t>((size_t)kSiteMaxRunsPerLaunch / groups_per_run, 1);
        for (size_t r0 = 0; r0 < n_runs; r0 += per_launch) {
            launch(r0, (int)std::min(n_runs - r0, per_launch));
            HIPCHK(ctx, hipGetLastError());
        }
        return FTK_OK;
    };
    if ((rc = enqueue())) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    if ((rc = s.finish(true))) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

}  // namespace

extern "C" {

int ftk_site_profile(ftk_ctx* ctx, int contig_id, const int32_t* centre, const uint8_t* flip, const int32_t* group, int64_t n_sites,
                     int32_t n_groups, int32_t half_width, int32_t bin_size, int32_t mapq_min, int32_t min_len, int32_t max_len,
                     int use_weights, int64_t* sum_out, int64_t* count_out) {
    int n_bins = 0;
    int rc = check_site_axis(ctx, n_sites, centre, sum_out, half_width, bin_size, &n_bins);
    if (rc) return rc;
    if (n_groups < 1 || (int64_t)n_groups * n_bins > (1 << 28))
        return fail(ctx, FTK_ERR_INVALID, "n_groups %d out of range (n_groups * n_bins <= 2^28)", n_groups);
    if (is_device_ptr(centre) || is_device_ptr(flip) || is_device_ptr(group))
        return fail(ctx, FTK_ERR_INVALID, "the sites must be host arrays");
    ContigData* c;
    if ((rc = get_contig(ctx, contig_id, &c))) return rc;
    if (use_weights && !c->weights) return no_weights(ctx, contig_id);
    SitePlan plan;
    if ((rc = plan.sort(ctx, centre, flip, group, n_sites, n_groups))) return rc;
    const ftk_filter f{mapq_min, min_len, max_len, FTK_POLICY_MIDPOINT, FTK_FETCH_TABIX};
    const SiteProfileParams p{half_width, bin_size, n_bins, mapq_min, min_len < 0 ? INT32_MIN : min_len,
                              max_len < 0 ? INT32_MAX : max_len, eff_lmax(&f, *c), use_weights != 0};
    plan.cut(n_sites > 0 && c->n > 0 ? site_run_sites(ctx->n_cu, n_sites, c->n, c->max_end, p) : 0);
    const size_t cells = (size_t)n_groups * (size_t)n_bins;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int64_t *d_sum = nullptr, *d_cnt = nullptr;
    return run_site_call(ctx, plan, {{&d_sum, sum_out, cells}, {&d_cnt, count_out, cells}}, 1, [&](size_t r0, int part) {
        launch_site_profile(ctx->stream, c->v, c->weights, plan.d_words, plan.d_off + r0, plan.d_group + r0, part, p,
                            (unsigned long long*)d_sum, (unsigned long long*)d_cnt);
    });
}

}  // extern "C"
