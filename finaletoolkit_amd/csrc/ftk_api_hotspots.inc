// Part of ftk_api.hip's translation unit (#included there behind the preferred-ends part) - IFS hotspots:
// `ftk_ifs_hotspots`, `ftk_ifs_track` and `ftk_ifs_totals` over the kernels of ftk_hotspots.hip.  The hotspot call checks
// its arguments and hands its rule's pieces to run_tile_call, which walks the intervals' tiles of windows in batches and
// brings the called windows home.  The merge (rule 6) is one linear pass on the host over the called windows as they come
// home; the hotspot that is open at the end of a batch stays open into the next, so hotspots do not depend on where a
// batch or a tile ends.
#include "ftk_hotspots.h"

extern "C++" {  // (templates, in a file that is included inside ftk_api.hip's extern "C" block)
namespace {

// the windows of interval [a, b): k_lo .. k_hi (rule 2; none: k_hi < k_lo)
void ifs_interval_windows(int64_t a, int64_t b, int64_t chrom, int64_t s, int64_t m, int64_t n_bins, int64_t* k_lo, int64_t* k_hi) {
    *k_lo = (a + s - 1) / s;
    *k_hi = b == chrom ? n_bins - m : std::min(b / s - m, n_bins - m);
}

// what the three calls share: the ranges of chrom_size, step, m and mean_len, the contig, the filter
int ifs_open(ftk_ctx* ctx, int contig_id, int64_t chrom_size, int32_t step, int32_t m, int32_t mean_len, int32_t min_len,
             int32_t max_len, int32_t mapq_min, ContigData** c, IfsParams* p) {
    if (chrom_size < 0 || chrom_size >= (1LL << 30)) return fail(ctx, FTK_ERR_INVALID, "chrom_size %lld outside [0, 2^30)", (long long)chrom_size);
    if (step < 1 || step > 65535) return fail(ctx, FTK_ERR_INVALID, "step %d outside [1, 65535]", step);
    if (m < 1 || m > FTK_IFS_MAX_WINDOW_BINS) return fail(ctx, FTK_ERR_INVALID, "m %d outside [1, %d]", m, FTK_IFS_MAX_WINDOW_BINS);
    if (mean_len < 1 || mean_len > 65535) return fail(ctx, FTK_ERR_INVALID, "mean_len %d outside [1, 65535]", mean_len);
    int rc = get_contig(ctx, contig_id, c);
    if (rc) return rc;
    const CleaveParams cp = cleave_params(**c, min_len, max_len, mapq_min);
    *p = IfsParams{};
    p->chrom = (int)chrom_size;
    p->step = step;
    p->m = m;
    p->n_bins = (int)((chrom_size + step - 1) / step);
    p->L = (unsigned)mean_len;
    p->min_len = cp.min_len;
    p->max_len = cp.max_len;
    p->mapq_min = cp.mapq_min;
    p->lmax = cp.lmax;
    p->packed = call_reads_packed((*c)->v, p->mapq_min, p->min_len, p->max_len);
    return FTK_OK;
}

constexpr size_t kIfsWinSize[8] = {4, 8, 4, 8, 8, 4, 8, 4};     // run, pos, count, ifs, bg1, nb1, bg2, nb2
constexpr size_t kIfsHotSize[9] = {4, 8, 8, 4, 8, 8, 4, 8, 4};  // run, start, stop, n_windows, summit, ifs, count, bg1, nb1

// Rule 6 over the called windows in (run, pos) order, fed a stretch at a time.
struct IfsMerge {
    int64_t step, m, chrom, join, min_windows;
    HostCols<9> hot{kIfsHotSize};
    int64_t* sums;  // [n_iv][6]
    bool open = false;
    int32_t run = 0, n = 0, best_count = 0, best_nb1 = 0;
    int64_t k_first = 0, k_last = 0, best_pos = 0, best_ifs = 0, best_bg1 = 0;
    int32_t cover_run = -1;  // the run whose kept hotspots reach cover_stop
    int64_t cover_stop = 0;

    bool close() {
        if (!open) return true;
        open = false;
        int64_t* st = sums + (size_t)run * 6;
        if (n < min_windows) {
            ++st[4];
            return true;
        }
        const int64_t start = k_first * step, stop = std::min((k_last + m) * step, chrom);
        ++st[3];
        st[5] += stop - (cover_run == run ? std::max(start, cover_stop) : start);  // (stops grow with the starts)
        cover_run = run;
        cover_stop = stop;
        if (!hot.grow(1)) return false;
        const int64_t j = hot.n++;
        hot.col<int32_t>(0)[j] = run;
        hot.col<int64_t>(1)[j] = start;
        hot.col<int64_t>(2)[j] = stop;
        hot.col<int32_t>(3)[j] = n;
        hot.col<int64_t>(4)[j] = best_pos;
        hot.col<int64_t>(5)[j] = best_ifs;
        hot.col<int32_t>(6)[j] = best_count;
        hot.col<int64_t>(7)[j] = best_bg1;
        hot.col<int32_t>(8)[j] = best_nb1;
        return true;
    }
    bool feed(const int32_t* w_run, const int64_t* w_pos, const int32_t* w_count, const int64_t* w_ifs, const int64_t* w_bg1,
              const int32_t* w_nb1, int64_t from, int64_t to) {
        for (int64_t j = from; j < to; ++j) {
            const int64_t k = w_pos[j] / step;
            if (open && (w_run[j] != run || k - k_last > join) && !close()) return false;
            if (!open) {
                open = true;
                run = w_run[j];
                n = 0;
                k_first = k;
            }
            if (n == 0 || w_ifs[j] < best_ifs) {
                best_pos = w_pos[j];
                best_ifs = w_ifs[j];
                best_count = w_count[j];
                best_bg1 = w_bg1[j];
                best_nb1 = w_nb1[j];
            }
            ++n;
            k_last = k;
        }
        return true;
    }
};

}  // namespace
}  // extern "C++"

extern "C" {

int ftk_ifs_hotspots(ftk_ctx* ctx, int contig_id, const int64_t* iv_start, const int64_t* iv_stop, int64_t n_iv, int64_t chrom_size,
                     int32_t step, int32_t m, int32_t mean_len, int32_t h1, int32_t h2, int32_t min_count, const uint64_t* thr,
                     int32_t n_thr, int64_t global_mean, int32_t join, int32_t min_windows, int32_t min_len, int32_t max_len,
                     int32_t mapq_min, int32_t** w_run, int64_t** w_pos, int32_t** w_count, int64_t** w_ifs, int64_t** w_bg1,
                     int32_t** w_nb1, int64_t** w_bg2, int32_t** w_nb2, int64_t* n_windows, int32_t** h_run, int64_t** h_start,
                     int64_t** h_stop, int32_t** h_n_windows, int64_t** h_summit, int64_t** h_ifs, int32_t** h_count,
                     int64_t** h_bg1, int32_t** h_nb1, int64_t* n_hotspots, int64_t* stats) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    void** const wout[8] = {(void**)w_run, (void**)w_pos, (void**)w_count, (void**)w_ifs, (void**)w_bg1, (void**)w_nb1, (void**)w_bg2, (void**)w_nb2};
    void** const hout[9] = {(void**)h_run, (void**)h_start, (void**)h_stop, (void**)h_n_windows, (void**)h_summit, (void**)h_ifs, (void**)h_count, (void**)h_bg1, (void**)h_nb1};
    for (void** q : wout)
        if (!q) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    for (void** q : hout)
        if (!q) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    if (!n_windows || !n_hotspots) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    for (void** q : wout) *q = nullptr;
    for (void** q : hout) *q = nullptr;
    *n_windows = *n_hotspots = 0;
    if (h1 < 1) return fail(ctx, FTK_ERR_INVALID, "h1 %d below 1", h1);
    if (h2 != 0 && h2 < h1) return fail(ctx, FTK_ERR_INVALID, "h2 %d is neither 0 nor at least h1 (%d)", h2, h1);
    if (m >= 1 && m <= FTK_IFS_MAX_WINDOW_BINS && (int64_t)std::max(h1, h2) + m > FTK_IFS_MAX_REACH)
        return fail(ctx, FTK_ERR_INVALID, "max(h1, h2) + m = %lld exceeds %d", (long long)std::max(h1, h2) + m, FTK_IFS_MAX_REACH);
    if (min_count < 0) return fail(ctx, FTK_ERR_INVALID, "min_count %d below 0", min_count);
    if (n_thr < 1 || n_thr > FTK_IFS_MAX_THR) return fail(ctx, FTK_ERR_INVALID, "n_thr %d outside [1, %d]", n_thr, FTK_IFS_MAX_THR);
    if (global_mean < 0) return fail(ctx, FTK_ERR_INVALID, "global_mean is negative");
    if (join < 1 || join > FTK_IFS_MAX_JOIN) return fail(ctx, FTK_ERR_INVALID, "join %d outside [1, %d]", join, FTK_IFS_MAX_JOIN);
    if (min_windows < 1) return fail(ctx, FTK_ERR_INVALID, "min_windows %d below 1", min_windows);
    if (n_iv < 0 || n_iv > INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "n_iv out of range");
    if (!thr || (n_iv > 0 && (!iv_start || !iv_stop || !stats))) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    if (is_device_ptr(thr) || is_device_ptr(iv_start) || is_device_ptr(iv_stop) || is_device_ptr(stats))
        return fail(ctx, FTK_ERR_INVALID, "interval, threshold and stats arrays must be host arrays");
    for (int k = 0; k < n_thr; ++k)
        if (thr[k] >= (1ULL << 32)) return fail(ctx, FTK_ERR_INVALID, "threshold %d reaches 2^32", k);
    ContigData* c;
    IfsParams p{};
    int rc = check_intervals_in_contig(ctx, iv_start, iv_stop, n_iv, chrom_size);
    if (rc) return rc;
    if ((rc = ifs_open(ctx, contig_id, chrom_size, step, m, mean_len, min_len, max_len, mapq_min, &c, &p))) return rc;
    p.h1 = h1;
    p.h2 = h2;
    p.reach = std::max(h1, h2);
    p.min_count = (unsigned)min_count;
    p.n_thr = n_thr;
    p.global_mean = (unsigned long long)global_mean;
    HIPCHK(ctx, hipSetDevice(ctx->device));

    const std::vector<uint32_t> thr32(thr, thr + n_thr);
    std::vector<int64_t> sums((size_t)n_iv * 6, 0);
    HostCols<8> home{kIfsWinSize};
    IfsMerge merge{step, m, chrom_size, join, min_windows};
    merge.sums = sums.data();
    rc = run_tile_call(
        ctx, thr32.data(), (size_t)n_thr * 4, kIfsStats, 1, home,
        [&](const void* d_thr, int nt, const TileCallPlan& pl) {
            p.thr = static_cast<const unsigned*>(d_thr);
            launch_ifs_count(ctx->stream, c->v, p, nt, pl);
        },
        [&](int nt, const TileCallPlan& pl, void* const* col) {
            IfsOut o{};
            o.run = (int32_t*)col[0];
            o.pos = (int64_t*)col[1];
            o.count = (int32_t*)col[2];
            o.ifs = (int64_t*)col[3];
            o.bg1 = (int64_t*)col[4];
            o.nb1 = (int32_t*)col[5];
            o.bg2 = (int64_t*)col[6];
            o.nb2 = (int32_t*)col[7];
            launch_ifs_write(ctx->stream, c->v, p, nt, pl, o);
        },
        [&](int32_t iv, int32_t len, const uint32_t* ts) {
            int64_t* st = &sums[(size_t)iv * 6];
            st[0] += len;
            st[1] += ts[0];
            st[2] += ts[1];
            return (int64_t)ts[1];
        },
        [&](int64_t from, int64_t to) {
            return merge.feed(home.col<int32_t>(0), home.col<int64_t>(1), home.col<int32_t>(2), home.col<int64_t>(3), home.col<int64_t>(4),
                              home.col<int32_t>(5), from, to);
        },
        [&](auto&& push_tile) {
            for (int64_t i = 0; i < n_iv; ++i) {
                int64_t k_lo, k_hi;
                ifs_interval_windows(iv_start[i], iv_stop[i], chrom_size, step, m, p.n_bins, &k_lo, &k_hi);
                for (int64_t a = k_lo; a <= k_hi; a += kCallTile)
                    if (int e = push_tile(a, std::min<int64_t>(k_hi + 1 - a, kCallTile), i)) return e;
            }
            return (int)FTK_OK;
        });
    if (rc) return rc;
    if (!merge.close()) return fail(ctx, FTK_ERR_OOM, "out of host memory");
    if (n_iv > 0) memcpy(stats, sums.data(), sums.size() * 8);
    home.give(wout, n_windows);
    merge.hot.give(hout, n_hotspots);
    return FTK_OK;
}

int ftk_ifs_track(ftk_ctx* ctx, int contig_id, const int64_t* iv_start, const int64_t* iv_stop, int64_t n_iv,
                  const int64_t* out_offset, int64_t chrom_size, int32_t step, int32_t m, int32_t mean_len, int32_t min_len,
                  int32_t max_len, int32_t mapq_min, int32_t* n_out, int64_t* ifs_out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (n_iv < 0 || n_iv > INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "n_iv out of range");
    if (n_iv > 0 && (!iv_start || !iv_stop || !out_offset)) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    if (is_device_ptr(iv_start) || is_device_ptr(iv_stop) || is_device_ptr(out_offset))
        return fail(ctx, FTK_ERR_INVALID, "interval and offset arrays must be host arrays");
    ContigData* c;
    IfsParams p{};
    int rc = check_intervals_in_contig(ctx, iv_start, iv_stop, n_iv, chrom_size);
    if (rc) return rc;
    if ((rc = ifs_open(ctx, contig_id, chrom_size, step, m, mean_len, min_len, max_len, mapq_min, &c, &p))) return rc;
    std::vector<int32_t> t0, tlen;  // (pageable staging: finish(true) waits for the uploads)
    std::vector<int64_t> tout;
    int64_t total = 0;
    for (int64_t i = 0; i < n_iv; ++i) {
        int64_t k_lo, k_hi;
        ifs_interval_windows(iv_start[i], iv_stop[i], chrom_size, step, m, p.n_bins, &k_lo, &k_hi);
        if (out_offset[i] < 0) return fail(ctx, FTK_ERR_INVALID, "out_offset[%lld] is negative", (long long)i);
        if (k_hi < k_lo) continue;
        total = std::max(total, out_offset[i] + (k_hi + 1 - k_lo));
        for (int64_t a = k_lo; a <= k_hi; a += kCallTile) {
            t0.push_back((int32_t)a);
            tlen.push_back((int32_t)std::min<int64_t>(k_hi + 1 - a, kCallTile));
            tout.push_back(out_offset[i] + (a - k_lo));
        }
    }
    if (t0.empty()) return FTK_OK;
    if (!n_out || !ifs_out) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    if (t0.size() > (size_t)INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "too many tiles");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nt = t0.size();
    SyncOnExit wait{ctx};
    Scratch s(ctx);
    IfsOut o{};
    int32_t *d_t0 = nullptr, *d_len = nullptr;
    int64_t* d_out = nullptr;
    s.out(&o.n_out, n_out, (size_t)total);
    s.out(&o.ifs_out, ifs_out, (size_t)total);
    s.tmp(&d_t0, nt);
    s.tmp(&d_len, nt);
    s.tmp(&d_out, nt);
    if ((rc = s.reserve())) return rc;
    // (windows that no interval owns stay as the caller left them only in a device array: a host array is copied back
    // whole, so the gaps of its stand-in are cleared first)
    if (!is_device_ptr(n_out)) HIPCHK(ctx, hipMemsetAsync(o.n_out, 0, (size_t)total * 4, ctx->stream));
    if (!is_device_ptr(ifs_out)) HIPCHK(ctx, hipMemsetAsync(o.ifs_out, 0, (size_t)total * 8, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_t0, t0.data(), nt * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_len, tlen.data(), nt * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_out, tout.data(), nt * 8, hipMemcpyHostToDevice, ctx->stream));
    TileCallPlan pl{};
    pl.tile_t0 = d_t0;
    pl.tile_len = d_len;
    pl.tile_out = d_out;
    launch_ifs_track(ctx->stream, c->v, p, (long long)nt, pl, o);
    HIPCHK(ctx, hipGetLastError());
    return s.finish(/*must_sync=*/true);
}

int ftk_ifs_totals(ftk_ctx* ctx, int contig_id, int64_t chrom_size, int32_t min_len, int32_t max_len, int32_t mapq_min,
                   int64_t* n_frags, int64_t* len_sum) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (!n_frags || !len_sum) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    ContigData* c;
    IfsParams p{};
    int rc = ifs_open(ctx, contig_id, chrom_size, 1, 1, 1, min_len, max_len, mapq_min, &c, &p);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = reserve_scratch(ctx, align_up((size_t)kIfsTotalsBlocks * 16)))) return rc;
    Arena a(ctx);
    unsigned long long* d = a.take<unsigned long long>((size_t)kIfsTotalsBlocks * 2);
    launch_ifs_totals(ctx->stream, c->v, p, d);
    HIPCHK(ctx, hipGetLastError());
    std::vector<unsigned long long> part((size_t)kIfsTotalsBlocks * 2);
    HIPCHK(ctx, hipMemcpyAsync(part.data(), d, part.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    int64_t n = 0, sum = 0;
    for (int b = 0; b < kIfsTotalsBlocks; ++b) {
        n += (int64_t)part[2 * b];
        sum += (int64_t)part[2 * b + 1];
    }
    *n_frags = n;
    *len_sum = sum;
    return FTK_OK;
}

}  // extern "C"
