// Part of ftk_api.hip's translation unit (#included there last) - the write direction: `ftk_frags_format_rows`,
// `ftk_bgzf_deflate_device`, `ftk_frags_write` and their region-mask forms over the kernels of ftk_fragtext.hip.
#include "ftk_fragtext.h"

namespace {

// One contig's rows as device text: everything format_contig leaves in the ctx scratch.
struct ExportText {
    RowAgg total{};
    uint8_t* d_text = nullptr;
    int32_t* d_run_bin = nullptr;
    uint32_t* d_run_off = nullptr;
    uint32_t* d_lin = nullptr;
    int64_t n_runs = 0;
    int32_t n_lin = 0;
    DeflateScratch ds{};
    int64_t n_blocks = 0;
};

size_t deflate_scratch_bytes(int64_t n) {
    const size_t nb = (size_t)bgzf_blocks(n);
    const size_t lanes = (size_t)deflate_lanes((int64_t)nb);
    return align_up(nb * kBgzfSlot) + 2 * align_up(nb * 4) + align_up(nb * sizeof(InflateBlock)) +
           align_up(lanes * kDeflateHash * 4) + align_up(lanes * kDeflateTokens * 4) + align_up((nb + 1) * 8) +
           align_up(nb * (size_t)(kBgzfData + 31) + 64);
}

void take_deflate_scratch(Arena& a, int64_t n, DeflateScratch* ds) {
    const size_t nb = (size_t)bgzf_blocks(n);
    const size_t lanes = (size_t)deflate_lanes((int64_t)nb);
    ds->slots = a.take<uint8_t>(nb * kBgzfSlot);
    ds->sizes = a.take<uint32_t>(nb);
    ds->crc = a.take<uint32_t>(nb);
    ds->tab = a.take<InflateBlock>(nb);
    ds->hash = a.take<uint32_t>(lanes * kDeflateHash);
    ds->tokens = a.take<uint32_t>(lanes * kDeflateTokens);
    ds->offs = a.take<unsigned long long>(nb + 1);
    ds->out = a.take<uint8_t>(nb * (size_t)(kBgzfData + 31) + 64);
}

int row_params(ftk_ctx* ctx, const char* name, int32_t mapq_min, int32_t min_len, int32_t max_len, int layout, RowParams* p) {
    if (layout != kLayoutFrag && layout != kLayoutBed6 && layout != kLayoutBed3)
        return fail(ctx, FTK_ERR_INVALID, "unknown row layout %d", layout);
    const size_t nl = name ? strlen(name) : 0;
    if (nl == 0 || nl > 255) return fail(ctx, FTK_ERR_INVALID, "contig name must hold 1..255 bytes");
    memset(p, 0, sizeof(*p));
    p->mapq_min = mapq_min;
    p->min_len = min_len < 0 ? -1 : min_len;
    p->max_len = max_len < 0 ? -1 : max_len;
    p->layout = layout;
    p->name_len = (int32_t)nl;
    memcpy(p->name, name, nl);
    return FTK_OK;
}

// A caller's region mask, checked and laid out the way the kernel reads it: four arrays (whitelist starts / ends,
// blacklist starts / ends) in one host block, each padded to a multiple of four entries (starts with INT32_MAX, ends
// with 0) and starting on a 256-byte boundary, so that one copy puts them into the scratch arena.
struct MaskPack {
    std::vector<int32_t> host;
    size_t off[4] = {0, 0, 0, 0};  // in entries
    int32_t n_wl = -1, n_bl = 0, policy = FTK_POLICY_MIDPOINT;
    MaskView view(const int32_t* dev) const {
        return MaskView{dev + off[0], dev + off[1], n_wl, dev + off[2], dev + off[3], n_bl, policy};
    }
};

int mask_check(ftk_ctx* ctx, const char* what, const int32_t* s, const int32_t* e, int64_t n) {
    if (n > (int64_t(1) << 30)) return fail(ctx, FTK_ERR_INVALID, "%s holds too many intervals (%lld)", what, (long long)n);
    if (n > 0 && (!s || !e)) return fail(ctx, FTK_ERR_INVALID, "%s arrays are NULL", what);
    for (int64_t k = 0; k < n; ++k) {
        if (s[k] >= e[k]) return fail(ctx, FTK_ERR_INVALID, "%s interval %lld: start %d >= end %d", what, (long long)k, s[k], e[k]);
        if (k && s[k] < e[k - 1])
            return fail(ctx, FTK_ERR_INVALID, "%s interval %lld starts at %d, inside or in front of its predecessor (end %d): "
                        "the intervals must be sorted and disjoint", what, (long long)k, s[k], e[k - 1]);
    }
    return FTK_OK;
}

int mask_pack(ftk_ctx* ctx, const ftk_region_mask* m, MaskPack* p) {
    if (m->policy != FTK_POLICY_MIDPOINT && m->policy != FTK_POLICY_ANY)
        return fail(ctx, FTK_ERR_INVALID, "region masks take FTK_POLICY_MIDPOINT or FTK_POLICY_ANY, not %d", m->policy);
    const int64_t n_wl = m->n_wl < 0 ? -1 : m->n_wl, n_bl = m->n_bl <= 0 ? 0 : m->n_bl;
    int rc = mask_check(ctx, "whitelist", m->wl_start, m->wl_end, n_wl);
    if (!rc) rc = mask_check(ctx, "blacklist", m->bl_start, m->bl_end, n_bl);
    if (rc) return rc;
    p->n_wl = (int32_t)n_wl;
    p->n_bl = (int32_t)n_bl;
    p->policy = m->policy;
    const int32_t* src[4] = {m->wl_start, m->wl_end, m->bl_start, m->bl_end};
    const int64_t cnt[4] = {n_wl < 0 ? 0 : n_wl, n_wl < 0 ? 0 : n_wl, n_bl, n_bl};
    size_t total = 0;
    for (int a = 0; a < 4; ++a) {
        p->off[a] = total;
        total += align_up(((size_t)cnt[a] + 3) / 4 * 4 * sizeof(int32_t) + 16) / sizeof(int32_t);
    }
    p->host.assign(total, 0);
    for (int a = 0; a < 4; ++a) {
        int32_t* dst = p->host.data() + p->off[a];
        if (cnt[a]) memcpy(dst, src[a], (size_t)cnt[a] * sizeof(int32_t));
        if (!(a & 1))
            for (size_t k = (size_t)cnt[a]; k < ((size_t)cnt[a] + 3) / 4 * 4 + 4; ++k) dst[k] = INT32_MAX;
    }
    return FTK_OK;
}

// Format contig `c` into the scratch (stream-ordered; total is on the host when this returns).  with_deflate reserves
// the BGZF scratch behind the text in the same arena.  mk (may be NULL): the region mask - its intervals are copied
// in and its keep bitmap written in front of pass 1, again if the scratch moves.
int format_contig(ftk_ctx* ctx, ContigData* c, const RowParams& p, bool with_deflate, const MaskPack* mk, ExportText* x) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t n = c->n;
    const size_t mask_bytes = mk ? align_up(mk->host.size() * sizeof(int32_t)) + align_up(mask_words(n) * 8 + 8) : 0;
    const size_t agg_bytes = format_agg_bytes(n) + mask_bytes;
    const size_t nb = (size_t)((n + kRowsPerBlock - 1) / kRowsPerBlock);
    int rc = reserve_scratch(ctx, agg_bytes);
    if (rc) return rc;
    RowAgg *d_agg = nullptr, *d_pre = nullptr, *d_total = nullptr;
    int32_t* d_mask = nullptr;
    unsigned long long* d_bits = nullptr;
    auto carve = [&](Arena& a) {
        d_agg = a.take<RowAgg>(nb + 1);
        d_pre = a.take<RowAgg>(nb + 1);
        d_total = d_pre + nb;
        if (mk) {
            d_mask = a.take<int32_t>(mk->host.size());
            d_bits = a.take<unsigned long long>(mask_words(n) + 1);
        }
    };
    auto pass1 = [&]() -> int {
        Arena a(ctx);
        carve(a);
        if (mk) {  // (the caller's MaskPack outlives the stream synchronisation below)
            HIPCHK(ctx, hipMemcpyAsync(d_mask, mk->host.data(), mk->host.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
            mask_keep(ctx->stream, c->v.start, c->v.end, n, mk->view(d_mask), d_bits);
            HIPCHK(ctx, hipGetLastError());
        }
        format_pass1(ctx->stream, c->v.start, c->v.end, c->v.mapq, n, p, d_agg, d_pre, d_total, d_bits);
        HIPCHK(ctx, hipGetLastError());
        return FTK_OK;
    };
    if ((rc = pass1())) return rc;
    HIPCHK(ctx, hipMemcpyAsync(&x->total, d_total, sizeof(RowAgg), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const RowAgg& t = x->total;
    if (t.bytes >= (1ull << 32) - 65536ull)
        return fail(ctx, FTK_ERR_INVALID, "a contig's text must stay below 4 GB (%llu bytes)", t.bytes);
    x->n_runs = t.rows ? (int64_t)t.runs + 1 : 0;
    x->n_lin = t.rows ? t.max_win + 1 : 0;
    x->n_blocks = bgzf_blocks((int64_t)t.bytes);
    const void* before = ctx->scratch;
    rc = reserve_scratch(ctx, agg_bytes + align_up((size_t)t.bytes + 64) + 2 * align_up((size_t)x->n_runs * 4 + 4) +
                                  align_up((size_t)x->n_lin * 4 + 4) + (with_deflate ? deflate_scratch_bytes((int64_t)t.bytes) : 0) + 4096);
    if (rc) return rc;
    if (ctx->scratch != before) {  // the scratch moved: the prefixes (and the mask) went with the old block
        if ((rc = pass1())) return rc;
        if (mk) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (the copy reads the caller's host block)
    }
    Arena a(ctx);
    carve(a);
    x->d_text = a.take<uint8_t>((size_t)t.bytes + 64);
    x->d_run_bin = a.take<int32_t>((size_t)x->n_runs + 1);
    x->d_run_off = a.take<uint32_t>((size_t)x->n_runs + 1);
    x->d_lin = a.take<uint32_t>((size_t)x->n_lin + 1);
    if (with_deflate) take_deflate_scratch(a, (int64_t)t.bytes, &x->ds);
    if (t.rows) {
        HIPCHK(ctx, hipMemsetAsync(x->d_lin, 0xFF, (size_t)x->n_lin * 4, ctx->stream));
        format_pass2(ctx->stream, c->v.start, c->v.end, c->v.mapq, c->v.strand, n, p, d_pre, x->d_text, x->d_run_bin,
                     x->d_run_off, x->d_lin, x->n_lin, d_bits);
        HIPCHK(ctx, hipGetLastError());
    }
    return FTK_OK;
}

const uint8_t kBgzfEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0,
                              0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

int write_fully(int fd, const uint8_t* p, size_t n) {
    while (n) {
        const ssize_t w = write(fd, p, std::min<size_t>(n, size_t(1) << 30));
        if (w < 0) {
            if (errno == EINTR) continue;
            return -1;
        }
        p += w;
        n -= (size_t)w;
    }
    return 0;
}

double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void export_result_free(ftk_export_result* r) {
    if (!r) return;
    free(r->linear);
    free(r->run_bin);
    free(r->run_beg);
    free(r->run_end);
    r->linear = nullptr;
    r->run_bin = nullptr;
    r->run_beg = r->run_end = nullptr;
    r->n_linear = r->n_runs = 0;
}

}  // namespace

extern "C" {

int ftk_mask_lds_intervals(void) { return kMaskLdsIntervals; }

int ftk_frags_mask_keep(ftk_ctx* ctx, int contig_id, const ftk_region_mask* mask, uint8_t* keep_out, int64_t* n_kept) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (!mask) return fail(ctx, FTK_ERR_INVALID, "mask is NULL");
    if (n_kept) *n_kept = 0;
    MaskPack mk;
    int rc = mask_pack(ctx, mask, &mk);
    if (rc) return rc;
    ContigData* c;
    if ((rc = get_contig(ctx, contig_id, &c))) return rc;
    const int64_t n = c->n;
    if (n > 0 && !keep_out) return fail(ctx, FTK_ERR_INVALID, "keep_out is NULL");
    if (n == 0) return FTK_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t words = mask_words(n);
    if ((rc = reserve_scratch(ctx, align_up(mk.host.size() * sizeof(int32_t)) + align_up(words * 8 + 8)))) return rc;
    Arena a(ctx);
    int32_t* d_mask = a.take<int32_t>(mk.host.size());
    unsigned long long* d_bits = a.take<unsigned long long>(words + 1);
    std::vector<unsigned long long> bits(words);
    HIPCHK(ctx, hipMemcpyAsync(d_mask, mk.host.data(), mk.host.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    mask_keep(ctx->stream, c->v.start, c->v.end, n, mk.view(d_mask), d_bits);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(bits.data(), d_bits, words * 8, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);  // (always: the copies use this frame's host blocks)
    if (e != hipSuccess || e2 != hipSuccess)
        return fail(ctx, FTK_ERR_HIP, "mask kernel failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    int64_t kept = 0;
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t b = (uint8_t)((bits[(size_t)(i >> 6)] >> (i & 63)) & 1u);
        keep_out[i] = b;
        kept += b;
    }
    if (n_kept) *n_kept = kept;
    return FTK_OK;
}

int ftk_frags_format_rows(ftk_ctx* ctx, int contig_id, const char* name, int32_t mapq_min, int32_t min_len, int32_t max_len,
                          int layout, char** out, int64_t* out_len, int64_t* n_rows) {
    return ftk_frags_format_rows_masked(ctx, contig_id, name, mapq_min, min_len, max_len, layout, out, out_len, n_rows, nullptr);
}

int ftk_frags_format_rows_masked(ftk_ctx* ctx, int contig_id, const char* name, int32_t mapq_min, int32_t min_len,
                                 int32_t max_len, int layout, char** out, int64_t* out_len, int64_t* n_rows,
                                 const ftk_region_mask* mask) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (!out || !out_len) return fail(ctx, FTK_ERR_INVALID, "bad arguments");
    *out = nullptr;
    *out_len = 0;
    if (n_rows) *n_rows = 0;
    RowParams p;
    int rc = row_params(ctx, name, mapq_min, min_len, max_len, layout, &p);
    if (rc) return rc;
    MaskPack mk;
    if (mask && (rc = mask_pack(ctx, mask, &mk))) return rc;
    ContigData* c;
    if ((rc = get_contig(ctx, contig_id, &c))) return rc;
    ExportText x;
    if ((rc = format_contig(ctx, c, p, false, mask ? &mk : nullptr, &x))) return rc;
    char* buf = (char*)malloc((size_t)x.total.bytes + 1);
    if (!buf) return fail(ctx, FTK_ERR_OOM, "out of host memory");
    if (x.total.bytes) {
        hipError_t e = hipMemcpyAsync(buf, x.d_text, (size_t)x.total.bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            free(buf);
            return fail(ctx, FTK_ERR_HIP, "copy of the rows failed: %s", hipGetErrorString(e));
        }
    }
    buf[x.total.bytes] = 0;
    *out = buf;
    *out_len = (int64_t)x.total.bytes;
    if (n_rows) *n_rows = x.total.rows;
    return FTK_OK;
}

int ftk_bgzf_deflate_device(ftk_ctx* ctx, const uint8_t* data, int64_t n, uint8_t* out, int64_t cap, int64_t* n_out,
                            int64_t* block_offsets, int write_eof) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (n < 0 || (n > 0 && !data) || (cap > 0 && !out) || !n_out) return fail(ctx, FTK_ERR_INVALID, "bad arguments");
    if (n >= (int64_t(1) << 32) - 65536) return fail(ctx, FTK_ERR_INVALID, "at most 4 GB per call");
    const int64_t nb = bgzf_blocks(n);
    const int64_t eof = write_eof ? 28 : 0;
    *n_out = eof;
    unsigned long long total = 0;
    DeflateScratch ds{};
    if (nb > 0) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        int rc = reserve_scratch(ctx, align_up((size_t)n + 64) + deflate_scratch_bytes(n) + 4096);
        if (rc) return rc;
        Arena a(ctx);
        uint8_t* d_text = a.take<uint8_t>((size_t)n + 64);
        take_deflate_scratch(a, n, &ds);
        HIPCHK(ctx, hipMemcpyAsync(d_text, data, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        deflate_members(ctx->stream, d_text, n, ds);
        HIPCHK(ctx, hipGetLastError());
        deflate_compact(ctx->stream, nb, ds);
        HIPCHK(ctx, hipGetLastError());
        std::vector<unsigned long long> offs((size_t)nb + 1);
        HIPCHK(ctx, hipMemcpyAsync(offs.data(), ds.offs, offs.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        total = offs[(size_t)nb];
        if (block_offsets)
            for (int64_t k = 0; k <= nb; ++k) block_offsets[k] = (int64_t)offs[(size_t)k];
    } else if (block_offsets) {
        block_offsets[0] = 0;
    }
    *n_out = (int64_t)total + eof;
    if (*n_out > cap) return fail(ctx, FTK_ERR_INVALID, "output holds %lld bytes, %lld needed", (long long)cap, (long long)*n_out);
    if (total) {
        HIPCHK(ctx, hipMemcpyAsync(out, ds.out, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (eof) memcpy(out + total, kBgzfEof, 28);
    return FTK_OK;
}

int ftk_frags_write(ftk_ctx* ctx, int contig_id, const char* name, int32_t mapq_min, int32_t min_len, int32_t max_len,
                    int layout, const char* path, int append, int write_eof, int deflate_on_host, ftk_export_result* res) {
    return ftk_frags_write_masked(ctx, contig_id, name, mapq_min, min_len, max_len, layout, path, append, write_eof,
                                  deflate_on_host, res, nullptr);
}

int ftk_frags_write_masked(ftk_ctx* ctx, int contig_id, const char* name, int32_t mapq_min, int32_t min_len,
                           int32_t max_len, int layout, const char* path, int append, int write_eof, int deflate_on_host,
                           ftk_export_result* res, const ftk_region_mask* mask) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (!path || !res) return fail(ctx, FTK_ERR_INVALID, "bad arguments");
    memset(res, 0, sizeof(*res));
    RowParams p;
    int rc = row_params(ctx, name, mapq_min, min_len, max_len, layout, &p);
    if (rc) return rc;
    MaskPack mk;
    if (mask && (rc = mask_pack(ctx, mask, &mk))) return rc;
    ContigData* c;
    if ((rc = get_contig(ctx, contig_id, &c))) return rc;
    if (const char* env = getenv("FTK_EXPORT_DEFLATE"))
        if (!strcmp(env, "host")) deflate_on_host = 1;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int i = 0; i < 4; ++i)
                if (e[i]) (void)hipEventDestroy(e[i]);
        }
    } guard{ev};
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (auto& e : ev) HIPCHK(ctx, hipEventCreate(&e));
    HIPCHK(ctx, hipEventRecord(ev[0], ctx->stream));
    ExportText x;
    if ((rc = format_contig(ctx, c, p, !deflate_on_host, mask ? &mk : nullptr, &x))) return rc;
    HIPCHK(ctx, hipEventRecord(ev[1], ctx->stream));
    const size_t T = (size_t)x.total.bytes;
    const int64_t nb = x.n_blocks;
    res->n_rows = x.total.rows;
    res->text_bytes = (int64_t)T;
    // the index inputs: small, on their way while the members are built
    std::vector<int32_t> run_bin((size_t)x.n_runs);
    std::vector<uint32_t> run_off((size_t)x.n_runs), lin((size_t)x.n_lin);
    if (x.n_runs) {
        HIPCHK(ctx, hipMemcpyAsync(run_bin.data(), x.d_run_bin, run_bin.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(run_off.data(), x.d_run_off, run_off.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(lin.data(), x.d_lin, lin.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    std::vector<int64_t> boff((size_t)nb + 1, 0);  // file offsets of the members, then of what follows them
    struct stat st;
    int64_t file_pos = 0;
    if (append && stat(path, &st) == 0) file_pos = (int64_t)st.st_size;
    res->first_off = file_pos;
    if (deflate_on_host) {
        std::vector<char> text(T + 1);
        if (T) HIPCHK(ctx, hipMemcpyAsync(text.data(), x.d_text, T, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipEventRecord(ev[2], ctx->stream));
        HIPCHK(ctx, hipEventRecord(ev[3], ctx->stream));
        const double t0 = wall_ms();
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        const double t1 = wall_ms();
        if (ftk_bgzf_write(path, text.data(), (int64_t)T, 1, 0, append, write_eof, boff.data()) != FTK_OK)
            return fail(ctx, FTK_ERR_IO, "%s", ftk_fragtable_error());
        res->stage_ms[3] = t1 - t0;
        res->stage_ms[4] = wall_ms() - t1;
    } else {
        deflate_members(ctx->stream, x.d_text, (int64_t)T, x.ds);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipEventRecord(ev[2], ctx->stream));
        deflate_compact(ctx->stream, nb, x.ds);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipEventRecord(ev[3], ctx->stream));
        std::vector<unsigned long long> offs((size_t)nb + 1, 0ull);
        if (nb) HIPCHK(ctx, hipMemcpyAsync(offs.data(), x.ds.offs, offs.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        const size_t total = (size_t)offs[(size_t)nb];
        for (int64_t k = 0; k <= nb; ++k) boff[(size_t)k] = file_pos + (int64_t)offs[(size_t)k];
        const double t0 = wall_ms();
        void* host = nullptr;
        bool pinned = total > 0 && ftk_host_alloc((int64_t)total, &host) == FTK_OK;
        if (total && !pinned && !(host = malloc(total))) return fail(ctx, FTK_ERR_OOM, "out of host memory");
        auto release = [&]() {
            if (pinned) ftk_host_free(host);
            else free(host);
        };
        if (total) {
            hipError_t e = hipMemcpyAsync(host, x.ds.out, total, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) {
                release();
                return fail(ctx, FTK_ERR_HIP, "copy of the BGZF members failed: %s", hipGetErrorString(e));
            }
        }
        const double t1 = wall_ms();
        const int fd = open(path, O_WRONLY | O_CREAT | (append ? O_APPEND : O_TRUNC), 0644);
        if (fd < 0) {
            release();
            return fail(ctx, FTK_ERR_IO, "cannot open %s for writing: %s", path, strerror(errno));
        }
        int bad = total ? write_fully(fd, (const uint8_t*)host, total) : 0;
        if (!bad && write_eof) bad = write_fully(fd, kBgzfEof, sizeof(kBgzfEof));
        const int err = errno;
        release();
        if (close(fd) || bad) return fail(ctx, FTK_ERR_IO, "write to %s failed: %s", path, strerror(bad ? err : errno));
        res->stage_ms[3] = t1 - t0;
        res->stage_ms[4] = wall_ms() - t1;
    }
    for (int k = 0; k < 3; ++k) {
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
        res->stage_ms[k] = ms;
    }
    res->end_off = boff[(size_t)nb];
    // text offsets -> virtual offsets; the end of the text is the start of whatever block follows the contig
    auto voff = [&](uint64_t t) -> uint64_t {
        if (t >= T) return (uint64_t)boff[(size_t)nb] << 16;
        return ((uint64_t)boff[t / kBgzfData] << 16) | (t % kBgzfData);
    };
    if (x.n_runs) {
        res->run_bin = (int32_t*)malloc(run_bin.size() * 4);
        res->run_beg = (uint64_t*)malloc(run_bin.size() * 8);
        res->run_end = (uint64_t*)malloc(run_bin.size() * 8);
        res->linear = (uint64_t*)malloc(lin.size() * 8 + 8);
        if (!res->run_bin || !res->run_beg || !res->run_end || !res->linear) {
            export_result_free(res);
            return fail(ctx, FTK_ERR_OOM, "out of host memory");
        }
        res->n_runs = x.n_runs;
        for (size_t r = 0; r < run_bin.size(); ++r) {
            res->run_bin[r] = run_bin[r];
            res->run_beg[r] = voff(run_off[r]);
            res->run_end[r] = voff(r + 1 < run_bin.size() ? run_off[r + 1] : T);
        }
        // (htslib: a window without a first row takes the next window's offset)
        res->n_linear = (int64_t)lin.size();
        uint64_t next = 0;
        for (size_t w = lin.size(); w-- > 0;) {
            if (lin[w] != 0xFFFFFFFFu) next = voff(lin[w]);
            res->linear[w] = next;
        }
    }
    return FTK_OK;
}

}  // extern "C"
