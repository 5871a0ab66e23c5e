// Part of ftk_api.hip's translation unit (#included there, in this order: perbase, ref, comm, export) - reference images (`ftk_ref_*`), `ftk_motif_counts`, `ftk_ref_gc_counts`, `ftk_bgzf_inflate_device` (still inside the extern "C" block opened in ftk_api.hip; this part closes it).


namespace {

constexpr size_t kRefStageBytes = size_t(16) << 20;
constexpr size_t kRefPoolMax = 4;

// a device block of at least `bytes` for a reference image: the smallest pooled one that fits, else a fresh one
int ref_block_take(ftk_ctx* ctx, size_t bytes, void** out, size_t* cap) {
    int best = -1;
    for (size_t i = 0; i < ctx->ref_pool.size(); ++i)
        if (ctx->ref_pool[i].second >= bytes && (best < 0 || ctx->ref_pool[i].second < ctx->ref_pool[best].second)) best = (int)i;
    if (best >= 0) {
        *out = ctx->ref_pool[best].first;
        *cap = ctx->ref_pool[best].second;
        ctx->ref_pool.erase(ctx->ref_pool.begin() + best);
        return FTK_OK;
    }
    const size_t want = align_up(bytes + bytes / 8, 1 << 20);  // a little slack: the next contig is often slightly larger
    HIPCHK(ctx, hipMalloc(out, want));
    *cap = want;
    return FTK_OK;
}

void ref_block_give(ftk_ctx* ctx, void* d, size_t cap) {
    if (!d) return;
    ctx->ref_pool.emplace_back(d, cap);
    while (ctx->ref_pool.size() > kRefPoolMax) {  // keep the largest blocks
        size_t k = 0;
        for (size_t i = 1; i < ctx->ref_pool.size(); ++i)
            if (ctx->ref_pool[i].second < ctx->ref_pool[k].second) k = i;
        (void)hipFree(ctx->ref_pool[k].first);
        ctx->ref_pool.erase(ctx->ref_pool.begin() + (long)k);
    }
}

int ref_drop(ftk_ctx* ctx, int ref_id) {  // an image about to be replaced / released: its blocks go back to the pool
    auto it = ctx->refs.find(ref_id);
    if (it == ctx->refs.end()) return FTK_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // launches that read it have finished
    ref_block_give(ctx, it->second.d, (size_t)it->second.cap);
    if (it->second.d_nblk) (void)hipFree(it->second.d_nblk);
    ctx->refs.erase(it);
    return FTK_OK;
}

}  // namespace

int ftk_ref_upload(ftk_ctx* ctx, int ref_id, const uint8_t* image, int64_t n_bytes, int kind) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (n_bytes < 0 || (n_bytes > 0 && !image) || (kind != FTK_REF_FASTA_TEXT && kind != FTK_REF_2BIT))
        return fail(ctx, FTK_ERR_INVALID, "bad reference image arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = ref_drop(ctx, ref_id);
    if (rc) return rc;
    ftk_ctx::RefImage r;
    r.bytes = n_bytes;
    r.kind = kind;
    size_t cap = 0;
    if ((rc = ref_block_take(ctx, (size_t)n_bytes + 32, &r.d, &cap))) return rc;  // padded: 16-byte loads never leave the block
    r.cap = (int64_t)cap;
    // on the ctx stream, one wait for THAT stream at the end (a synchronous hipMemcpy waits for every transfer the
    // device has in flight)
    hipError_t e = hipMemsetAsync((char*)r.d + n_bytes, 0, 32, ctx->stream);
    if (e == hipSuccess && n_bytes)
        e = hipMemcpyAsync(r.d, image, n_bytes, is_device_ptr(image) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(r.d);
        return fail(ctx, FTK_ERR_HIP, "reference upload failed: %s", hipGetErrorString(e));
    }
    ctx->refs[ref_id] = r;
    return FTK_OK;
}

int ftk_ref_upload_file(ftk_ctx* ctx, int ref_id, const char* path, int64_t file_offset, int64_t n_bytes, int kind) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (!path || file_offset < 0 || n_bytes < 0 || (kind != FTK_REF_FASTA_TEXT && kind != FTK_REF_2BIT))
        return fail(ctx, FTK_ERR_INVALID, "bad reference image arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(ctx, FTK_ERR_IO, "cannot open %s: %s", path, strerror(errno));
    struct Closer { int fd; ~Closer() { close(fd); } } closer{fd};
    int rc = ref_drop(ctx, ref_id);
    if (rc) return rc;
    for (int k = 0; k < 2; ++k) {
        if (!ctx->ref_stage[k]) HIPCHK(ctx, hipHostMalloc(&ctx->ref_stage[k], kRefStageBytes, hipHostMallocDefault));
        if (!ctx->ref_stage_done[k]) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ref_stage_done[k], hipEventDisableTiming));
    }
    ftk_ctx::RefImage r;
    r.bytes = n_bytes;
    r.kind = kind;
    size_t cap = 0;
    if ((rc = ref_block_take(ctx, (size_t)n_bytes + 32, &r.d, &cap))) return rc;
    r.cap = (int64_t)cap;
    // (a chunk is only rewritten once the copy that last read it has finished - the event of a PREVIOUS call's last
    // chunks included: the call returns with its final copies still in flight; an event never recorded is complete)
    hipError_t e = hipMemsetAsync((char*)r.d + n_bytes, 0, 32, ctx->stream);
    int k = 0;
    // the file (page cache) -> a page-locked chunk on four pread threads -> the device, the next chunk read while the
    // previous one is on its way
    for (int64_t off = 0; off < n_bytes && e == hipSuccess; off += (int64_t)kRefStageBytes, k ^= 1) {
        const size_t n = (size_t)std::min<int64_t>((int64_t)kRefStageBytes, n_bytes - off);
        e = hipEventSynchronize(ctx->ref_stage_done[k]);
        if (e != hipSuccess) break;
        std::atomic<int> bad{0};
        const int nt = n >= (size_t(4) << 20) ? 4 : 1;
        char* dst = (char*)ctx->ref_stage[k];
        ftk_host::parallel_run(nt, [&](int t) {
            size_t a = n * (size_t)t / nt;
            const size_t b = n * (size_t)(t + 1) / nt;
            while (a < b) {
                const ssize_t got = pread(fd, dst + a, b - a, (off_t)(file_offset + off + (int64_t)a));
                if (got <= 0) { bad.store(1); return; }
                a += (size_t)got;
            }
        });
        if (bad.load()) {
            (void)hipStreamSynchronize(ctx->stream);
            ref_block_give(ctx, r.d, cap);
            return fail(ctx, FTK_ERR_IO, "%s is shorter than the reference image it should hold", path);
        }
        e = hipMemcpyAsync((char*)r.d + off, dst, n, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(ctx->ref_stage_done[k], ctx->stream);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(ctx->stream);
        ref_block_give(ctx, r.d, cap);
        return fail(ctx, FTK_ERR_HIP, "reference upload failed: %s", hipGetErrorString(e));
    }
    ctx->refs[ref_id] = r;  // (kernels of this stream run behind the copies; the staging chunks wait on their events)
    return FTK_OK;
}

int ftk_ref_release(ftk_ctx* ctx, int ref_id) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (ctx->refs.find(ref_id) == ctx->refs.end()) return fail(ctx, FTK_ERR_NO_CONTIG, "reference image %d is not loaded", ref_id);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return ref_drop(ctx, ref_id);
}

int ftk_ref_set_layout(ftk_ctx* ctx, int ref_id, int64_t chrom_len, int32_t line_bases, int32_t line_width,
                       const int32_t* nblock_start, const int32_t* nblock_end, int64_t n_nblocks) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    auto it = ctx->refs.find(ref_id);
    if (it == ctx->refs.end()) return fail(ctx, FTK_ERR_NO_CONTIG, "reference image %d is not loaded", ref_id);
    ftk_ctx::RefImage& r = it->second;
    if (chrom_len < 0 || chrom_len > INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "chrom_len out of range");
    if (n_nblocks < 0 || n_nblocks > (1 << 28) || (n_nblocks > 0 && (!nblock_start || !nblock_end)))
        return fail(ctx, FTK_ERR_INVALID, "bad N-block arguments");
    if (r.kind == FTK_REF_FASTA_TEXT) {
        if (chrom_len > 0 && (line_bases <= 0 || line_width < line_bases))
            return fail(ctx, FTK_ERR_INVALID, "FASTA images need line_bases > 0 and line_width >= line_bases");
        if (chrom_len > 0 && (chrom_len / line_bases) * line_width + chrom_len % line_bases > r.bytes)
            return fail(ctx, FTK_ERR_INVALID, "chrom_len does not fit the uploaded FASTA text");
    } else if ((chrom_len + 3) / 4 > r.bytes) {
        return fail(ctx, FTK_ERR_INVALID, "chrom_len does not fit the uploaded 2bit image");
    }
    for (int64_t i = 0; i < n_nblocks; ++i)
        if (nblock_start[i] < 0 || nblock_end[i] < nblock_start[i] || (i && nblock_start[i] < nblock_end[i - 1]))
            return fail(ctx, FTK_ERR_INVALID, "N blocks must be sorted and disjoint");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (r.d_nblk) (void)hipFree(r.d_nblk);
    r.d_nblk = nullptr;
    r.n_nblk = 0;
    if (n_nblocks) {
        HIPCHK(ctx, hipMalloc((void**)&r.d_nblk, (size_t)n_nblocks * 8));
        HIPCHK(ctx, hipMemcpy(r.d_nblk, nblock_start, (size_t)n_nblocks * 4, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(r.d_nblk + n_nblocks, nblock_end, (size_t)n_nblocks * 4, hipMemcpyHostToDevice));
        r.n_nblk = (int32_t)n_nblocks;
    }
    r.chrom_len = chrom_len;
    r.line_bases = line_bases;
    r.line_width = line_width;
    return FTK_OK;
}

int ftk_motif_counts(ftk_ctx* ctx, int contig_id, int ref_id, const int32_t* w_start, const int32_t* w_end,
                     int64_t n_win, const ftk_motif* motif, int32_t mapq_min, int32_t fetch_mode,
                     uint32_t* counts_out, int64_t* nfrag_out, int64_t* err_out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    MotifParams mp{};
    const int rc = open_ref_view(ctx, ref_id, &mp);
    if (rc) return rc;
    if (!motif) return fail(ctx, FTK_ERR_INVALID, "motif is NULL");
    if (motif->k < 1 || motif->k > 7) return fail(ctx, FTK_ERR_INVALID, "k must be in [1, 7]");
    if (n_win > 0 && (!counts_out || !err_out)) return fail(ctx, FTK_ERR_INVALID, "NULL output pointer");
    mp.k = motif->k;
    mp.f_off = motif->fwd_offset;
    mp.r_off = motif->rev_offset;
    mp.both = motif->both_strands != 0;
    mp.neg = motif->negative_strand != 0;
    mp.guard = motif->guard;
    mp.rev_err = motif->rev_oob_is_error != 0;
    ftk_filter f{mapq_min, FTK_LEN_OPEN, FTK_LEN_OPEN, FTK_POLICY_ANY, fetch_mode};
    FeatCall fc;
    fc.f = &f;
    fc.count_out = nfrag_out;
    fc.hist_out = counts_out;
    fc.overflow_out = err_out;
    fc.len_lo = 0;
    fc.n_bins = 1 << (2 * motif->k);
    fc.motif = &mp;
    return features_common(ctx, contig_id, w_start, w_end, n_win, fc);
}

int ftk_ref_gc_counts(ftk_ctx* ctx, int ref_id, const int64_t* range_lo, const int64_t* range_hi, int64_t n,
                      int64_t* gc_out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    auto it = ctx->refs.find(ref_id);
    if (it == ctx->refs.end()) return fail(ctx, FTK_ERR_NO_CONTIG, "reference image %d is not loaded", ref_id);
    if (n < 0 || n > INT32_MAX) return fail(ctx, FTK_ERR_INVALID, "n out of range");
    if (n == 0) return FTK_OK;
    if (!range_lo || !range_hi || !gc_out) return fail(ctx, FTK_ERR_INVALID, "NULL argument");
    const ftk_ctx::RefImage& r = it->second;
    const int64_t limit = r.kind == FTK_REF_2BIT ? r.bytes * 4 : r.bytes;
    if (!is_device_ptr(range_lo))
        for (int64_t i = 0; i < n; ++i)
            if (range_lo[i] < 0 || range_hi[i] > limit)
                return fail(ctx, FTK_ERR_INVALID, "range %lld outside the reference image", (long long)i);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int64_t *b_lo = nullptr, *b_hi = nullptr, *d_out = nullptr;
    Scratch s(ctx);
    s.tmp(&b_lo, n);
    s.tmp(&b_hi, n);
    s.out(&d_out, gc_out, n);
    int rc = s.reserve();
    if (rc) return rc;
    const int64_t *d_lo, *d_hi;
    if ((rc = stage_in(ctx, range_lo, n, b_lo, &d_lo))) return rc;
    if ((rc = stage_in(ctx, range_hi, n, b_hi, &d_hi))) return rc;
    launch_gc_count(ctx->stream, (const uint8_t*)r.d, r.bytes, r.kind, d_lo, d_hi, (int)n, d_out);
    HIPCHK(ctx, hipGetLastError());
    return s.finish();
}

// ---- DEFLATE on the device (csrc/ftk_inflate.hip) -------------------------------------------------------
int ftk_bgzf_inflate_device(ftk_ctx* ctx, const uint8_t* file_bytes, int64_t n, uint8_t* out, int64_t cap, int64_t* n_out) {
    if (!ctx) return fail(nullptr, FTK_ERR_INVALID, "ctx is NULL");
    if (!file_bytes || n < 0 || (cap > 0 && !out) || !n_out) return fail(ctx, FTK_ERR_INVALID, "bad arguments");
    if (n >= (int64_t(1) << 32) - 65536) return fail(ctx, FTK_ERR_INVALID, "at most 4 GB per call");
    // walk the BGZF blocks: 12-byte gzip header with FEXTRA, the BC subfield gives the block size
    std::vector<ftk::InflateBlock> tab;
    std::vector<uint32_t> want_crc;
    uint64_t off = 0, total = 0;
    while (off < (uint64_t)n) {
        const uint8_t* p = file_bytes + off;
        if (off + 18 > (uint64_t)n || p[0] != 31 || p[1] != 139 || p[2] != 8 || !(p[3] & 4))
            return fail(ctx, FTK_ERR_FORMAT, "not a BGZF block at byte %llu", (unsigned long long)off);
        const unsigned xlen = p[10] | (p[11] << 8);
        unsigned bsize = 0;
        for (unsigned x = 0; x + 4 <= xlen && off + 12 + x + 4 <= (uint64_t)n;) {
            const uint8_t* f = p + 12 + x;
            const unsigned slen = f[2] | (f[3] << 8);
            if (f[0] == 66 && f[1] == 67 && slen == 2 && off + 12 + x + 6 <= (uint64_t)n) bsize = (f[4] | (f[5] << 8)) + 1u;
            x += 4 + slen;
        }
        const uint64_t q = off + 12 + xlen;
        if (!bsize || off + bsize > (uint64_t)n || q + 8 > off + bsize)
            return fail(ctx, FTK_ERR_FORMAT, "corrupt BGZF block at byte %llu", (unsigned long long)off);
        const uint8_t* tr = p + bsize - 8;
        const uint32_t isize = (uint32_t)tr[4] | ((uint32_t)tr[5] << 8) | ((uint32_t)tr[6] << 16) | ((uint32_t)tr[7] << 24);
        if (isize > 65536u || total + isize >= (uint64_t(1) << 32)) return fail(ctx, FTK_ERR_FORMAT, "BGZF block too large");
        tab.push_back({(uint32_t)q, (uint32_t)(off + bsize - 8 - q), (uint32_t)total, isize});
        want_crc.push_back((uint32_t)tr[0] | ((uint32_t)tr[1] << 8) | ((uint32_t)tr[2] << 16) | ((uint32_t)tr[3] << 24));
        total += isize;
        off += bsize;
    }
    *n_out = (int64_t)total;
    if ((int64_t)total > cap) return fail(ctx, FTK_ERR_INVALID, "output holds %lld bytes, %lld needed", (long long)cap, (long long)total);
    if (tab.empty() || total == 0) return FTK_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    uint8_t *d_comp = nullptr, *d_out = nullptr;
    ftk::InflateBlock* d_tab = nullptr;
    ftk::InflateStatus* d_st = nullptr;
    uint32_t* d_crc = nullptr;
    Scratch s(ctx);  // (`out` is a host array that takes its bytes only after the checks below: temporaries throughout)
    s.tmp(&d_comp, (size_t)n + 8);
    s.tmp(&d_tab, tab.size());
    s.tmp(&d_st, 1);
    s.tmp(&d_crc, tab.size());
    s.tmp(&d_out, (size_t)total + 8192 + 4096);  // (rounded up to a 4 KB bound below: at least 8 KB stay behind `total`)
    int rc = s.reserve();
    if (rc) return rc;
    d_out = (uint8_t*)(((uintptr_t)d_out + 4095) & ~(uintptr_t)4095);
    // The kernel addresses its input by 32-BIT BIT POSITIONS from the pointer it is given: a launch takes blocks whose
    // compressed bytes lie within 2^28 bytes of its first one (the streams' pieces are 48-96 MB; an image of more than
    // that goes in several launches, each from a base of its own - block offsets are rebased here, before the table goes up).
    struct Run {
        size_t first, count, base;
    };
    std::vector<Run> runs;
    for (size_t i = 0; i < tab.size();) {
        const size_t base = (size_t)tab[i].in_off & ~(size_t)3;
        size_t j = i;
        while (j < tab.size() && (size_t)tab[j].in_off + tab[j].in_len - base < (size_t(1) << 28)) ++j;
        if (j == i) return fail(ctx, FTK_ERR_FORMAT, "BGZF block too large");  // (cannot happen: a block is at most 64 KB)
        runs.push_back({i, j - i, base});
        for (size_t k = i; k < j; ++k) tab[k].in_off -= (uint32_t)base;
        i = j;
    }
    HIPCHK(ctx, hipMemcpyAsync(d_comp, file_bytes, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(tab[0]), hipMemcpyHostToDevice, ctx->stream));
    // (FTK_INFLATE_VECTOR_MATCHES=1: the launch shape BAM streams use - a window's matches resolved on the lanes side
    // by side; read per call so that the tests can hold both shapes against zlib)
    const char* vm = getenv("FTK_INFLATE_VECTOR_MATCHES");
    ftk::InflateStatus st{};
    for (size_t r = 0; r < runs.size(); ++r) {
        HIPCHK(ctx, hipMemsetAsync(d_st, 0, sizeof(*d_st), ctx->stream));
        ftk::inflate_launch(ctx->stream, d_comp + runs[r].base, d_tab + runs[r].first, (int)runs[r].count, d_out, d_st,
                            d_crc + runs[r].first, vm && atoi(vm) != 0);
        HIPCHK(ctx, hipGetLastError());
        if (r + 1 < runs.size()) {  // (the status words are the launch's own: read before the next one clears them)
            ftk::InflateStatus sr{};
            HIPCHK(ctx, hipMemcpyAsync(&sr, d_st, sizeof(sr), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            if (sr.n_bad)
                return fail(ctx, FTK_ERR_FORMAT, "device inflate: %u of %zu BGZF blocks did not decode (block %zu: reason %u)", sr.n_bad,
                            tab.size(), runs[r].first + sr.first_bad, sr.reason);
        }
    }
    const size_t last_first = runs.back().first;
    std::vector<uint32_t> got_crc(tab.size());
    HIPCHK(ctx, hipMemcpyAsync(&st, d_st, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(got_crc.data(), d_crc, tab.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(out, d_out, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (st.n_bad)
        return fail(ctx, FTK_ERR_FORMAT, "device inflate: %u of %zu BGZF blocks did not decode (block %zu: reason %u)", st.n_bad,
                    tab.size(), last_first + st.first_bad, st.reason);
    for (size_t k = 0; k < tab.size(); ++k)  // the gzip trailer's CRC-32 against the one computed on the device
        if (got_crc[k] != want_crc[k])
            return fail(ctx, FTK_ERR_FORMAT, "device inflate: CRC mismatch in BGZF block %zu (%08x, trailer says %08x)", k,
                        got_crc[k], want_crc[k]);
    return FTK_OK;
}

}  // extern "C"
