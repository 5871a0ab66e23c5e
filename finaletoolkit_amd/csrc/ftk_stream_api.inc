// Part of ftk_decode.cpp's translation unit (#included there, in this order: core, sets, text, bam, api) - the C entry points of the streams and the caches (`ftk_fragstream_*`, `ftk_cache_trim`, `ftk_fragfile_index_contigs`).

extern "C" {

// Give back what the library keeps for reuse between calls: idle page-locked blocks (decoded tables, result arrays),
// idle device blocks of parsed contigs, the streams' idle buffer sets.  Nothing in use is touched.
int64_t ftk_cache_trim(void) {
    size_t n = table_cache().trim() + result_cache().trim() + plain_result_cache().trim();
    if (have_hip_device()) {
        n += device_cache().trim() + devset_pool().trim();
        (void)stream_pool().trim();
        n += ftk::inflate_release_scratch();
    }
    return (int64_t)n;
}

int ftk_fragfile_index_contigs(const char* path, char* names_out, int64_t cap, int64_t* needed_out, int* is_bed6_out) {
    if (!path || !needed_out) return dfail(FTK_ERR_INVALID, "NULL argument");
    *needed_out = 0;
    Bytes raw, img;
    const std::string ipath = std::string(path) + ".tbi";
    if (!read_file(ipath.c_str(), &raw) || raw.size() < 8) return dfail(FTK_ERR_FORMAT, "no usable tabix index at %s", ipath.c_str());
    if (inflate_all(raw, 1, &img) != FTK_OK || img.size() < 36 || memcmp(img.data(), "TBI\1", 4) != 0)
        return dfail(FTK_ERR_FORMAT, "%s is not a tabix index", ipath.c_str());
    const uint8_t* p = img.data();
    const int32_t n_ref = rd_i32(p + 4), l_nm = rd_i32(p + 32);
    if (n_ref < 0 || l_nm < 0 || 36 + (size_t)l_nm > img.size()) return dfail(FTK_ERR_FORMAT, "corrupt tabix index");
    // names of the references that hold at least one chunk, newline-separated
    std::string joined;
    size_t a = 36;
    for (int k = 0; k < n_ref && a < 36 + (size_t)l_nm; ++k) {
        const char* nm = (const char*)p + a;
        const size_t len = strnlen(nm, 36 + (size_t)l_nm - a);
        const IndexSpan sp = index_lookup(ipath, false, std::string(nm, len), -1);
        if (!sp.usable) return dfail(FTK_ERR_FORMAT, "corrupt tabix index");
        if (sp.present) { joined.append(nm, len); joined.push_back('\n'); }
        a += len + 1;
    }
    *needed_out = (int64_t)joined.size() + 1;
    if (names_out && cap >= (int64_t)joined.size() + 1) memcpy(names_out, joined.c_str(), joined.size() + 1);
    if (is_bed6_out) {  // layout of the first data row (io/alignment.py:143-156), from the file's first block
        *is_bed6_out = 0;
        FILE* fp = fopen(path, "rb");
        if (!fp) return dfail(FTK_ERR_IO, "cannot read %s", path);
        Bytes head, text;
        head.alloc(1 << 17);
        const size_t got = fread(head.data(), 1, head.size(), fp);
        fclose(fp);
        size_t bs = 0;
        const size_t q = gzip_header(head.data(), got, 0, &bs);
        if (q && bs && bs <= got) {
            Bytes one;
            one.alloc(bs);
            memcpy(one.data(), head.data(), bs);
            if (inflate_all(one, 1, &text) == FTK_OK) {
                const char* b = (const char*)text.data();
                bool six = false;
                if (sniff_bed6(b, b + text.size(), true, &six)) *is_bed6_out = six;
            }
        }
    }
    return FTK_OK;
}

static int fragstream_open_impl(const char* path, const char* contig, int is_bam, int n_threads, int max_queued,
                                int device, ftk_fragstream** out, long long reg_start = -1, long long reg_stop = -1) {
    if (!path || !out) return dfail(FTK_ERR_INVALID, "NULL argument");
    *out = nullptr;
    FILE* fp = fopen(path, "rb");
    if (!fp) return dfail(FTK_ERR_IO, "cannot read %s", path);
    ftk_fragstream* s = new ftk_fragstream();
    s->path = path;
    if (contig) { s->only = contig; s->has_only = true; }
    if (contig && reg_start >= 0 && reg_stop > reg_start) {
        s->has_region = true;
        s->reg_start = reg_start;
        s->reg_stop = reg_stop;
    }
    s->bam = is_bam != 0;
    s->n_threads = std::max(1, n_threads);
    s->max_queued = (size_t)std::max(1, max_queued);
    s->fp = fp;
    // BAM records are parsed by the host; FTK_DEVICE_PARSE=0 keeps text rows there too
    static const bool device_parse = !(getenv("FTK_DEVICE_PARSE") && atoi(getenv("FTK_DEVICE_PARSE")) == 0);
    s->device = (!s->bam && device_parse) ? device : -1;
    s->inflate_device = s->bam ? device : -1;  // BAM: records stay on the host, the BGZF inflate may use the GPU
    s->producer = std::thread([s] { s->run(); });
    *out = s;
    return FTK_OK;
}

int ftk_fragstream_open(const char* path, const char* contig, int is_bam, int n_threads, int max_queued,
                        ftk_fragstream** out) {
    return fragstream_open_impl(path, contig, is_bam, n_threads, max_queued, -1, out);
}

int ftk_fragstream_open_device(int device_id, const char* path, const char* contig, int is_bam, int n_threads,
                               int max_queued, ftk_fragstream** out) {
    if (device_id < 0 || !have_hip_device()) return dfail(FTK_ERR_NO_DEVICE, "ftk_fragstream_open_device: no HIP device");
    return fragstream_open_impl(path, contig, is_bam, n_threads, max_queued, device_id, out);
}

int ftk_fragstream_open_region(int device_id, const char* path, const char* contig, int64_t start, int64_t stop, int is_bam,
                               int n_threads, int max_queued, ftk_fragstream** out) {
    if (!contig || start < 0 || stop <= start) return dfail(FTK_ERR_INVALID, "a region needs a contig and 0 <= start < stop");
    return fragstream_open_impl(path, contig, is_bam, n_threads, max_queued, device_id, out, (long long)start, (long long)stop);
}

int ftk_fragstream_next(ftk_fragstream* s, ftk_fragtable** out) {
    if (!s || !out) return dfail(FTK_ERR_INVALID, "NULL argument");
    *out = nullptr;
    std::unique_lock<std::mutex> lk(s->mu);
    s->consumer_waiting = true;
    s->cv.wait(lk, [&] { return !s->ready.empty() || s->finished; });
    s->consumer_waiting = false;
    if (!s->ready.empty()) {
        *out = s->ready.front();
        s->ready.pop_front();
        s->cv.notify_all();
        return FTK_OK;
    }
    if (s->err != FTK_OK) return dfail(s->err, "%s", s->errmsg.c_str());
    return FTK_OK;  // end of file: *out stays NULL
}

int ftk_fragstream_n_refs(ftk_fragstream* s) {
    if (!s) return 0;
    std::unique_lock<std::mutex> lk(s->mu);
    s->cv.wait(lk, [&] { return s->header_ready || s->finished; });
    return (int)s->ref_names.size();
}
const char* ftk_fragstream_ref_name(ftk_fragstream* s, int i) {
    if (!s || i < 0 || i >= ftk_fragstream_n_refs(s)) return nullptr;
    return s->ref_names[i].c_str();
}
int64_t ftk_fragstream_ref_length(ftk_fragstream* s, int i) {
    if (!s || i < 0 || i >= ftk_fragstream_n_refs(s)) return -1;
    return s->ref_lens[i];
}

int ftk_fragstream_skipped(ftk_fragstream* s, int64_t out[2]) {
    if (!s || !out) return FTK_ERR_INVALID;
    out[0] = s->skipped[0].load();
    out[1] = s->skipped[1].load();
    return FTK_OK;
}

int ftk_fragtable_skipped(const ftk_fragtable* t, int64_t out[2]) {
    if (!t || !out) return FTK_ERR_INVALID;
    out[0] = t->skipped[0];
    out[1] = t->skipped[1];
    return FTK_OK;
}

int ftk_fragstream_stage_ms(ftk_fragstream* s, double out[6]) {
    if (!s || !out) return FTK_ERR_INVALID;
    std::lock_guard<std::mutex> lk(s->mu);
    for (int k = 0; k < 6; ++k) out[k] = s->stage_ms[k];
    return FTK_OK;
}

void ftk_fragstream_close(ftk_fragstream* s) {
    if (!s) return;
    {
        std::lock_guard<std::mutex> lk(s->mu);
        s->stop = true;
        s->cv.notify_all();
    }
    if (s->producer.joinable()) s->producer.join();
    s->drain_ahead();
    for (auto* t : s->ready) delete t;
    if (s->pstream) {
        (void)hipSetDevice(s->device >= 0 ? s->device : s->inflate_device);
        (void)hipStreamSynchronize(s->pstream);
        stream_pool().give(s->device >= 0 ? s->device : s->inflate_device, s->pstream);
    }
    if (s->fp) fclose(s->fp);
    delete s;
}

}  // extern "C"
