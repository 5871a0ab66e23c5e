// Part of ftk_decode.cpp's translation unit (#included there, in this order: core, sets, text, bam, api) - the streaming decoder: pieces of whole BGZF blocks, the tabix / BAI index reader, `struct ftk_fragstream` (reader, read-ahead, slot ring bookkeeping, hand-over of finished contigs), the producer thread.

// ---------------------------------------------------------------------------------------
// Streaming decoder: one contig at a time, decoded ahead of the consumer
// ---------------------------------------------------------------------------------------
// A producer thread reads the file in pieces of whole BGZF blocks, inflates and parses each
// piece on the worker threads and hands every finished contig (coordinate-sorted files keep a
// contig's rows together) to a bounded queue as a one-contig ftk_fragtable in page-locked
// memory.  The consumer uploads / computes on contig k while contig k+1 is being decoded, and
// host memory stays bounded by the piece size plus `max_queued` contigs however large the file.
namespace {

// compressed bytes read per piece (FTK_STREAM_PIECE overrides it: the tests use small pieces to
// exercise blocks, lines and records that straddle a piece boundary)
const size_t kStreamPiece = [] {
    const char* e = getenv("FTK_STREAM_PIECE");
    const long long v = e ? atoll(e) : 0;
    // (at most 120 MB: a large BAM doubles it, and the device inflate addresses a piece by 32-bit bit positions - 2^28 bytes a launch)
    return v >= (1 << 16) ? (size_t)std::min<long long>(v, 120ll << 20) : (size_t)(48u << 20);
}();

// bytes of inflated BAM per speculative stretch of the record chain (FTK_BAM_STRETCH: the tests make the
// stretches tiny so that small files exercise the guess / check / redo logic)
const size_t kBamStretch = [] {
    const char* e = getenv("FTK_BAM_STRETCH");
    const long long v = e ? atoll(e) : 0;
    return v >= 64 ? (size_t)v : (size_t)(1u << 20);
}();

struct BamRun {
    int ref = -1;
    Columns c;
};

// Growable byte buffer without zero-fill (a std::vector would memset every piece it grows by).
// `pinned`: page-locked memory from the library's recycled blocks instead - the pieces of a BAM stream whose records
// are parsed on the device go up straight from the buffer they were read into.
struct RawBuf {
    uint8_t* p = nullptr;
    size_t cap = 0;
    size_t head = 0;  // data() starts here (the read-ahead piece leaves room in front for carried bytes)
    bool pinned = false;
    RawBuf() = default;
    RawBuf(const RawBuf&) = delete;
    RawBuf& operator=(const RawBuf&) = delete;
    ~RawBuf() {
        if (!p) return;
        if (pinned) pinned_free(p); else huge_unmap(p, cap);
    }
    bool reserve(size_t n) {
        if (n <= cap) return true;
        if (pinned) {
            const size_t want = std::max(n, cap + cap / 2);
            uint8_t* q = (uint8_t*)pinned_alloc(want);
            if (!q) return false;
            if (p) {
                memcpy(q, p, cap);
                pinned_free(p);
            }
            p = q;
            cap = want;
            return true;
        }
        const size_t want = huge_round(std::max(n, cap + cap / 2));
        uint8_t* q = p ? huge_remap(p, cap, want) : huge_map(want);
        if (!q) return false;
        p = q;
        touch_pages(p, cap, want);
        cap = want;
        return true;
    }
    uint8_t* data() { return p + head; }
    void swap(RawBuf& o) {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        std::swap(head, o.head);
        std::swap(pinned, o.pinned);
    }
};

// Pack a contig held as a list of runs: one block (page-locked when a device is present), the runs
// copied to their final places by `n_threads` threads.
void pack_parts(Contig& ct, int n_threads) {
    size_t m = 0;
    std::vector<size_t> at;
    for (auto& c : ct.parts) { at.push_back(m); m += c.start.size(); }
    const size_t total = packed_bytes(m, false);
    Packed& p = ct.p;
    if (have_hip_device() && (p.base = pinned_alloc(total)) != nullptr) {
        p.pinned = true;
    } else {
        p.base = malloc(total);
        p.pinned = false;
    }
    if (!p.base) return;
    place(p, (char*)p.base, m, false);
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (;;) {
            const size_t k = next.fetch_add(1);
            if (k >= ct.parts.size()) break;
            const Columns& c = ct.parts[k];
            const size_t n = c.start.size(), o = at[k];
            if (!n) continue;
            memcpy(p.start + o, c.start.data(), n * 4);
            memcpy(p.end + o, c.end.data(), n * 4);
            memcpy(p.mapq + o, c.mapq.data(), n);
            memcpy(p.strand + o, c.strand.data(), n);
        }
    };
    const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_threads, ct.parts.size()));
    parallel_run(nt, [&](int) { work(); });
    std::vector<Columns>().swap(ct.parts);
}

// A BAM contig held as runs in read1-position order -> its page-locked block in fragment-start order:
// keys (start << 32 | file rank) built, sorted and merged in parallel, then every column gathered from
// the runs straight into its final place - no concatenated or sorted intermediate copy of the contig.
void pack_bam_parts(Contig& ct, int n_threads) {
    Stopwatch sw;
    std::vector<size_t> at;
    size_t m = 0;
    for (auto& c : ct.parts) { at.push_back(m); m += c.start.size(); }
    at.push_back(m);
    const size_t total = packed_bytes(m, true);
    Packed& p = ct.p;
    if (have_hip_device() && (p.base = pinned_alloc(total)) != nullptr) {
        p.pinned = true;
    } else {
        p.base = malloc(total);
        p.pinned = false;
    }
    if (!p.base) return;
    place(p, (char*)p.base, m, true);
    sw.lap("  packer: block");
    const size_t np = ct.parts.size();
    if (m) {
        std::unique_ptr<uint64_t[]> key(new uint64_t[m]);  // (not zeroed: the threads below write every key)
        std::atomic<int> unsorted{0};
        {
            std::atomic<size_t> next{0};
            parallel_run((int)std::max<size_t>(1, std::min<size_t>((size_t)n_threads, np)), [&](int) {
                bool bad = false;
                for (;;) {
                    const size_t k = next.fetch_add(1);
                    if (k >= np) break;
                    const std::vector<int32_t>& st = ct.parts[k].start;
                    for (size_t i = 0; i < st.size(); ++i) {
                        key[at[k] + i] = ((uint64_t)(uint32_t)st[i] << 32) | (uint64_t)(at[k] + i);
                        bad |= i > 0 && st[i] < st[i - 1];
                    }
                    // (across parts: the first start of this one against the last of the one before)
                    if (k > 0 && !st.empty() && !ct.parts[k - 1].start.empty()) bad |= st.front() < ct.parts[k - 1].start.back();
                }
                if (bad) unsorted.store(1);
            });
        }
        int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(n_threads, 1), m / 65536));
        sw.lap("  packer: keys");
        if (unsorted.load()) nt = sort_keys(key.get(), m, n_threads);
        sw.lap("  packer: sort");
        parallel_run(nt, [&](int t) {
            size_t k = 0;
            for (size_t i = m * (size_t)t / (size_t)nt, e = m * (size_t)(t + 1) / (size_t)nt; i < e; ++i) {
                const size_t j = (size_t)(uint32_t)key[i];
                while (j < at[k]) --k;            // nearly sorted: the run changes rarely
                while (j >= at[k + 1]) ++k;
                const Columns& c = ct.parts[k];
                const size_t o = j - at[k];
                p.start[i] = c.start[o];
                p.end[i] = c.end[o];
                p.mapq[i] = c.mapq[o];
                p.strand[i] = c.strand[o];
                p.r1s[i] = c.r1s[o];
                p.r1e[i] = c.r1e[o];
                p.ord[i] = (int32_t)j;
            }
        });
    }
    sw.lap("  packer: gather");
    std::vector<Columns>().swap(ct.parts);
    sw.lap("  packer: free parts");
}

// Complete text lines [b, e) -> runs in file order (segments parsed in parallel).
void parse_text_parallel(const char* b, const char* e, bool bed6, const char* only, int n_threads,
                         std::vector<Run>* out) {
    const size_t n = (size_t)(e - b);
    int nseg = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_threads, n / (1 << 16) + 1));
    std::vector<const char*> cut(nseg + 1);
    cut[0] = b;
    cut[nseg] = e;
    for (int i = 1; i < nseg; ++i) {
        const char* q = b + n * (size_t)i / (size_t)nseg;
        if (q < cut[i - 1]) q = cut[i - 1];
        const char* nl = (const char*)memchr(q, '\n', (size_t)(e - q));
        cut[i] = nl ? nl + 1 : e;
    }
    std::vector<std::vector<Run>> seg(nseg);
    parallel_run(nseg, [&](int i) { parse_segment(cut[i], cut[i + 1], bed6, only, &seg[i]); });
    for (auto& v : seg)
        for (auto& r : v) out->push_back(std::move(r));
}

// Does p[o..) look like the start of a BAM alignment record?  Only used to GUESS where a thread may
// enter the record chain in the middle of a piece (run_bam); a wrong guess is detected and redone.
inline bool plausible_record(const uint8_t* p, size_t o, size_t m, int n_ref) {
    if (o + 36 > m) return false;
    const uint32_t bs = rd_u32(p + o);
    if (bs < 32 || bs > (1u << 24)) return false;
    const uint8_t* r = p + o + 4;
    const int32_t ref = rd_i32(r), pos = rd_i32(r + 4), next_ref = rd_i32(r + 20), next_pos = rd_i32(r + 24);
    if (ref < -1 || ref >= n_ref || next_ref < -1 || next_ref >= n_ref || pos < -1 || next_pos < -1) return false;
    const uint32_t l_name = r[8], n_cigar = rd_u16(r + 12);
    const int32_t l_seq = rd_i32(r + 16);
    if (l_name < 2 || l_seq < 0) return false;  // (a missing name is "*": never empty)
    if (rd_u16(r + 14) & 0xf000) return false;   // undefined flag bits
    const uint64_t need = 32 + (uint64_t)l_name + 4ull * n_cigar + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq;
    if (need > bs) return false;
    if (o + 36 + l_name <= m) {  // the read name: printable characters, NUL-terminated
        if (r[32 + l_name - 1] != 0) return false;
        for (uint32_t k = 0; k + 1 < l_name; ++k)
            if (r[32 + k] < 33 || r[32 + k] > 126) return false;
    }
    return true;
}

inline size_t guess_record_start(const uint8_t* p, size_t from, size_t m, int n_ref) {
    // A candidate whose very first link leaves the piece proves nothing - and two bytes in front of a real record
    // of reference 0 there is one: the low half of the real block_size lands in the high half of a 32-bit size of
    // megabytes, the zeros behind it read as reference 0 (11 % of the stretches of a 60x file were redone for
    // that).  Such a candidate is kept only as a fallback for when nothing checkable follows.
    size_t fallback = SIZE_MAX;
    for (size_t o = from; o + 36 <= m; ++o) {
        if (!plausible_record(p, o, m, n_ref)) continue;
        size_t o2 = o + 4 + (size_t)rd_u32(p + o);
        bool ok = true;
        int checked = 0;
        for (int k = 0; k < 2; ++k) {  // two more links must hold, unless the piece ends first
            if (o2 + 36 > m) break;
            if (!plausible_record(p, o2, m, n_ref)) { ok = false; break; }
            ++checked;
            o2 += 4 + (size_t)rd_u32(p + o2);
        }
        if (!ok) continue;
        if (checked) return o;
        if (fallback == SIZE_MAX) fallback = o;
        if (o - from > (size_t(1) << 16)) break;  // (do not scan a long unverifiable tail byte by byte)
    }
    return fallback;
}

}  // namespace

// ---- tabix (.tbi) / BAM (.bai) index: where a contig's rows start and end in the file --------
// Both hold, per reference, bins of chunks [virtual begin, virtual end) (virtual = block file
// offset << 16 | offset inside the inflated block).  htslib's pseudo-bin 37450 carries the span of the
// whole reference in its first chunk; without it the span is the hull of the chunks.
namespace {

struct IndexSpan {
    bool usable = false;   // the index could be read
    bool present = false;  // ... and lists the contig with at least one chunk
    uint64_t beg = 0, end = 0;
    // region look-ups (tabix): where the rows that overlap the region start, and where - by the 16 kb linear index -
    // the rows that start behind the region begin (a hint: a row longer than an index window can sit behind it)
    bool region = false;
    uint64_t reg_beg = 0, reg_soft_end = 0;
};

inline uint64_t rd_u64(const uint8_t* p) { return (uint64_t)rd_u32(p) | ((uint64_t)rd_u32(p + 4) << 32); }

// ref < 0: look the contig up by name (tabix); else by reference id (BAI)
IndexSpan index_lookup(const std::string& index_path, bool bai, const std::string& name, int ref, long long reg_start = -1,
                       long long reg_stop = -1) {
    IndexSpan out;
    // The index image (a tabix index inflated) of the file asked for last stays in memory: a whole-genome .tbi is
    // ~1.5 MB to read and inflate - 3 ms on one thread - and region reads ask for it once per region (a rank's two
    // partial contigs, every one-interval API call).  Keyed by path, size and modification time.
    struct Cached {
        std::string path;
        long long size = -1, mtime_ns = 0;
        std::shared_ptr<std::vector<uint8_t>> image;
    };
    static std::mutex cache_mu;
    static Cached cache[2];
    static unsigned cache_turn = 0;
    std::shared_ptr<std::vector<uint8_t>> image;
    struct stat ist;
    if (stat(index_path.c_str(), &ist) != 0) return out;
    const long long isize = (long long)ist.st_size,
                    imtime = (long long)ist.st_mtim.tv_sec * 1000000000LL + (long long)ist.st_mtim.tv_nsec;
    {
        std::lock_guard<std::mutex> lk(cache_mu);
        for (auto& c : cache)
            if (c.image && c.path == index_path && c.size == isize && c.mtime_ns == imtime) image = c.image;
    }
    if (!image) {
        Bytes raw, img;
        if (!read_file(index_path.c_str(), &raw) || raw.size() < 8) return out;
        const Bytes* src = &raw;
        if (!bai) {
            if (inflate_all(raw, 1, &img) != FTK_OK || img.size() < 36) return out;
            src = &img;
        }
        image = std::make_shared<std::vector<uint8_t>>(src->data(), src->data() + src->size());
        std::lock_guard<std::mutex> lk(cache_mu);
        Cached& slot = cache[cache_turn++ & 1u];
        slot.path = index_path;
        slot.size = isize;
        slot.mtime_ns = imtime;
        slot.image = image;
    }
    const uint8_t* p = image->data();
    const size_t n = image->size();
    if (n < 8 || memcmp(p, bai ? "BAI\1" : "TBI\1", 4) != 0) return out;
    if (!bai && n < 36) return out;
    const int32_t n_ref = rd_i32(p + 4);
    size_t o = 8;
    if (!bai) {
        const int32_t l_nm = rd_i32(p + 32);
        o = 36;
        if (l_nm < 0 || o + (size_t)l_nm > n) return out;
        ref = -1;
        int k = 0;
        for (size_t a = o; a < o + (size_t)l_nm && k < n_ref; ++k) {
            const char* nm = (const char*)p + a;
            const size_t len = strnlen(nm, o + l_nm - a);
            if (name.size() == len && memcmp(nm, name.data(), len) == 0) ref = k;
            a += len + 1;
        }
        o += (size_t)l_nm;
        out.usable = true;
        if (ref < 0) return out;  // the file has no such contig
    }
    if (n_ref < 0 || ref >= n_ref) { out.usable = bai; return out; }
    for (int r = 0; r <= ref; ++r) {
        if (o + 4 > n) return IndexSpan{};
        const int32_t n_bin = rd_i32(p + o);
        o += 4;
        uint64_t lo = UINT64_MAX, hi = 0;
        bool pseudo = false;
        for (int32_t b = 0; b < n_bin; ++b) {
            if (o + 8 > n) return IndexSpan{};
            const uint32_t bin = rd_u32(p + o);
            const int32_t n_chunk = rd_i32(p + o + 4);
            o += 8;
            if (n_chunk < 0 || o + 16 * (size_t)n_chunk > n) return IndexSpan{};
            if (r == ref) {
                if (bin == 37450 && n_chunk >= 1) {
                    lo = rd_u64(p + o);
                    hi = rd_u64(p + o + 8);
                    pseudo = true;
                } else if (!pseudo && bin != 37450) {
                    for (int32_t c = 0; c < n_chunk; ++c) {
                        lo = std::min(lo, rd_u64(p + o + 16 * (size_t)c));
                        hi = std::max(hi, rd_u64(p + o + 16 * (size_t)c + 8));
                    }
                }
            }
            o += 16 * (size_t)n_chunk;
        }
        if (o + 4 > n) return IndexSpan{};
        const int32_t n_intv = rd_i32(p + o);
        o += 4;
        if (n_intv < 0 || o + 8 * (size_t)n_intv > n) return IndexSpan{};
        const uint8_t* ioff = p + o;
        o += 8 * (size_t)n_intv;
        if (r == ref) {
            out.usable = true;
            if (lo != UINT64_MAX && hi > lo) { out.present = true; out.beg = lo; out.end = hi; }
            if (out.present && reg_start >= 0 && reg_stop > reg_start && n_intv > 0) {
                // linear index: ioff[w] = the smallest virtual offset of a row that overlaps [w * 16384, (w + 1) * 16384)
                // (0: none seen up to there).  Every row overlapping the region's first base overlaps its window, so
                // nothing before ioff[w0] is needed; rows that START in window w1 = (stop >> 14) + 1 or later lie
                // behind the region.
                const long long w0 = std::min<long long>(reg_start >> 14, n_intv - 1), w1 = (reg_stop >> 14) + 1;
                uint64_t b = rd_u64(ioff + 8 * (size_t)w0);
                out.reg_beg = b >= lo && b < hi ? b : lo;
                uint64_t e = w1 < n_intv ? rd_u64(ioff + 8 * (size_t)w1) : 0;
                out.reg_soft_end = e >= out.reg_beg && e < hi ? e : hi;  // (== : the region lies in a stretch without rows)
                out.region = true;
            }
        }
    }
    return out;
}

std::string index_path_of(const std::string& path, bool bam) {
    if (!bam) return path + ".tbi";
    std::string a = path + ".bai";
    if (FILE* f = fopen(a.c_str(), "rb")) { fclose(f); return a; }
    if (path.size() > 4) return path.substr(0, path.size() - 4) + ".bai";
    return a;
}

}  // namespace

struct ftk_fragstream {
    std::string path, only;
    bool has_only = false, bam = false, bed6 = false;
    // compressed bytes per piece of THIS stream: kStreamPiece, doubled for a large BAM parsed on the device (run_guarded)
    size_t piece_bytes = kStreamPiece;
    int n_threads = 1;
    size_t max_queued = 2;
    FILE* fp = nullptr;
    std::thread producer;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<ftk_fragtable*> ready;
    bool finished = false, stop = false;
    bool consumer_waiting = false;  // ftk_fragstream_next is blocked on an empty queue
    int err = FTK_OK;
    std::string errmsg;
    // BAM header
    std::vector<std::string> ref_names;
    std::vector<int64_t> ref_lens;
    bool header_ready = false;
    double stage_ms[6] = {0, 0, 0, 0, 0, 0};  // read, inflate, parse, merge, emit, other: set when the producer is done
    // BAM records the reference handles differently from "no fragment" (ftk_bamrule.h), met so far: [0] fragments the
    // columns cannot hold (negative start / beyond int32), [1] CIGAR-less read1 with TLEN < 0 (ftk_fragstream_skipped)
    std::atomic<int64_t> skipped[2] = {{0}, {0}};

    // Text files on a stream opened with ftk_fragstream_open_on: the rows are parsed on this GPU
    // (run_text_device) and the tables handed out hold device columns.
    int device = -1;
    int inflate_device = -1;  // BAM streams opened with a device: where run_bam inflates the pieces
    hipStream_t pstream = nullptr;
    bool emit_device(Contig&& ct, bool bam_rows);  // (ftk_stream_sets.inc)
    bool run_text_device(RawBuf& first, size_t first_n);
    // A row / comment line longer than the device carry (kTextCarryMax) cannot be moved from piece to piece on the
    // device: run_text_device then asks for a second pass over the file with the inflate on the host threads (whose
    // carry has no limit); the contigs already handed out are skipped in that pass.
    bool want_host_restart = false, host_inflate_only = false;
    // run_bam_device: a doubled piece outgrew the text a piece may hold - the DEVICE path takes the file once more with
    // standard pieces (contigs handed out already are skipped); only if that fails too does the host decoder take it
    bool want_device_retry = false;
    std::set<std::string> emitted_names;

    // Hand one finished contig to the consumer.  Sorting (BAM), packing into page-locked memory and
    // waiting for queue space happen on a helper thread, one contig at a time (so the order is kept),
    // while the producer already decodes the next contig's pieces.
    std::thread packer;
    std::atomic<int> packer_ok{1};
    bool emit(Contig&& ct) {
        if (packer.joinable()) packer.join();
        if (!packer_ok.load()) return false;
        std::shared_ptr<Contig> held(new Contig(std::move(ct)));
        packer = std::thread([this, held] {
            std::unique_ptr<ftk_fragtable> t(new ftk_fragtable());
            t->bam = bam;
            t->bed6 = bed6;
            t->contigs.push_back(std::move(*held));
            Contig& c = t->contigs[0];
            Stopwatch sw;
            if (!c.parts.empty()) {
                if (bam) pack_bam_parts(c, n_threads);
                else pack_parts(c, n_threads);
                sw.lap(bam ? "packer: sort + gather runs" : "packer: pack runs");
            } else {
                if (bam) sort_by_start(c.c, n_threads);
                sw.lap("packer: sort by start");
                pack(c);
                sw.lap("packer: pack");
            }
            if (!c.p.base) { fail(FTK_ERR_OOM, "out of host memory"); packer_ok = 0; return; }
            if (!queue_table(std::move(t))) packer_ok = 0;
        });
        return true;
    }
    // a finished table into the consumer's queue, when it has room; false: the stream is being closed
    bool queue_table(std::unique_ptr<ftk_fragtable> t) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || ready.size() < max_queued; });
        if (stop) return false;
        ready.push_back(t.release());
        cv.notify_all();
        return true;
    }
    bool flush() {  // wait for the last contig to be queued
        if (packer.joinable()) packer.join();
        return packer_ok.load() != 0;
    }
    bool fail(int code, const char* msg) {
        std::lock_guard<std::mutex> lk(mu);
        if (err == FTK_OK) { err = code; errmsg = msg; }
        return false;
    }
    void run();          // producer thread body: run_guarded() with exceptions turned into a stream error
    void run_guarded();
    bool run_text(RawBuf& first, size_t first_n);
    bool run_bam(RawBuf& first, size_t first_n);
    // BAM with the records parsed ON THE DEVICE (ftk_bamparse.hip): the inflated bytes stay in HBM, the tables handed
    // out hold device columns sorted by fragment start.  A piece whose record chain the device cannot settle (or a
    // header larger than a piece) makes the stream start over on the host path (run_bam), which skips the contigs
    // already handed out (emitted_refs).
    bool run_bam_device(RawBuf& first, size_t first_n);
    std::set<int> emitted_refs;
    // pieces a whole-file read will come to (0 for an index-driven read of a contig or region: short, and its length is
    // not the file's)
    int pieces_expected() const {
        struct stat sb;
        if (read_end >= 0 || !fp || fstat(fileno(fp), &sb) != 0 || !S_ISREG(sb.st_mode) || piece_bytes == 0) return 0;
        return (int)std::min<long long>((long long)sb.st_size / (long long)piece_bytes + 1, 1 << 20);
    }
    // single-contig requests with a usable index: read only the file range holding the contig
    long long read_end = -1;      // file offset to stop reading at (-1: none)
    bool partial_tail_ok = false;  // the range may end inside a block that belongs to the next contig
    size_t first_skip = 0;        // bytes of the first inflated block that precede the contig
    long long first_piece_off = -1;  // file offset of the first piece handed to run_* (-1: unknown)
    // Region reads (ftk_fragstream_open_region, text files with a tabix index): the stream hands out the contig's rows
    // from the first that can overlap [reg_start, reg_stop) to the last that starts before reg_stop - a superset is
    // allowed, nothing of the region may be missing.  The read first stops at the linear index's hint
    // (read_end < hard_read_end); the device parser's rows then say whether the region is complete (a row starting at
    // or behind reg_stop, or another contig's rows, were seen) and the read goes on in steps if not.
    bool has_region = false;
    long long reg_start = 0, reg_stop = 0;
    long long hard_read_end = -1;  // where the contig's rows end (read_end of a whole-contig read)
    bool range_limited = false;    // the last read_piece() came back short because of read_end, not the file's end
    // One piece of the file -> dst; returns the bytes read (short at the end of the file / of the range).
    // FTK_STREAM_RAMP=<bytes>: the first reads of a stream short - that many bytes, then twice as much each time up to
    // piece_bytes.  The idea: a launch of the inflate kernel lasts one block's chain whatever its size, so the first
    // rows would reach HBM after the time it takes to read and send up 4 MB instead of 48 (96 for a large BAM).
    // Measured (tools/env_ab.sh, alternating runs on one box and file): the whole genome 0.123 -> 0.128 s, the 5.9 GB
    // BAM 0.265 -> 0.272 s - the short launches fill the chip worse than the wait they save; OFF by default.  `base`
    // is what a read asks for before any range limit; fewer bytes than that = the file, or the range, ended there
    // (last_want, set by fill()).
    size_t reads_issued = 0, last_want = 0, ahead_want = 0;
    size_t next_want() {
        static const size_t ramp0 = [] {
            const char* e = getenv("FTK_STREAM_RAMP");
            return e ? (size_t)std::max(0ll, atoll(e)) : (size_t)0;
        }();
        size_t w = piece_bytes;
        if (ramp0 && reads_issued < 6) w = std::min(piece_bytes, ramp0 << reads_issued);
        ++reads_issued;
        return w;
    }
    size_t read_piece(uint8_t* dst, size_t base) {
        size_t want = base;
        range_limited = false;
        if (read_end >= 0) {
            const long long pos = ftell(fp);
            want = pos >= read_end ? 0 : (size_t)std::min<long long>((long long)base, read_end - pos);
            range_limited = want < base;
        }
        size_t got = 0;
        bool done = false;
        // threads that copy a piece out of the page cache (one thread: ~6 GB/s).  Four until round 6; with eight the
        // chr1-sized 60x BAM's producer waits 42 ms for its reads instead of 96 and the pass is the GPU's (0.216 ->
        // 0.200 s; sixteen: the same - profiles/r6_read_threads.txt).  FTK_READ_THREADS=<1..16> overrides.
        static const int n_readers = [] {
            const char* e = getenv("FTK_READ_THREADS");
            if (e) return std::max(1, std::min(16, atoi(e)));
            return ftk_host::default_threads() >= 16 ? 8 : 4;
        }();
        if (want >= (size_t(8) << 20) && n_readers > 1) {
            // a large piece of a regular file: the threads pread their shares (one thread copies ~6 GB/s out of
            // the page cache - 8 ms per 48 MB piece, as long as the GPU takes to inflate it)
            const long long pos = ftell(fp);
            struct stat sb;
            if (pos >= 0 && fstat(fileno(fp), &sb) == 0 && S_ISREG(sb.st_mode) && (long long)sb.st_size > pos) {
                const size_t n = (size_t)std::min<long long>((long long)want, (long long)sb.st_size - pos);
                const int kReaders = n_readers;
                std::atomic<int> failed{0};
                auto part = [&](int t) {
                    size_t a = n * (size_t)t / kReaders;
                    const size_t b = n * (size_t)(t + 1) / kReaders;
                    while (a < b) {
                        const ssize_t r = pread(fileno(fp), dst + a, b - a, (off_t)(pos + (long long)a));
                        if (r <= 0) { failed.store(1); return; }
                        a += (size_t)r;
                    }
                };
                std::vector<std::thread> helpers;
                for (int t = 1; t < kReaders; ++t) helpers.emplace_back(part, t);
                part(0);
                for (auto& h : helpers) h.join();
                if (!failed.load() && fseek(fp, (long)(pos + (long long)n), SEEK_SET) == 0) {
                    got = n;
                    done = true;
                } else if (fseek(fp, (long)pos, SEEK_SET) != 0) {
                    return 0;
                }
            }
        }
        if (!done) got = want ? fread(dst, 1, want, fp) : 0;
        if (got == want && want) {
            // ask the kernel for the piece after this one (a hint only; failure is ignored)
            const long long pos = ftell(fp);
            if (pos >= 0) (void)posix_fadvise(fileno(fp), (off_t)pos, (off_t)piece_bytes, POSIX_FADV_WILLNEED);
        }
        return got;
    }
    // Read-ahead: while a piece is inflated and parsed, a helper thread reads the next one into `ahead`,
    // kHead bytes in: the bytes carried over (less than one BGZF block) are put in front of it and the two
    // buffers trade places - the file read (12 GB/s from the page cache, far less from a cold disk)
    // leaves the producer's critical path.  Only the helper touches `fp` while a read is in flight.
    static constexpr size_t kHead = size_t(1) << 16;
    RawBuf ahead;
    std::future<size_t> ahead_got;
    bool ahead_ok = true;  // false while the BAM header is probed before an index seek (the read would be thrown away)
    void start_ahead() {
        if (!ahead_ok || !ahead.reserve(kHead + piece_bytes)) return;
        ahead.head = 0;
        ahead_want = next_want();
        ahead_got = std::async(std::launch::async, [this] { return read_piece(ahead.p + kHead, ahead_want); });
    }
    void drain_ahead() {  // before anything else moves the file position
        if (ahead_got.valid()) (void)ahead_got.get();
    }
    // A text stream sends its GPU pieces up straight from the (page-locked) buffer they were read into.  The copy is
    // asynchronous: the caller hands fill() the event recorded behind it (buf_in_flight), the buffer rests until the
    // event is done, and the next read goes into one that has rested (up to three rest, so the producer never waits).
    struct Resting {
        std::unique_ptr<RawBuf> b;
        hipEvent_t ev;
    };
    std::deque<Resting> resting;
    std::vector<hipEvent_t> up_events;  // idle events of rested buffers
    hipEvent_t buf_in_flight = nullptr;
    hipEvent_t take_up_event() {
        if (!up_events.empty()) {
            hipEvent_t e = up_events.back();
            up_events.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        return e;
    }
    void drop_resting() {
        for (auto& r : resting) {
            if (hipEventSynchronize(r.ev) != hipSuccess) (void)hipGetLastError();
            up_events.push_back(r.ev);
        }
        resting.clear();
        if (buf_in_flight) {
            if (hipEventSynchronize(buf_in_flight) != hipSuccess) (void)hipGetLastError();
            up_events.push_back(buf_in_flight);
        }
        buf_in_flight = nullptr;
        for (hipEvent_t e : up_events) (void)hipEventDestroy(e);
        up_events.clear();
    }
    // read the next piece after the `carry` bytes at the front of buf (at carry_off of buf when a copy of buf is in
    // flight and the caller could not move them); returns bytes now in buf
    size_t fill(RawBuf& buf, size_t carry, size_t carry_off = 0) {
        size_t got;
        if (buf_in_flight && !ahead_got.valid()) {  // no read-ahead to trade places with: wait for the copy
            if (hipEventSynchronize(buf_in_flight) != hipSuccess) (void)hipGetLastError();
            up_events.push_back(buf_in_flight);
            buf_in_flight = nullptr;
        }
        if (ahead_got.valid()) {
            got = ahead_got.get();
            last_want = ahead_want;
            if (carry <= kHead) {
                if (carry) memcpy(ahead.p + kHead - carry, buf.data() + carry_off, carry);
                ahead.head = kHead - carry;
            } else {  // (not with BGZF blocks, which are at most 64 KB)
                if (!ahead.reserve(carry + piece_bytes)) return carry;
                memmove(ahead.p + carry, ahead.p + kHead, got);
                memcpy(ahead.p, buf.data() + carry_off, carry);
                ahead.head = 0;
            }
            buf.swap(ahead);
            if (buf_in_flight) {  // the old buffer rests; the next read goes into one that has rested, or a new one
                resting.push_back({std::unique_ptr<RawBuf>(new RawBuf()), buf_in_flight});
                resting.back().b->swap(ahead);
                buf_in_flight = nullptr;
                ahead.pinned = true;
                if (resting.size() > 3 || hipEventQuery(resting.front().ev) == hipSuccess) {
                    if (hipEventSynchronize(resting.front().ev) != hipSuccess) (void)hipGetLastError();
                    ahead.swap(*resting.front().b);
                    up_events.push_back(resting.front().ev);
                    resting.pop_front();
                } else {
                    (void)hipGetLastError();  // (not ready is no error)
                }
            }
        } else {
            if (carry && carry_off) memmove(buf.data(), buf.data() + carry_off, carry);
            if (!buf.reserve(buf.head + carry + piece_bytes)) return carry;
            last_want = next_want();
            got = read_piece(buf.data() + carry, last_want);
        }
        if (got == last_want) start_ahead();
        return carry + got;
    }
    // seek to a contig's rows; false = index unusable (caller scans the whole file)
    bool seek_to(const IndexSpan& sp) {
        drain_ahead();
        if (fseek(fp, (long)(sp.beg >> 16), SEEK_SET) != 0) return false;
        first_skip = (size_t)(sp.beg & 0xffff);
        read_end = (long long)(sp.end >> 16) + 0x10000 + 64;  // through the block that holds the last row
        hard_read_end = read_end;
        partial_tail_ok = true;
        return true;
    }
    // complete BGZF blocks at the front of buf[0, n): block list + bytes consumed; false on corruption
    bool whole_blocks(const uint8_t* p, size_t n, bool eof, std::vector<Block>* blocks, size_t* used, size_t* total) {
        blocks->clear();
        size_t off = 0, tot = 0;
        while (off < n) {
            size_t bs = 0;
            if (off + 18 > n) break;
            const size_t q = gzip_header(p, n, off, &bs);
            if (q && bs && off + bs <= n) {
                if (q + 8 > off + bs) return false;
                const uint8_t* tr = p + off + bs - 8;
                const size_t isize = (size_t)tr[4] | ((size_t)tr[5] << 8) | ((size_t)tr[6] << 16) | ((size_t)tr[7] << 24);
                if (isize > (size_t(1) << 16)) return false;  // a BGZF block holds at most 64 KB of data (htslib refuses more too)
                blocks->push_back({q, off + bs - 8 - q, tot, isize});
                tot += isize;
                off += bs;
                continue;
            }
            if (p[off] != 31 || p[off + 1] != 139) return false;  // not at a block boundary
            if (q && bs && off + bs > n) break;                     // block continues in the next piece
            if (!q && n - off < (1u << 16)) break;                  // header itself is cut
            return false;
        }
        if (eof && off != n && !partial_tail_ok) return false;  // trailing garbage / truncated last block
        *used = off;
        *total = tot;
        return true;
    }
};

void ftk_fragstream::run_guarded() {
    RawBuf buf;
    ahead_ok = !(bam && has_only);  // run_bam decides about the index seek after the header
    {
        // a region is read as one only where the device inflates and parses the rows (run_text_device tells from the
        // parsed rows whether the region is complete); elsewhere the stream hands out the whole contig - a superset
        static const bool dev_inf = !(getenv("FTK_DEVICE_INFLATE") && atoi(getenv("FTK_DEVICE_INFLATE")) == 0);
        static const bool dev_bam_rec = !(getenv("FTK_DEVICE_BAM_PARSE") && atoi(getenv("FTK_DEVICE_BAM_PARSE")) == 0);
        if (!dev_inf || !has_only || (bam ? (inflate_device < 0 || !dev_bam_rec) : device < 0)) has_region = false;
    }
    if (has_only && !bam) {  // tabix index: jump straight to the contig's rows
        IndexSpan sp = index_lookup(index_path_of(path, false), false, only, -1, has_region ? reg_start : -1, has_region ? reg_stop : -1);
        if (has_region && !(sp.usable && sp.present && sp.region)) has_region = false;  // (the whole contig: a superset)
        if (sp.usable && !sp.present) {  // the file has no row of this contig
            std::lock_guard<std::mutex> lk(mu);
            finished = true;
            header_ready = true;
            cv.notify_all();
            return;
        }
        if (sp.usable && has_region) {
            // start at the region's first row; stop - for now - where the linear index says the rows behind it begin
            sp.beg = sp.reg_beg;
            if (!seek_to(sp)) { read_end = -1; partial_tail_ok = false; first_skip = 0; has_region = false; rewind(fp); }
            else read_end = std::min(hard_read_end, (long long)(sp.reg_soft_end >> 16) + 0x10000 + 64);
        } else if (sp.usable && !seek_to(sp)) { read_end = -1; partial_tail_ok = false; first_skip = 0; rewind(fp); }
    }
    {
        static const bool dev_bam = !(getenv("FTK_DEVICE_BAM_PARSE") && atoi(getenv("FTK_DEVICE_BAM_PARSE")) == 0) &&
                                    !(getenv("FTK_DEVICE_INFLATE") && atoi(getenv("FTK_DEVICE_INFLATE")) == 0);
        if (bam && inflate_device >= 0 && dev_bam && have_hip_device()) {
            buf.pinned = ahead.pinned = true;  // (see RawBuf)
            // A launch of the inflate kernel lasts one block's chain (~4 ms for BAM records) whatever its size, until
            // the chip's 5 120 wavefront slots are full; a 48 MB piece of BAM is ~1 900 blocks, and the stream keeps
            // about two such launches side by side: a third of the slots idle.  Pieces of 96 MB: a chr1-sized 60x
            // BAM 0.266 -> 0.233 s until resident (144 MB: no further gain; text streams, ~3 000 blocks per piece
            // and three fronts side by side, LOSE 5-10 % with larger pieces - tools/piece_size_ab.sh).  Small files
            // keep the short pieces (latency to the first contig); FTK_STREAM_PIECE set by hand wins.
            struct stat sb;
            const bool test_limits = getenv("FTK_TEST_PIECE_LIMIT") != nullptr;  // (tests: the doubling and its overflow on small files)
            if ((!getenv("FTK_STREAM_PIECE") || test_limits) && fstat(fileno(fp), &sb) == 0 &&
                ((long long)sb.st_size >= (1ll << 30) || test_limits))
                piece_bytes = 2 * kStreamPiece;
        }
        // a text stream's GPU pieces go up straight from the read buffer too (FTK_TEXT_DIRECT_UP=0: staged in the buffer
        // sets' own page-locked memory by a copy of the producer's - 0.8 ms per 48 MB piece on 16 threads, and in the
        // way of the host threads' inflate jobs)
        static const bool text_direct = !(getenv("FTK_TEXT_DIRECT_UP") && atoi(getenv("FTK_TEXT_DIRECT_UP")) == 0) &&
                                        !(getenv("FTK_DEVICE_INFLATE") && atoi(getenv("FTK_DEVICE_INFLATE")) == 0);
        if (!bam && device >= 0 && text_direct && have_hip_device()) buf.pinned = ahead.pinned = true;
    }
    first_piece_off = ftell(fp);
    const size_t n = fill(buf, 0);
    size_t bsize = 0;
    const bool bgzf = n >= 18 && gzip_header(buf.data(), n, 0, &bsize) && bsize;
    bool ok;
    if (!bgzf) {
        // not block-compressed (plain gzip): no block parallelism to stream; decode whole and hand out per contig
        drain_ahead();
        fclose(fp);
        fp = nullptr;
        ftk_fragtable* whole = nullptr;
        const int rc = bam ? ftk_bam_decode(path.c_str(), has_only ? only.c_str() : nullptr, n_threads, &whole)
                           : ftk_fragfile_decode(path.c_str(), has_only ? only.c_str() : nullptr, n_threads, &whole);
        if (rc != FTK_OK) {
            fail(rc, g_decode_err.c_str());
        } else {
            bed6 = whole->bed6;
            skipped[0] += whole->skipped[0];
            skipped[1] += whole->skipped[1];
            if (bam) {
                std::lock_guard<std::mutex> lk(mu);
                for (auto& ct : whole->contigs) { ref_names.push_back(ct.name); ref_lens.push_back(ct.length); }
                header_ready = true;
                cv.notify_all();
            }
            for (auto& ct : whole->contigs) {
                Contig copy;
                copy.name = ct.name;
                copy.length = ct.length;
                const Packed& p = ct.p;
                copy.c.start.assign(p.start, p.start + p.rows);
                copy.c.end.assign(p.end, p.end + p.rows);
                copy.c.mapq.assign(p.mapq, p.mapq + p.rows);
                copy.c.strand.assign(p.strand, p.strand + p.rows);
                if (p.r1s) { copy.c.r1s.assign(p.r1s, p.r1s + p.rows); copy.c.r1e.assign(p.r1e, p.r1e + p.rows); }
                if (p.ord) copy.c.ord.assign(p.ord, p.ord + p.rows);
                if (p.rows == 0) continue;
                if (!emit(std::move(copy))) break;
            }
            delete whole;
        }
        ok = true;
    } else {
        static const bool dev_bam_parse = !(getenv("FTK_DEVICE_BAM_PARSE") && atoi(getenv("FTK_DEVICE_BAM_PARSE")) == 0) &&
                                          !(getenv("FTK_DEVICE_INFLATE") && atoi(getenv("FTK_DEVICE_INFLATE")) == 0);
        const bool bam_on_device = bam && inflate_device >= 0 && dev_bam_parse;
        ok = bam ? (bam_on_device ? run_bam_device(buf, n) : run_bam(buf, n)) : device >= 0 ? run_text_device(buf, n) : run_text(buf, n);
        bool stopped;
        {
            std::lock_guard<std::mutex> lk(mu);
            stopped = stop || err != FTK_OK;
        }
        auto rewind_whole = [&] {
            drain_ahead();
            if (pstream) (void)hipStreamSynchronize(pstream);
            has_region = false;  // (the second pass hands out whole contigs)
            read_end = -1;
            partial_tail_ok = false;
            first_skip = 0;
            ahead_ok = !has_only;
            reads_issued = 0;
            // the second pass parses every record of the file again, those of the contigs handed out included
            skipped[0] = 0;
            skipped[1] = 0;
            rewind(fp);
        };
        if (!ok && want_device_retry && !stopped && bam) {
            want_device_retry = false;
            rewind_whole();
            const size_t n2 = fill(buf, 0);
            ok = run_bam_device(buf, n2);
            std::lock_guard<std::mutex> lk(mu);
            stopped = stop || err != FTK_OK;
        }
        if (!ok && want_host_restart && !stopped && bam) {
            // (see run_bam_device) the file once more on the host decoder; contigs handed out already are skipped
            drain_ahead();
            if (pstream) (void)hipStreamSynchronize(pstream);
            want_host_restart = false;
            has_region = false;  // (the host decoder hands out the whole contig)
            read_end = -1;
            partial_tail_ok = false;
            first_skip = 0;
            ahead_ok = !has_only;
            skipped[0] = 0;  // (run_bam counts every contig's records again, those handed out included)
            skipped[1] = 0;
            rewind(fp);
            const size_t n2 = fill(buf, 0);
            ok = run_bam(buf, n2);
        } else if (!ok && want_host_restart && !stopped) {
            // (see want_host_restart) the same range of the file once more, inflated by the host threads
            drain_ahead();
            (void)hipStreamSynchronize(pstream);
            host_inflate_only = true;
            has_region = false;  // (the second pass hands out the whole contig)
            read_end = -1;
            partial_tail_ok = false;
            first_skip = 0;
            rewind(fp);
            if (has_only) {
                const IndexSpan sp = index_lookup(index_path_of(path, false), false, only, -1);
                if (sp.usable && sp.present && !seek_to(sp)) { read_end = -1; partial_tail_ok = false; first_skip = 0; rewind(fp); }
            }
            first_piece_off = ftell(fp);
            const size_t n2 = fill(buf, 0);
            ok = run_text_device(buf, n2);
        }
    }
    (void)ok;
    flush();
    std::lock_guard<std::mutex> lk(mu);
    finished = true;
    header_ready = true;
    cv.notify_all();
}

void ftk_fragstream::run() {
    try {
        run_guarded();
        return;
    } catch (const std::exception& ex) {
        fail(FTK_ERR_OOM, ex.what());
    }
    std::lock_guard<std::mutex> lk(mu);
    finished = true;
    header_ready = true;
    cv.notify_all();
}

namespace {
struct StageClock {  // where the producer thread of the streaming decoder spends its time (ftk_fragstream_stage_ms;
                     // FTK_DECODE_TIMING=1 also prints it)
    bool on = getenv("FTK_DECODE_TIMING") != nullptr;
    ftk_fragstream* owner;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    explicit StageClock(ftk_fragstream* s) : owner(s) {}
    void lap(int k) {
        auto now = std::chrono::steady_clock::now();
        acc[k] += std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
    }
    void report(const char* what) {
        {
            std::lock_guard<std::mutex> lk(owner->mu);
            for (int k = 0; k < 6; ++k) owner->stage_ms[k] = acc[k];
        }
        if (!on) return;
        fprintf(stderr, "[ftk stream %s] read %.1f  inflate %.1f  parse %.1f  merge %.1f  emit(pack+queue) %.1f  other %.1f ms\n",
                what, acc[0], acc[1], acc[2], acc[3], acc[4], acc[5]);
    }
};
}  // namespace
