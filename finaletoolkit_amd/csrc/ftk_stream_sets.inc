// Part of ftk_decode.cpp's translation unit (#included there, in this order: core, sets, text, bam, api) - what the device routes (`run_text_device`, `run_bam`, `run_bam_device`) share: the buffer sets and their pools, the front streams, and ONE statement of each step of staging a piece (block table, staging copy, host-share inflate job, front enqueue, host piece up, inflate verdict), the BED6 sniff, the ring guards and the hand-over of a device-resident contig.

namespace {
// One of the two buffer sets of the device row parser: page-locked host text (the inflate target and the
// DMA source), the device copy, the kernels' scratch and outputs, and the summary that comes back.
struct DevSet {
    uint8_t* h_text = nullptr;  // page-locked twin of d_text: only where the host touches a piece's text (its own share
                                // of the inflate, a piece of odd rows, the host-parse streams) - see ensure_host_text
    size_t h_text_cap = 0;
    uint8_t* d_text = nullptr;
    size_t cap = 0, max_lines = 0;
    void* d_blocks = nullptr;   // the row parser's scan state (ftk::textparse_scratch_bytes)
    int32_t *d_s = nullptr, *d_e = nullptr;
    uint8_t *d_q = nullptr, *d_t = nullptr;
    ftk::TextSummary* d_sum = nullptr;
    ftk::TextSummary* h_sum = nullptr;
    hipEvent_t done = nullptr;
    hipEvent_t front = nullptr;  // the piece's bytes are on the device, inflated, CRCs computed (the set's own stream)
    hipEvent_t freed = nullptr;  // the appends that read the set's columns last have run (parse stream)
    bool freed_valid = false;
    bool pending = false;
    bool host_only = false;   // the piece was not sent to the device (4 GB or more: the kernels index with 32 bits)
    size_t off = 0, len = 0;  // the launched range of h_text (complete lines)
    bool cut_tail = false;    // last piece of an index-driven read that may stop inside a row (ignore that one row)
    // pieces inflated on the device (FTK_DEVICE_INFLATE): compressed bytes, block table, per-block CRCs, status
    bool inflated = false;
    uint8_t* d_comp = nullptr;
    uint8_t* h_comp = nullptr;  // page-locked copy of the compressed piece (BAM path; text pieces stage in h_text)
    size_t h_comp_cap = 0;
    size_t comp_cap = 0, tab_cap = 0, n_tab = 0;
    ftk::InflateBlock *d_tab = nullptr, *h_tab = nullptr;
    uint32_t *d_crc = nullptr, *h_crc = nullptr, *want_crc = nullptr;  // want_crc: the blocks' trailers (plain host memory)
    ftk::InflateStatus *d_ist = nullptr, *h_ist = nullptr;

    // BAM pieces parsed on the device (ftk_bamparse.hip): the extra row columns, the stretch scratch, the summary
    int32_t *d_r1s = nullptr, *d_r1e = nullptr, *d_ref = nullptr;
    uint32_t* d_stretch = nullptr;
    size_t stretch_words = 0, bam_rows = 0;
    ftk::BamSummary *d_bsum = nullptr, *h_bsum = nullptr;
    void release_bam() {
        for (void* q : {(void*)d_r1s, (void*)d_r1e, (void*)d_ref, (void*)d_stretch, (void*)d_bsum})
            if (q) (void)hipFree(q);
        if (h_bsum) (void)hipHostFree(h_bsum);
        d_r1s = d_r1e = d_ref = nullptr;
        d_stretch = nullptr;
        d_bsum = h_bsum = nullptr;
        stretch_words = bam_rows = 0;
    }
    // call after ensure(): columns for max_lines rows, stretch scratch for `bytes` of records
    bool ensure_bam(size_t bytes, uint32_t stretch_bytes) {
        const size_t words = ftk::bam_stretch_words(bytes, stretch_bytes);
        if (bam_rows >= max_lines && stretch_words >= words && d_bsum) return true;
        release_bam();
        const bool ok = hipMalloc((void**)&d_r1s, max_lines * 4) == hipSuccess && hipMalloc((void**)&d_r1e, max_lines * 4) == hipSuccess &&
                        hipMalloc((void**)&d_ref, max_lines * 4) == hipSuccess &&
                        hipMalloc((void**)&d_stretch, (words + words / 4) * 4) == hipSuccess &&
                        hipMalloc((void**)&d_bsum, sizeof(ftk::BamSummary)) == hipSuccess &&
                        hipHostMalloc((void**)&h_bsum, sizeof(ftk::BamSummary), hipHostMallocDefault) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            release_bam();
            return false;
        }
        bam_rows = max_lines;
        stretch_words = words + words / 4;
        return true;
    }

    void release_inflate() {
        for (void* q : {(void*)d_comp, (void*)d_tab})  // (d_crc / d_ist lie in d_tab's block, h_crc / h_ist in h_tab's)
            if (q) (void)hipFree(q);
        if (h_tab) (void)hipHostFree(h_tab);
        pinned_unmap(h_comp);
        free(want_crc);
        d_comp = h_comp = nullptr; d_tab = h_tab = nullptr; d_crc = h_crc = want_crc = nullptr; d_ist = h_ist = nullptr;
        comp_cap = tab_cap = h_comp_cap = 0;
    }
    void release() {
        release_inflate();
        release_bam();
        if (h_text) pinned_unmap(h_text);
        h_text_cap = 0;
        if (h_sum) (void)hipHostFree(h_sum);
        for (void* q : {(void*)d_text, (void*)d_blocks, (void*)d_s, (void*)d_e, (void*)d_q, (void*)d_t, (void*)d_sum})
            if (q) (void)hipFree(q);
        for (hipEvent_t ev : {done, front, freed})
            if (ev) (void)hipEventDestroy(ev);
        *this = DevSet{};
    }
    bool ensure_host_comp(size_t comp_bytes) {
        if (comp_bytes <= h_comp_cap) return true;
        if (h_comp) pinned_unmap(h_comp);
        h_comp = nullptr;
        h_comp_cap = comp_bytes + comp_bytes / 4 + 4096;
        if ((h_comp = (uint8_t*)pinned_map(h_comp_cap)) == nullptr) {
            h_comp_cap = 0;
            return false;
        }
        return true;
    }
    // room for a piece of comp_bytes of BGZF data in n_blocks blocks
    bool ensure_inflate(size_t comp_bytes, size_t n_blocks) {
        bool ok = true;
        if (comp_bytes + 64 > comp_cap) {
            if (d_comp) (void)hipFree(d_comp);
            d_comp = nullptr;
            comp_cap = comp_bytes + comp_bytes / 4 + 4096;
            ok = hipMalloc((void**)&d_comp, comp_cap) == hipSuccess;
        }
        if (ok && (n_blocks > tab_cap || !d_ist)) {  // (also a piece without a complete block: the status words are still used)
            const size_t cc = comp_cap, hc = h_comp_cap;
            uint8_t *keep = d_comp, *keep_h = h_comp;
            d_comp = h_comp = nullptr;
            release_inflate();
            d_comp = keep;
            comp_cap = cc;
            h_comp = keep_h;
            h_comp_cap = hc;
            tab_cap = n_blocks + n_blocks / 4 + 64;
            want_crc = (uint32_t*)malloc(tab_cap * 4);
            // block table | CRCs | status, ONE device block and ONE page-locked block (d_tab / h_tab are their bases): a
            // small hipHostMalloc costs 1-8 ms in a process's first pass, a small hipMalloc ~1 ms, and a text stream's
            // twelve sets made three of each
            auto up = [](size_t v) { return (v + 255) / 256 * 256; };
            const size_t o_crc = up(tab_cap * sizeof(ftk::InflateBlock)), o_ist = o_crc + up(tab_cap * 4);
            const size_t all = o_ist + up(sizeof(ftk::InflateStatus));
            ok = want_crc && hipMalloc((void**)&d_tab, all) == hipSuccess &&
                 hipHostMalloc((void**)&h_tab, all, hipHostMallocDefault) == hipSuccess;
            if (ok) {
                d_crc = (uint32_t*)((char*)d_tab + o_crc);
                d_ist = (ftk::InflateStatus*)((char*)d_tab + o_ist);
                h_crc = (uint32_t*)((char*)h_tab + o_crc);
                h_ist = (ftk::InflateStatus*)((char*)h_tab + o_ist);
            }
        }
        if (!ok) {
            (void)hipGetLastError();
            release_inflate();
        }
        return ok;
    }
    // page-locked room for `bytes` of text on the host side (page-locking 250 MB takes ~25 ms: a text stream whose
    // pieces stay on the device never pays it - the first whole-genome pass of a process spent 0.2 s here for its
    // sets)
    bool ensure_host_text(size_t bytes) {
        if (bytes <= h_text_cap) return true;
        if (h_text) pinned_unmap(h_text);
        h_text = nullptr;
        h_text_cap = std::max(bytes + bytes / 4 + 4096, cap);
        if ((h_text = (uint8_t*)pinned_map(h_text_cap)) == nullptr) {
            h_text_cap = 0;
            return false;
        }
        return true;
    }
    // room for `bytes` of text; false: out of (page-locked or device) memory
    bool ensure(size_t bytes, bool with_host_text = true) {
        if (bytes <= cap) return !with_host_text || ensure_host_text(bytes);
        release();
        const size_t want = bytes + bytes / 4 + 4096;
        const size_t lines = want / 10 + 1;  // a plain row is at least 10 bytes; more lines -> the host parses the piece
        bool ok = (!with_host_text || ensure_host_text(want)) &&
                  hipHostMalloc((void**)&h_sum, sizeof(ftk::TextSummary), hipHostMallocDefault) == hipSuccess &&
                  hipMalloc((void**)&d_text, want) == hipSuccess &&
                  hipMalloc((void**)&d_blocks, ftk::textparse_scratch_bytes(want)) == hipSuccess &&
                  hipMalloc((void**)&d_s, lines * 4) == hipSuccess && hipMalloc((void**)&d_e, lines * 4) == hipSuccess &&
                  hipMalloc((void**)&d_q, lines) == hipSuccess && hipMalloc((void**)&d_t, lines) == hipSuccess &&
                  hipMalloc((void**)&d_sum, sizeof(ftk::TextSummary)) == hipSuccess &&
                  hipEventCreateWithFlags(&done, hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&front, hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&freed, hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            release();
            return false;
        }
        cap = want;
        max_lines = lines;
        return true;
    }
    // call after ensure_inflate(): the device's block table of a piece whose compressed bytes lie at `src` and whose
    // text starts text_base bytes into d_text (the room in front is the carry's), and the CRCs its blocks' trailers ask for
    void set_block_table(const std::vector<Block>& blocks, const uint8_t* src, size_t text_base) {
        for (size_t i = 0; i < blocks.size(); ++i) {
            const Block& bl = blocks[i];
            h_tab[i] = {(uint32_t)bl.in_off, (uint32_t)bl.in_len, (uint32_t)(text_base + bl.out_off), (uint32_t)bl.out_len};
            want_crc[i] = trailer_crc(src + bl.in_off + bl.in_len);
        }
        n_tab = blocks.size();
    }
    // a settled piece (h_ist and h_crc are back): did the device inflate every block, and to the bytes its trailer asks for?
    // (a piece the host threads inflated has n_tab == 0 and a cleared status: ok)
    enum class Inflate { ok, bad_block, crc_mismatch };
    Inflate inflate_verdict() const {
        if (h_ist->n_bad) return Inflate::bad_block;
        for (size_t i = 0; i < n_tab; ++i)
            if (h_crc[i] != want_crc[i]) return Inflate::crc_mismatch;
        return Inflate::ok;
    }
};
// The two buffer sets of a finished stream wait here for the next one: allocating them costs ~100 ms (400 MB
// of page-locked memory, ~1 GB of device memory, the frees synchronise the device) - more than a small file
// takes to decode.  At most twelve idle sets are kept (per process, any device): the ring of a text stream.
struct DevSetPool {
    std::mutex mu;
    std::vector<std::pair<int, DevSet>> idle;
    DevSet take(int device) {
        std::lock_guard<std::mutex> lk(mu);
        for (size_t i = 0; i < idle.size(); ++i)
            if (idle[i].first == device) {
                DevSet s = idle[i].second;
                idle.erase(idle.begin() + i);
                return s;
            }
        return DevSet{};
    }
    void give(int device, DevSet& s) {
        s.pending = false;
        s.freed_valid = false;  // (the giver has synchronised its streams)
        {
            std::lock_guard<std::mutex> lk(mu);
            if (s.cap && idle.size() < 12) {
                idle.emplace_back(device, s);
                s = DevSet{};
                return;
            }
        }
        s.release();
    }
    size_t trim() {  // release every idle set; returns their page-locked + device bytes (text buffers only: a lower bound)
        std::vector<std::pair<int, DevSet>> drop;
        {
            std::lock_guard<std::mutex> lk(mu);
            drop.swap(idle);
        }
        size_t n = 0;
        for (auto& d : drop) {
            (void)hipSetDevice(d.first);
            n += d.second.cap + d.second.h_text_cap + d.second.h_comp_cap + d.second.comp_cap;
            d.second.release();
        }
        return n;
    }
};
DevSetPool& devset_pool() {
    static DevSetPool* p = new DevSetPool();  // leaked: the driver frees at process exit
    return *p;
}

// HIP streams of finished decoder streams wait here for the next one: creating one costs ~1 ms, destroying it as
// much, a decoder stream uses five - a fifth of the time a small file takes from disk to results.  A stream is idle
// (synchronised) when it is given back.
struct StreamPool {
    std::mutex mu;
    std::vector<std::pair<int, hipStream_t>> idle;
    hipStream_t take(int device) {  // nullptr: cannot create one
        {
            std::lock_guard<std::mutex> lk(mu);
            for (size_t i = 0; i < idle.size(); ++i)
                if (idle[i].first == device) {
                    hipStream_t s = idle[i].second;
                    idle.erase(idle.begin() + i);
                    return s;
                }
        }
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        return s;
    }
    hipStream_t take_idle(int device) {  // an idle one or nullptr - never creates
        std::lock_guard<std::mutex> lk(mu);
        for (size_t i = 0; i < idle.size(); ++i)
            if (idle[i].first == device) {
                hipStream_t s = idle[i].second;
                idle.erase(idle.begin() + i);
                return s;
            }
        return nullptr;
    }
    void fill_to(int device, int n) {  // idle streams of `device` up to n (a helper thread's job: see FrontStreams::prefill)
        for (;;) {
            {
                std::lock_guard<std::mutex> lk(mu);
                int have = 0;
                for (auto& e : idle) have += e.first == device;
                if (have >= n || idle.size() >= 16) return;
            }
            hipStream_t s = nullptr;
            if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
                (void)hipGetLastError();
                return;
            }
            give(device, s);
        }
    }
    void give(int device, hipStream_t s) {
        if (!s) return;
        {
            std::lock_guard<std::mutex> lk(mu);
            if (idle.size() < 16) {
                idle.emplace_back(device, s);
                return;
            }
        }
        (void)hipStreamDestroy(s);
    }
    size_t trim() {
        std::vector<std::pair<int, hipStream_t>> drop;
        {
            std::lock_guard<std::mutex> lk(mu);
            drop.swap(idle);
        }
        for (auto& d : drop) {
            (void)hipSetDevice(d.first);
            (void)hipStreamDestroy(d.second);
        }
        return drop.size();
    }
};
StreamPool& stream_pool() {
    static StreamPool* p = new StreamPool();  // leaked: the driver frees at process exit
    return *p;
}

// The front streams of a decoder stream's ring, created when a piece first needs one.  With sixteen hardware queues
// (GPU_MAX_HW_QUEUES, see _hardware_queues) a NEW stream costs 5.5 ms - its queue is set up with it - and a decoder
// stream that opened its whole ring up front spent 72 of the 80 ms a small file takes in a fresh process on thirteen
// hipStreamCreateWithFlags (profiles/r4_cold_start.txt); a file of one piece needs one.  Streams of earlier decoder
// streams come back from the pool at no cost, so a warm process sees no difference.  If a stream cannot be created
// the piece runs on `fallback` (the parse stream): ordering is by events, so that only serialises it.
template <int N>
struct FrontStreams {
    int device = -1;
    hipStream_t fallback = nullptr;
    hipStream_t s[N] = {};
    // In a fresh process the pool is empty and the helper thread (prefill) needs ~10 ms per stream, while the producer
    // asks for a new slot's stream every 2 ms: a slot whose stream is not there yet BORROWS one a neighbour holds (its
    // front then queues behind that neighbour's - ordering is by events, so that only serialises the two) instead of
    // creating one itself, and takes its own the next time round.  Round 6: a first whole-genome text pass spent 85 of
    // its 170 ms waiting in hipStreamCreateWithFlags (profiles/r6_first_pass_hip.txt).
    hipStream_t get(int k) {
        if (s[k]) return s[k];
        if ((s[k] = stream_pool().take_idle(device)) != nullptr) return s[k];
        for (int d = 1; d < N; ++d)
            if (s[(k + N - d) % N]) return s[(k + N - d) % N];
        if ((s[k] = stream_pool().take(device)) == nullptr) return fallback;  // the very first stream: made here
        return s[k];
    }
    // A file of many pieces will use the whole ring: a helper thread creates the streams the pool lacks while the
    // producer reads and launches the first pieces (each get() then finds one idle instead of spending 5.5 ms).
    std::thread filler;
    void prefill(int n) {
        if (n <= 0 || filler.joinable()) return;
        const int dev = device;
        filler = std::thread([dev, n] {
            if (hipSetDevice(dev) == hipSuccess) stream_pool().fill_to(dev, std::min(n, N));
        });
    }
    void settle_and_give() {  // (the caller has set the device)
        if (filler.joinable()) filler.join();
        for (auto& q : s)
            if (q) {
                (void)hipStreamSynchronize(q);
                stream_pool().give(device, q);
                q = nullptr;
            }
    }
};

// ---- staging a piece: ONE statement of each step the device routes share -------------------------------------------
// A piece's FRONT (its set's own stream): compressed bytes up, inflate, CRC - or, for a piece the host threads inflate,
// their text up.  Its BACK (the parse stream, in file order): the row / record parser and the appends.

// a piece's compressed bytes into page-locked memory, one thread per MB
void stage_bytes(uint8_t* dst, const uint8_t* src, size_t used, int n_threads) {
    const int nt = std::max(1, std::min(n_threads, (int)(used >> 20) + 1));
    parallel_run(nt, [&](int t) {
        const size_t a = used * (size_t)t / nt, b = used * (size_t)(t + 1) / nt;
        memcpy(dst + a, src + a, b - a);
    });
}

// The host threads' share: the piece's blocks inflated from `comp` into `out` (both page-locked buffers of the piece's
// set), CRCs checked like the GPU's pieces.  The job owns its block list.  file_off >= 0: it first reads its own copy of
// the `used` compressed bytes from the file (page cache), four pread threads; < 0: the caller has staged them.
std::future<int> start_host_inflate(std::vector<Block> blocks, uint8_t* comp, uint8_t* out, int n_threads, int fd, size_t used,
                                    long long file_off) {
    return std::async(std::launch::async, [bl = std::move(blocks), comp, out, nt = std::max(1, n_threads - 2), fd, used, file_off] {
        if (file_off >= 0) {
            std::atomic<int> bad{0};
            std::vector<std::thread> th;
            auto part = [&](int t) {
                size_t a = used * (size_t)t / 4;
                const size_t e = used * (size_t)(t + 1) / 4;
                while (a < e) {
                    const ssize_t r = pread(fd, comp + a, e - a, (off_t)(file_off + (long long)a));
                    if (r <= 0) { bad.store(1); return; }
                    a += (size_t)r;
                }
            };
            for (int t = 1; t < 4; ++t) th.emplace_back(part, t);
            part(0);
            for (auto& t : th) t.join();
            if (bad.load()) return (int)FTK_ERR_IO;
        }
        return bl.empty() ? (int)FTK_OK : inflate_block_list(comp, bl, nt, out, true, true);
    });
}

// The front of a GPU piece on `st`: the `used` compressed bytes at `src` up (up_ev, when given, recorded behind that
// copy: the read buffer they came from may be reused), the block table up, inflate + CRC, S.front recorded.
// (the compressed bytes go up at once - nothing of the set's previous piece uses d_comp any more - and only the
// inflate, which overwrites the text the appends may still read, waits for the set's release)
// tev (FTK_DECODE_TIMING, else nullptr): [0] front start, [1] front end, [4] bytes up.
bool enqueue_front(hipStream_t st, DevSet& S, const uint8_t* src, size_t used, size_t n_blocks, hipEvent_t up_ev, bool vector_matches,
                   hipEvent_t* tev) {
    bool ok = (!tev || hipEventRecord(tev[0], st) == hipSuccess) &&
              (used == 0 || hipMemcpyAsync(S.d_comp, src, used, hipMemcpyHostToDevice, st) == hipSuccess) &&
              (!up_ev || hipEventRecord(up_ev, st) == hipSuccess) &&
              (!S.freed_valid || hipStreamWaitEvent(st, S.freed, 0) == hipSuccess) &&
              hipMemsetAsync(S.d_ist, 0, sizeof(ftk::InflateStatus), st) == hipSuccess &&
              (n_blocks == 0 || hipMemcpyAsync(S.d_tab, S.h_tab, n_blocks * sizeof(ftk::InflateBlock), hipMemcpyHostToDevice, st) == hipSuccess) &&
              (!tev || hipEventRecord(tev[4], st) == hipSuccess);
    if (ok) {
        ftk::inflate_launch(st, S.d_comp, S.d_tab, (int)n_blocks, S.d_text, S.d_ist, S.d_crc, vector_matches);
        ok = hipGetLastError() == hipSuccess && (!tev || hipEventRecord(tev[1], st) == hipSuccess) &&
             hipEventRecord(S.front, st) == hipSuccess;
    }
    return ok;
}

// The front of a piece the host threads inflated: its `total` bytes of text up on `st`, behind the appends that read
// the set last, S.front recorded (its CRCs were checked by the job: the status the back copies home is a cleared one).
bool upload_host_piece(hipStream_t st, DevSet& S, size_t text_base, size_t total, hipEvent_t* tev) {
    return (!S.freed_valid || hipStreamWaitEvent(st, S.freed, 0) == hipSuccess) &&
           (!tev || hipEventRecord(tev[0], st) == hipSuccess) &&
           hipMemsetAsync(S.d_ist, 0, sizeof(ftk::InflateStatus), st) == hipSuccess &&
           (total == 0 || hipMemcpyAsync(S.d_text + text_base, S.h_text + text_base, total, hipMemcpyHostToDevice, st) == hipSuccess) &&
           (!tev || (hipEventRecord(tev[4], st) == hipSuccess && hipEventRecord(tev[1], st) == hipSuccess)) &&
           hipEventRecord(S.front, st) == hipSuccess;
}

// io/alignment.py:143-156: BED6 when the first data row (not empty, no '#' comment) of [b, e) has > 5 columns.  A
// row without its line end counts only with unterminated_ok (the text may be cut there).  True: *bed6 is known.
bool sniff_bed6(const char* b, const char* e, bool unterminated_ok, bool* bed6) {
    for (const char* q = b; q < e;) {
        const char* nl = (const char*)memchr(q, '\n', (size_t)(e - q));
        const char* le = nl ? nl : e;
        if (le > q && *q != '#' && (nl || unterminated_ok)) {
            int tabs = 0;
            for (const char* x = q; x < le; ++x) tabs += (*x == '\t');
            *bed6 = (tabs + 1) > 5;
            return true;
        }
        if (!nl) break;
        q = nl + 1;
    }
    return false;
}

// ---- the guards of a route's ring (declared in this order, so that they go in the reverse one) ----------------------
struct AtExit {  // what a route has to give back AFTER its ring is idle (timing events, a device array)
    std::function<void()> f;
    ~AtExit() { f(); }
};
template <int N>
struct RingCleanup {  // the ring's streams and sets back to their pools
    DevSet* s;
    int device;
    hipStream_t pst;
    FrontStreams<N>* fs;
    bool on = true;
    ~RingCleanup() {
        if (!on) return;
        fs->settle_and_give();
        (void)hipStreamSynchronize(pst);  // nothing in flight touches the sets any more
        for (int k = 0; k < N; ++k) devset_pool().give(device, s[k]);
    }
};
struct JobGuard {  // no job outlives the buffers it works on
    std::future<int>* j;
    int n;
    ~JobGuard() {
        for (int i = 0; i < n; ++i)
            if (j[i].valid()) (void)j[i].get();
    }
};
// (a GPU piece's compressed bytes go up straight from the page-locked read buffer; fill() lets that buffer rest
// until the copy is done - see buf_in_flight)
struct RestGuard {  // waits for the copies that still read a resting buffer
    ftk_fragstream* s;
    ~RestGuard() { s->drop_resting(); }
};
}  // namespace

// A finished, device-resident contig -> the consumer (bam_rows: a BAM contig, sorted, with the read1 spans and the
// file-order rank beside the four columns).
bool ftk_fragstream::emit_device(Contig&& ct, bool bam_rows) {
    DevColumns& d = *ct.dev;
    if (hipEventCreateWithFlags(&d.ready, hipEventDisableTiming) != hipSuccess || hipEventRecord(d.ready, pstream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FTK_ERR_HIP, "cannot record the contig's ready event");
    }
    std::unique_ptr<ftk_fragtable> t(new ftk_fragtable());
    t->bam = bam_rows;
    t->bed6 = !bam_rows && bed6;
    ct.p.rows = d.rows;
    ct.p.start = d.start;
    ct.p.end = d.end;
    ct.p.mapq = d.mapq;
    ct.p.strand = d.strand;
    ct.p.r1s = d.r1s;  // (nullptr in a text contig's block)
    ct.p.r1e = d.r1e;
    ct.p.ord = d.ord;
    if (!bam_rows) emitted_names.insert(ct.name);  // (a BAM contig: emitted_refs, by the caller)
    t->contigs.push_back(std::move(ct));
    return queue_table(std::move(t));
}
