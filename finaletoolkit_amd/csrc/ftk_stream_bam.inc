// Part of ftk_decode.cpp's translation unit (#included there, in this order: core, sets, text, bam, api) - BAM streams: `run_bam` (host record walk over speculative stretches) and `run_bam_device` (device inflate + the record parser of ftk_bamparse.hip; the record rule itself: ftk_bamrule.h).

bool ftk_fragstream::run_bam(RawBuf& buf, size_t n_first) {
    StageClock clk(this);
    size_t n_stretches = 0, n_redone = 0;
    RawBuf data;                // carry (partial record / header) + this piece's inflated bytes (host inflate)
    std::vector<uint8_t> carry_buf;  // the same carry while the pieces are inflated on the device
    size_t carry = 0;
    bool header_done = false;
    std::vector<int> wanted;    // ref id -> 1 when selected
    Contig cur;
    size_t cur_rows = 0;
    int cur_ref = -1;
    std::set<int> seen;
    size_t pending_skip = 0;
    // One piece of the file: compressed bytes in buf[0, n), its whole BGZF blocks, and (device inflate) the slot
    // that inflates it.
    struct Piece {
        size_t n = 0, used = 0, total = 0;
        bool eof = false, listed = false;
        std::vector<Block> blocks;
        int slot = -1;
    };
    // Device inflate (default on a stream that knows its GPU; FTK_DEVICE_INFLATE=0: host threads): the blocks of
    // pieces k+1 .. k+kAhead are inflated on the GPU and copied back while the host walks the records of piece k.
    // One slot and one HIP stream per piece in flight: a 48 MB piece holds ~800 blocks = 800 wavefronts, a
    // quarter of what the chip holds at this kernel's occupancy, and a block's decode chain takes the same ~6.5 ms
    // whether the chip is full or not - so three pieces' kernels (and their copies, either direction) run side by
    // side.  A slot's output is page-locked memory with room in front for the carry.
    constexpr size_t kRoom = size_t(32) << 20;
    constexpr int kAhead = 7, kSlots = kAhead + 1;
    static const bool want_dinf = !(getenv("FTK_DEVICE_INFLATE") && atoi(getenv("FTK_DEVICE_INFLATE")) == 0);
    const int device = inflate_device;  // (shadows the member: this path's GPU)
    bool dinf = want_dinf && device >= 0;
    FrontStreams<kSlots> streams;  // (slot 0 runs on the member pstream, which is destroyed with the stream object)
    if (dinf) {
        const bool ok = hipSetDevice(device) == hipSuccess && (pstream || (pstream = stream_pool().take(device)) != nullptr);
        if (!ok) {
            (void)hipGetLastError();
            dinf = false;
        }
        streams.device = device;
        streams.fallback = pstream;
        if (dinf) streams.prefill(std::min(pieces_expected(), kSlots) - 1);
    }
    DevSet sets[kSlots];
    if (dinf)
        for (auto& S : sets) S = devset_pool().take(device);
    RingCleanup<kSlots> cleanup{sets, device, pstream, &streams, dinf};
    // Every third piece of the look-ahead is inflated by the host threads instead (straight into its slot's
    // page-locked output, while the GPU works on the two in front of it): the chip turns a 64 KB block of BAM over
    // every 2.7 us = 24 GB/s of records, the 16 threads manage 11 GB/s, and between record walks they have nothing
    // else to do.  FTK_BAM_HOST_SHARE=<n>: every n-th piece (0: none).
    static const int host_share = [] {
        const char* e = getenv("FTK_BAM_HOST_SHARE");
        return e ? atoi(e) : 3;
    }();
    bool slot_on_host[kSlots] = {};
    std::future<int> host_job[kSlots];  // the host threads' inflate of a slot's piece (from the slot's own copy of the bytes)
    JobGuard job_guard{host_job, kSlots};
    auto submit = [&](Piece& pc, int index) -> bool {  // index: the piece's number among the submitted ones
        const int slot = index % kSlots;
        DevSet& S = sets[slot];
        hipStream_t pstream = slot ? streams.get(slot) : this->pstream;  // (shadows the member: this slot's stream)
        if (pc.total + kRoom + 64 >= (size_t(1) << 32)) return fail(FTK_ERR_FORMAT, "BGZF piece too large");
        slot_on_host[slot] = host_share > 0 && header_done && (index % host_share) == host_share - 1;
        if (slot_on_host[slot]) {
            if (!S.ensure(kRoom + pc.total + 64) || !S.ensure_host_comp(pc.used + 64))
                return fail(FTK_ERR_OOM, "out of page-locked memory for the BAM piece");
            stage_bytes(S.h_comp, buf.data(), pc.used, n_threads);
            // (the job owns its block list; the bytes stay in the slot until the piece has been walked)
            host_job[slot] = start_host_inflate(pc.blocks, S.h_comp, S.h_text + kRoom, n_threads, -1, pc.used, -1);
            pc.slot = slot;
            return true;
        }
        if (!S.ensure(kRoom + pc.total + 64) || !S.ensure_inflate(pc.used, pc.blocks.size()) || !S.ensure_host_comp(pc.used + 64))
            return fail(FTK_ERR_OOM, "out of page-locked / device memory for the BAM piece");
        stage_bytes(S.h_comp, buf.data(), pc.used, n_threads);
        S.set_block_table(pc.blocks, buf.data(), kRoom);
        // (not enqueue_front: this route copies the text BACK for the host's record walk and records S.done)
        bool ok = hipMemsetAsync(S.d_ist, 0, sizeof(ftk::InflateStatus), pstream) == hipSuccess &&
                  (pc.used == 0 || hipMemcpyAsync(S.d_comp, S.h_comp, pc.used, hipMemcpyHostToDevice, pstream) == hipSuccess) &&
                  (pc.blocks.empty() || hipMemcpyAsync(S.d_tab, S.h_tab, pc.blocks.size() * sizeof(ftk::InflateBlock),
                                                       hipMemcpyHostToDevice, pstream) == hipSuccess);
        if (ok) {
            ftk::inflate_launch(pstream, S.d_comp, S.d_tab, (int)pc.blocks.size(), S.d_text, S.d_ist, S.d_crc, /*vector_matches=*/true);
            ok = hipGetLastError() == hipSuccess &&
                 (pc.total == 0 || hipMemcpyAsync(S.h_text + kRoom, S.d_text + kRoom, pc.total, hipMemcpyDeviceToHost, pstream) == hipSuccess) &&
                 hipMemcpyAsync(S.h_ist, S.d_ist, sizeof(ftk::InflateStatus), hipMemcpyDeviceToHost, pstream) == hipSuccess &&
                 (pc.blocks.empty() || hipMemcpyAsync(S.h_crc, S.d_crc, pc.blocks.size() * 4, hipMemcpyDeviceToHost, pstream) == hipSuccess) &&
                 hipEventRecord(S.done, pstream) == hipSuccess;
        }
        if (!ok) {
            (void)hipGetLastError();
            return fail(FTK_ERR_HIP, "cannot launch the device inflate");
        }
        pc.slot = slot;
        return true;
    };
    auto wait_slot = [&](int slot) -> bool {
        DevSet& S = sets[slot];
        if (slot_on_host[slot]) {  // inflated by the host threads
            if (host_job[slot].valid() && host_job[slot].get() != FTK_OK)
                return fail(FTK_ERR_FORMAT, "BGZF inflate failed or block CRC mismatch (host share of a device stream)");
            return true;
        }
        if (hipEventSynchronize(S.done) != hipSuccess) {
            (void)hipGetLastError();
            return fail(FTK_ERR_HIP, "the device inflate failed");
        }
        const DevSet::Inflate verdict = S.inflate_verdict();
        if (verdict == DevSet::Inflate::bad_block) return fail(FTK_ERR_FORMAT, "BGZF inflate failed");
        if (verdict == DevSet::Inflate::crc_mismatch) return fail(FTK_ERR_FORMAT, "BGZF block CRC mismatch (device inflate)");
        return true;
    };
    auto list_blocks = [&](Piece& pc) -> bool {
        if (pc.listed) return true;
        if (!whole_blocks(buf.data(), pc.n, pc.eof, &pc.blocks, &pc.used, &pc.total)) return fail(FTK_ERR_FORMAT, "corrupt BGZF block");
        pc.listed = true;
        return true;
    };
    Piece curp;
    std::deque<Piece> ahead;  // pieces behind curp that are already on the device, in file order
    curp.n = n_first;
    curp.eof = n_first < last_want;
    int n_submitted = 0;
    for (;;) {
        if (!list_blocks(curp)) return false;
        if (dinf && curp.slot < 0 && !submit(curp, n_submitted++)) return false;
        // read the next pieces and start their inflate before this piece's records are walked (not while the header
        // is still being probed: an index seek may throw those reads away).  `buf` holds the compressed bytes of the
        // piece read last - the newest of `ahead`, or curp.
        if (dinf && header_done) {
            while ((int)ahead.size() < kAhead) {
                const Piece& last = ahead.empty() ? curp : ahead.back();
                if (last.eof) break;
                const size_t raw_carry = last.n - last.used;
                if (raw_carry) memmove(buf.data(), buf.data() + last.used, raw_carry);
                clk.lap(5);
                Piece np;
                np.n = fill(buf, raw_carry);
                clk.lap(0);
                np.eof = np.n - raw_carry < last_want;
                if (!list_blocks(np) || !submit(np, n_submitted++)) return false;
                ahead.push_back(std::move(np));
            }
        }
        size_t& n = curp.n;
        bool& eof = curp.eof;
        const size_t used = curp.used, total = curp.total;
        const uint8_t* p;
        clk.lap(5);
        if (dinf) {
            if (carry > kRoom) return fail(FTK_ERR_FORMAT, "a BAM header or record of more than 32 MB: set FTK_DEVICE_INFLATE=0");
            if (!wait_slot(curp.slot)) return false;
            uint8_t* base = sets[curp.slot].h_text + kRoom - carry;
            if (carry) memcpy(base, carry_buf.data(), carry);
            p = base;
        } else {
            if (!data.reserve(carry + total + 1)) return fail(FTK_ERR_OOM, "out of host memory");
            if (!curp.blocks.empty() && inflate_block_list(buf.data(), curp.blocks, n_threads, data.data() + carry) != FTK_OK)
                return fail(FTK_ERR_FORMAT, "BGZF inflate failed");
            p = data.data();
        }
        clk.lap(1);
        const size_t m = carry + total;
        size_t off = std::min(pending_skip, m);  // (a damaged index may point past the block)
        pending_skip = 0;
        if (!header_done) {
            bool complete = false;
            do {
                if (m < 12) break;
                if (memcmp(p, "BAM\1", 4) != 0) return fail(FTK_ERR_FORMAT, (path + " is not a BAM file").c_str());
                size_t o = 4;
                const uint32_t l_text = rd_u32(p + o);
                o += 4 + (size_t)l_text;
                if (o + 4 > m) break;
                const uint32_t n_ref = rd_u32(p + o);
                o += 4;
                std::vector<std::string> names;
                std::vector<int64_t> lens;
                bool cut = false;
                for (uint32_t r = 0; r < n_ref; ++r) {
                    if (o + 4 > m) { cut = true; break; }
                    const uint32_t l_name = rd_u32(p + o);
                    o += 4;
                    if (l_name == 0) return fail(FTK_ERR_FORMAT, "corrupt BAM reference list");
                    if (o + l_name + 4 > m) { cut = true; break; }
                    names.emplace_back((const char*)p + o, l_name - 1);
                    o += l_name;
                    lens.push_back(rd_i32(p + o));
                    o += 4;
                }
                if (cut) break;
                {
                    std::lock_guard<std::mutex> lk(mu);
                    ref_names = names;
                    ref_lens = lens;
                    header_ready = true;
                    cv.notify_all();
                }
                wanted.assign(n_ref, 0);
                for (uint32_t r = 0; r < n_ref; ++r) wanted[r] = !has_only || names[r] == only;
                off = o;
                complete = true;
            } while (false);
            if (!complete) {
                if (eof) return fail(FTK_ERR_FORMAT, "truncated BAM header");
                carry = m;  // need more bytes: keep everything
                if (dinf) carry_buf.assign(p, p + m);
                goto next_piece;
            }
            header_done = true;
            ahead_ok = true;
            if (has_only) {  // BAI: jump to the contig's records instead of walking the whole file
                int target = -1;
                for (size_t r = 0; r < ref_names.size(); ++r)
                    if (ref_names[r] == only) target = (int)r;
                if (target < 0) return true;  // not in the header: nothing to hand out
                const IndexSpan sp = index_lookup(index_path_of(path, true), true, std::string(), target);
                if (sp.usable && !sp.present) return true;  // no alignment on this contig
                if (sp.usable && seek_to(sp)) {
                    carry = 0;
                    curp = Piece{};
                    curp.n = fill(buf, 0);
                    curp.eof = curp.n < last_want;
                    pending_skip = first_skip;
                    first_skip = 0;
                    continue;
                }
                read_end = -1;
                partial_tail_ok = false;
                first_skip = 0;
            }
        }
        {
            // The records form a chain (each starts where the previous one ends), and walking it is one
            // dependent cache miss per record - ~80 ns x millions.  So the piece is cut into byte ranges:
            // every thread GUESSES the first record start in its range (header plausibility, three links
            // deep), walks and parses from there; afterwards the chain is checked range by range - a range
            // whose guessed start is not where the previous range's walk ended is redone from the true
            // offset.  The result never depends on the guess, only the speed does.
            const int n_ref = (int)wanted.size();
            const int nseg = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_threads, (m - off) / kBamStretch + 1));
            struct Stretch {
                size_t start = SIZE_MAX, landing = 0;
                bool bad = false;
                std::vector<BamRun> runs;
            };
            std::vector<Stretch> seg(nseg);
            auto walk = [&](size_t from, size_t until, Stretch& st) {
                st.runs.clear();
                st.bad = false;
                st.start = from;
                BamRun* run = nullptr;
                size_t o = from;
                while (o < until && o + 4 <= m) {
                    const uint32_t bs = rd_u32(p + o);
                    if (bs < 32) { st.bad = true; break; }
                    if (o + 4 + (size_t)bs > m) break;  // incomplete: waits for the next piece
                    const uint8_t* r = p + o + 4;
                    const int32_t ref_id = rd_i32(r);
                    if (ref_id >= 0 && ref_id < n_ref && wanted[ref_id]) {
                        if (!run || run->ref != ref_id) {
                            st.runs.push_back(BamRun{ref_id, {}});
                            run = &st.runs.back();
                            // both mates of a pair are at least ~150 bytes each: room for the rest of the stretch
                            const size_t guess = (until > o ? until - o : 0) / 300 + 16;
                            run->c.start.reserve(guess);
                            run->c.end.reserve(guess);
                            run->c.mapq.reserve(guess);
                            run->c.strand.reserve(guess);
                            run->c.r1s.reserve(guess);
                            run->c.r1e.reserve(guess);
                        }
                        bam_record(r, bs, run->c);
                    }
                    o += 4 + (size_t)bs;
                }
                st.landing = o;
            };
            auto bound = [&](int k) { return k >= nseg ? m : off + (m - off) * (size_t)k / (size_t)nseg; };
            parallel_run(nseg, [&](int k) {
                const size_t from = k == 0 ? off : guess_record_start(p, bound(k), m, n_ref);
                if (from == SIZE_MAX) return;  // nothing that looks like a record: settled by the check below
                walk(from, bound(k + 1), seg[k]);
            });
            clk.lap(2);
            size_t o = off;
            for (int k = 0; k < nseg; ++k) {
                ++n_stretches;
                if (seg[k].start != o || seg[k].bad) {
                    ++n_redone;
                    if (clk.on && getenv("FTK_DECODE_TIMING")[0] >= '2')
                        fprintf(stderr, "[ftk stream bam] stretch %d of %d redone: guessed %zd, chain at %zu, bound %zu, piece %zu bytes%s\n", k, nseg,
                                seg[k].start == SIZE_MAX ? (ssize_t)-1 : (ssize_t)seg[k].start, o, bound(k), m, seg[k].bad ? " (bad)" : "");
                    walk(o, bound(k + 1), seg[k]);
                    if (seg[k].bad) return fail(FTK_ERR_FORMAT, "corrupt BAM record");
                }
                o = seg[k].landing;
            }
            if (eof && o != m && !partial_tail_ok) return fail(FTK_ERR_FORMAT, "truncated BAM record");
            clk.lap(5);  // "other" holds the chain check (and any redone range)
            for (auto& st : seg)
                for (auto& r : st.runs) {
                    // (counted for every contig: a pass that takes over from the device pass counts the file anew)
                    skipped[0] += r.c.skipped[0];
                    skipped[1] += r.c.skipped[1];
                    if (emitted_refs.count(r.ref)) continue;  // handed out by the device pass this one replaces
                    if (cur_ref >= 0 && r.ref != cur_ref) {
                        clk.lap(3);
                        if (cur_rows && !emit(std::move(cur))) return false;
                        clk.lap(4);
                        cur = Contig{};
                        cur_rows = 0;
                        cur_ref = -1;
                    }
                    if (cur_ref < 0) {
                        if (!seen.insert(r.ref).second)
                            return fail(FTK_ERR_UNSORTED, ("contig " + ref_names[r.ref] + " appears in two separate runs: the BAM is not coordinate-sorted").c_str());
                        cur_ref = r.ref;
                        cur.name = ref_names[r.ref];
                        cur.length = ref_lens[r.ref];
                    }
                    cur_rows += r.c.start.size();
                    if (!r.c.start.empty()) cur.parts.push_back(std::move(r.c));  // sorted / gathered by the packer
                }
            clk.lap(3);
            carry = m - o;
            if (dinf) carry_buf.assign(p + o, p + o + carry);
            else if (carry) memmove(data.data(), p + o, carry);
        }
    next_piece:
        if (eof) break;
        if (!ahead.empty()) {
            curp = std::move(ahead.front());
            ahead.pop_front();
        } else {
            const size_t raw_carry = n - used;
            if (raw_carry) memmove(buf.data(), buf.data() + used, raw_carry);
            clk.lap(5);
            Piece np;
            np.n = fill(buf, raw_carry);
            clk.lap(0);
            np.eof = np.n - raw_carry < last_want;
            curp = std::move(np);
        }
        {
            std::lock_guard<std::mutex> lk(mu);
            if (stop) return false;
        }
    }
    clk.lap(5);
    if (cur_ref >= 0 && cur_rows && !emit(std::move(cur))) return false;
    clk.lap(4);
    clk.report("bam");
    if (clk.on) fprintf(stderr, "[ftk stream bam] %zu stretches of the record chain, %zu redone after the chain check\n", n_stretches, n_redone);
    return true;
}

bool ftk_fragstream::run_bam_device(RawBuf& buf, size_t n_first) {
    StageClock clk(this);
    const int device = inflate_device;
    constexpr size_t kRoom = size_t(32) << 20;
    constexpr int kAhead = 7, kSlots = kAhead + 1;  // (3 ahead: the 60x slice 0.050 s; 5: 0.038-0.044; 7: 0.036-0.042)
    // bytes of records per thread of the chain walk (FTK_BAM_DEV_STRETCH: tests walk tiny stretches).  A thread follows
    // its stretch's records link by link - dependent loads - so shorter stretches are shorter chains on more threads,
    // until the guesses at their starts and the fix passes cost more than they save: the 5.9 GB BAM, warm passes
    // alternated on one box (tools/env_ab.sh), 32 KB 0.284-0.300 s, 16 KB (rounds 3-4) 0.253-0.287, 8 KB 0.248-0.269,
    // 4 KB 0.250-0.270, 2 KB 0.254-0.268, 1 KB 0.283-0.314
    static const uint32_t stretch_bytes = [] {
        const char* e = getenv("FTK_BAM_DEV_STRETCH");
        const long v = e ? atol(e) : 0;
        return (uint32_t)(v >= 64 ? v : 8192);
    }();
    if (hipSetDevice(device) != hipSuccess || (!pstream && (pstream = stream_pool().take(device)) == nullptr)) {
        (void)hipGetLastError();
        return fail(FTK_ERR_HIP, "cannot create the parse stream");
    }
    FrontStreams<kSlots> streams;
    streams.device = device;
    streams.fallback = pstream;
    streams.prefill(std::min(pieces_expected(), kSlots) - 1);
    DevSet sets[kSlots];
    for (auto& S : sets) S = devset_pool().take(device);
    uint8_t* d_wanted = nullptr;
    AtExit free_wanted{[&] {
        if (d_wanted) (void)hipFree(d_wanted);
    }};
    RingCleanup<kSlots> cleanup{sets, device, pstream, &streams};

    struct Piece {
        size_t n = 0, used = 0, total = 0;
        bool eof = false;
        std::vector<Block> blocks;
        int slot = -1;
        uint32_t first_off = 0;
        bool has_prev = false;
        int prev_slot = -1;
        long long file_off = -1; // where the piece's first byte lies in the file (-1: unknown)
        bool on_host = false;    // inflated by the host threads (its text goes up before the parse)
        bool back_done = false;  // the parse is on the parse stream
    };
    // Every third piece is inflated by the host threads beside the GPU (the chip turns BAM blocks over at ~24 GB/s,
    // the 16 threads manage ~11 GB/s and have nothing else to do now that the records stay on the device); its text
    // goes up in one DMA before its parse.  FTK_BAM_HOST_SHARE=<n>: every n-th piece (0: none).
    // Only with enough threads to keep up: a rank of eight on a 16-core quota has two, and a piece that took 10 ms
    // on fourteen threads would hold the pipeline for 70.
    static const int host_share_env = [] {
        const char* e = getenv("FTK_BAM_HOST_SHARE");
        return e ? atoi(e) : -1;
    }();
    // (round 5, with the lane-parallel inflate loop - tools/env_ab.sh bam, five runs each on one box, warm passes of the
    // 5.9 GB file: none 0.238-0.251 s, every 32nd 0.221-0.241, every 16th 0.214-0.225, 12th 0.253-0.258, 8th 0.251-0.281,
    // 6th - the default of round 4 - 0.234-0.249, 4th 0.31-0.33)
    const int host_share = host_share_env >= 0 ? host_share_env : (n_threads >= 8 ? 16 : 0);
    std::future<int> host_job[kSlots];
    JobGuard job_guard{host_job, kSlots};
    RestGuard rest_guard{this};
    double t_jobwait = 0, t_front = 0, t_header = 0;  // FTK_DECODE_TIMING: what "other" is made of
    auto tick = [] { return std::chrono::steady_clock::now(); };
    auto since = [](std::chrono::steady_clock::time_point t0) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    auto list_blocks = [&](Piece& pc) -> bool {
        if (!whole_blocks(buf.data(), pc.n, pc.eof, &pc.blocks, &pc.used, &pc.total)) return fail(FTK_ERR_FORMAT, "corrupt BGZF block");
        return true;
    };
    // front of a piece (its slot's own stream): compressed bytes up, inflate, CRC
    auto submit_front = [&](Piece& pc, int index) -> bool {
        const auto t_in = tick();
        struct Acc { double* d; std::chrono::steady_clock::time_point t0; ~Acc() { *d += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); } } acc{&t_front, t_in};
        const int slot = index % kSlots;
        DevSet& S = sets[slot];
        hipStream_t st = streams.get(slot);
        if (S.pending) return fail(FTK_ERR_HIP, "buffer ring out of step");
        // The doubled pieces of a large BAM (run_guarded) assume records that deflate 3-5 x.  The first pieces of a
        // stream are short (the read ramp): one that inflates 16 x or more says the file is of another kind (synthetic,
        // all-N reads), and the stream goes on with the standard pieces before a 96 MB piece can outgrow the 4 GiB a
        // piece's text may take.
        const bool read_doubled = piece_bytes > kStreamPiece;  // (this piece was read at the doubled size)
        if (index == 0 && piece_bytes > kStreamPiece && pc.used > 0 && pc.total / pc.used >= 16) piece_bytes = kStreamPiece;
        // (bytes of text one piece may inflate to: the parsers address a piece with 32 bits; FTK_TEST_PIECE_LIMIT lets a
        //  test meet the limit with a small file)
        static const size_t piece_text_limit = [] {
            const char* e = getenv("FTK_TEST_PIECE_LIMIT");
            const long long v = e ? atoll(e) : 0;
            return v > 0 ? (size_t)v : (size_t(1) << 32);
        }();
        if (pc.total + kRoom + 64 >= piece_text_limit) {
            if (read_doubled) {
                // a file whose compression rises behind its first piece: a doubled piece does not fit, a standard one
                // does - the device path starts over with standard pieces, skipping the contigs handed out
                if (clk.on)
                    fprintf(stderr, "[ftk stream bam] piece %d: %zu bytes of records from %zu compressed do not fit a piece's text (%zu): "
                                    "the device path starts over with standard pieces\n", index, pc.total, pc.used, piece_text_limit);
                piece_bytes = kStreamPiece;
                want_device_retry = true;
                return false;
            }
            return fail(FTK_ERR_FORMAT, "BGZF piece too large");
        }
        pc.on_host = host_share > 0 && index > 0 && (index % host_share) == host_share - 1;
        // a GPU piece goes up straight from the (page-locked) read buffer; the host threads work on their own copy of
        // theirs, which they read from the file (page cache) themselves when the piece's file offset is known
        hipEvent_t up_ev = (buf.pinned && !pc.on_host) ? take_up_event() : nullptr;
        const bool direct = up_ev != nullptr;
        const bool job_reads = pc.on_host && pc.file_off >= 0;
        if (!S.ensure(kRoom + pc.total + 64, false) || (pc.on_host && !S.ensure_host_text(kRoom + pc.total + 64)) ||
            !S.ensure_inflate(pc.used, pc.blocks.size()) || (!direct && !S.ensure_host_comp(pc.used + 64)) ||
            !S.ensure_bam(kRoom + pc.total + 64, stretch_bytes))
            return fail(FTK_ERR_OOM, "out of page-locked / device memory for the BAM piece");
        if (!direct && !job_reads) stage_bytes(S.h_comp, buf.data(), pc.used, n_threads);
        S.set_block_table(pc.blocks, buf.data(), kRoom);
        pc.slot = slot;
        if (pc.on_host) {
            // (the job owns its block list; compressed bytes and output are the slot's page-locked buffers)
            host_job[slot] = start_host_inflate(pc.blocks, S.h_comp, S.h_text + kRoom, n_threads, fileno(fp), pc.used,
                                                job_reads ? pc.file_off : -1);
            return true;
        }
        const bool ok = enqueue_front(st, S, direct ? buf.data() : S.h_comp, pc.used, pc.blocks.size(), up_ev, /*vector_matches=*/true, nullptr);
        if (direct) buf_in_flight = up_ev;  // (fill() parks the buffer behind it)
        if (!ok) {
            (void)hipGetLastError();
            return fail(FTK_ERR_HIP, "cannot launch the device inflate");
        }
        return true;
    };
    // back of a piece (the parse stream, piece after piece): the record chain behind the previous piece's
    int n_ref = 0;
    auto submit_back = [&](Piece& pc) -> bool {
        DevSet& S = sets[pc.slot];
        DevSet* P = pc.has_prev ? &sets[pc.prev_slot] : nullptr;
        if (pc.on_host) {  // the host threads' text goes up on the slot's stream (behind the appends that read the set last)
            hipStream_t st = streams.get(pc.slot);
            const auto t0 = tick();
            const int jrc = host_job[pc.slot].valid() ? host_job[pc.slot].get() : (int)FTK_OK;
            t_jobwait += since(t0);
            if (jrc != FTK_OK)
                return fail(FTK_ERR_FORMAT, "BGZF inflate failed or block CRC mismatch (host share of a device stream)");
            if (!upload_host_piece(st, S, kRoom, pc.total, nullptr)) {
                (void)hipGetLastError();
                return fail(FTK_ERR_HIP, "cannot send a host-inflated piece to the device");
            }
            S.n_tab = 0;  // (its CRCs were checked by the host job)
        }
        bool ok = hipMemsetAsync(S.d_bsum, 0, sizeof(ftk::BamSummary), pstream) == hipSuccess &&
                  hipStreamWaitEvent(pstream, S.front, 0) == hipSuccess;
        if (ok) {
            ftk::bamparse_launch(pstream, S.d_text, (uint32_t)kRoom, (uint32_t)pc.total, P ? P->d_text : nullptr, P ? P->d_bsum : nullptr,
                                 pc.first_off, d_wanted, n_ref, stretch_bytes, S.d_stretch, S.stretch_words, S.max_lines, S.d_s,
                                 S.d_e, S.d_q, S.d_t, S.d_r1s, S.d_r1e, S.d_ref, S.d_bsum);
            ok = hipGetLastError() == hipSuccess &&
                 hipMemcpyAsync(S.h_bsum, S.d_bsum, sizeof(ftk::BamSummary), hipMemcpyDeviceToHost, pstream) == hipSuccess &&
                 hipMemcpyAsync(S.h_ist, S.d_ist, sizeof(ftk::InflateStatus), hipMemcpyDeviceToHost, pstream) == hipSuccess &&
                 (S.n_tab == 0 || hipMemcpyAsync(S.h_crc, S.d_crc, S.n_tab * 4, hipMemcpyDeviceToHost, pstream) == hipSuccess) &&
                 hipEventRecord(S.done, pstream) == hipSuccess;
        }
        if (!ok) {
            (void)hipGetLastError();
            return fail(FTK_ERR_HIP, "cannot launch the device record parser");
        }
        if (P) {  // the previous piece's text has been read (the carry): its slot may take a new piece behind this point
            P->freed_valid = hipEventRecord(P->freed, pstream) == hipSuccess;
            if (!P->freed_valid) {
                (void)hipGetLastError();
                return fail(FTK_ERR_HIP, "cannot record a buffer set's release");
            }
        }
        S.pending = true;
        pc.back_done = true;
        return true;
    };

    // ---- the header: the first piece is inflated on the device, its head copied back until the header is complete
    int region_ref = -1;                // (region reads) the reference the region lies on
    unsigned long long last_key = 0;    // the last record settled so far: (reference << 32) | position
    Piece curp;
    curp.n = n_first;
    curp.eof = n_first < last_want;
    curp.file_off = 0;  // (run_guarded read the first piece from the start of the file)
    int n_submitted = 0;
    if (!list_blocks(curp)) return false;
    std::deque<Piece> ahead;  // pieces behind curp whose fronts (and, in file order, backs) are enqueued
    auto read_ahead_fronts = [&]() -> bool {  // read the next pieces and start their inflate
        while ((int)ahead.size() < kAhead) {
            const Piece& last = ahead.empty() ? curp : ahead.back();
            if (last.eof) break;
            const size_t raw_carry = last.n - last.used;
            // (with a copy of buf in flight the carried bytes are only read: fill() moves them into the next buffer)
            const size_t carry_at = buf_in_flight ? last.used : 0;
            if (raw_carry && !buf_in_flight) memmove(buf.data(), buf.data() + last.used, raw_carry);
            clk.lap(5);
            Piece np;
            np.n = fill(buf, raw_carry, carry_at);
            clk.lap(0);
            np.eof = np.n - raw_carry < last_want;
            np.has_prev = true;
            np.prev_slot = last.slot;
            np.file_off = last.file_off >= 0 ? last.file_off + (long long)last.used : -1;
            if (!list_blocks(np) || !submit_front(np, n_submitted++)) return false;
            ahead.push_back(std::move(np));
        }
        return true;
    };

    std::vector<int> wanted;
    const auto t_head0 = tick();
    {
        // The header sits in the first BGZF blocks: those are inflated right here on the host (a few blocks of 64 KB,
        // microseconds) so that the pipeline does not wait for the first piece's trip through the device.
        std::vector<uint8_t> head;
        size_t nb = 0, o = 0;
        bool complete = false;
        while (!complete) {
            const size_t take = std::min(curp.blocks.size(), std::max<size_t>(2 * nb, 4));
            if (take == nb) {  // the header does not end inside the first piece: the host path
                if (curp.eof) return fail(FTK_ERR_FORMAT, "truncated BAM header");
                want_host_restart = true;
                return false;
            }
            nb = take;
            std::vector<Block> first(curp.blocks.begin(), curp.blocks.begin() + nb);
            const size_t m = first.back().out_off + first.back().out_len;
            head.resize(m + 1);
            if (inflate_block_list(buf.data(), first, std::min(n_threads, 4), head.data()) != FTK_OK)
                return fail(FTK_ERR_FORMAT, "BGZF inflate failed");
            const uint8_t* p = head.data();
            do {
                if (m < 12) break;
                if (memcmp(p, "BAM\1", 4) != 0) return fail(FTK_ERR_FORMAT, (path + " is not a BAM file").c_str());
                o = 4;
                const uint32_t l_text = rd_u32(p + o);
                o += 4 + (size_t)l_text;
                if (o + 4 > m) break;
                const uint32_t nr = rd_u32(p + o);
                o += 4;
                std::vector<std::string> names;
                std::vector<int64_t> lens;
                bool cut = false;
                for (uint32_t r = 0; r < nr; ++r) {
                    if (o + 4 > m) { cut = true; break; }
                    const uint32_t l_name = rd_u32(p + o);
                    o += 4;
                    if (l_name == 0) return fail(FTK_ERR_FORMAT, "corrupt BAM reference list");
                    if (o + l_name + 4 > m) { cut = true; break; }
                    names.emplace_back((const char*)p + o, l_name - 1);
                    o += l_name;
                    lens.push_back(rd_i32(p + o));
                    o += 4;
                }
                if (cut) break;
                {
                    std::lock_guard<std::mutex> lk(mu);
                    ref_names = names;
                    ref_lens = lens;
                    header_ready = true;
                    cv.notify_all();
                }
                wanted.assign(nr, 0);
                for (uint32_t r = 0; r < nr; ++r) wanted[r] = !has_only || names[r] == only;
                complete = true;
            } while (false);
        }
        n_ref = (int)wanted.size();
        std::vector<uint8_t> w8(std::max<size_t>(wanted.size(), 1), 0);
        for (size_t r = 0; r < wanted.size(); ++r) w8[r] = (uint8_t)wanted[r];
        if (hipMalloc((void**)&d_wanted, w8.size()) != hipSuccess ||
            hipMemcpy(d_wanted, w8.data(), w8.size(), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            return fail(FTK_ERR_OOM, "out of device memory");
        }
        curp.first_off = (uint32_t)o;
        ahead_ok = true;
        if (has_only) {  // BAI: jump to the contig's records instead of walking the whole file
            int target = -1;
            for (size_t r = 0; r < ref_names.size(); ++r)
                if (ref_names[r] == only) target = (int)r;
            if (target < 0) return true;
            IndexSpan sp = index_lookup(index_path_of(path, true), true, std::string(), target, has_region ? reg_start : -1,
                                        has_region ? reg_stop : -1);
            if (sp.usable && !sp.present) return true;
            if (has_region && !(sp.usable && sp.region)) has_region = false;  // (the whole contig: a superset)
            if (has_region) sp.beg = sp.reg_beg;  // start at the first record that overlaps the region ...
            region_ref = target;
            if (sp.usable && seek_to(sp)) {
                // ... and stop - for now - where the linear index says the records behind it begin
                if (has_region) read_end = std::min(hard_read_end, (long long)(sp.reg_soft_end >> 16) + 0x10000 + 64);
                const long long seek_pos = ftell(fp);
                curp = Piece{};
                curp.n = fill(buf, 0);
                curp.eof = curp.n < last_want;
                curp.file_off = seek_pos;
                curp.first_off = (uint32_t)first_skip;
                first_skip = 0;
                if (!list_blocks(curp)) return false;
            } else {
                read_end = -1;
                partial_tail_ok = false;
                first_skip = 0;
                has_region = false;
            }
        } else {
            has_region = false;
        }
    }
    if (!submit_front(curp, n_submitted++) || !submit_back(curp)) return false;
    t_header = since(t_head0);

    // ---- the pieces ---------------------------------------------------------------------------------------------
    Contig cur;
    bool have_cur = false;
    int cur_ref = -1;
    std::set<int> seen;
    size_t n_pieces = 0, n_rows_total = 0, n_records = 0;
    auto finish_contig = [&]() -> bool {  // sort the finished contig's rows by fragment start and hand it out
        if (!have_cur) return true;
        clk.lap(3);
        DevColumns& U = *cur.dev;
        const size_t n = U.rows;
        bool ok = true;
        if (n) {
            std::shared_ptr<DevColumns> sorted(new DevColumns());
            sorted->device = device;
            sorted->bam = true;
            const size_t tmp_bytes = ftk::bam_sort_tmp_bytes(n);
            size_t tmp_cap = 0;
            void* tmp = device_cache().take(tmp_bytes, device, &tmp_cap, false);
            ok = tmp && sorted->reserve(n, pstream, true) &&
                 ftk::bam_sort_contig(pstream, n, U.start, U.end, U.mapq, U.strand, U.r1s, U.r1e, sorted->start, sorted->end,
                                      sorted->mapq, sorted->strand, sorted->r1s, sorted->r1e, sorted->ord, tmp, tmp_bytes) == 0 &&
                 hipGetLastError() == hipSuccess && hipStreamSynchronize(pstream) == hipSuccess;  // the unsorted block and the scratch go back
            if (tmp) device_cache().give(tmp, tmp_cap, device);
            if (!ok) {
                (void)hipGetLastError();
                return fail(FTK_ERR_OOM, "cannot sort the contig's rows on the device");
            }
            sorted->rows = n;
            if (hipEventCreateWithFlags(&U.ready, hipEventDisableTiming) == hipSuccess) (void)hipEventRecord(U.ready, pstream);
            cur.dev = sorted;
            emitted_refs.insert(cur_ref);
            if (!emit_device(std::move(cur), true)) return false;
        }
        cur = Contig{};
        have_cur = false;
        cur_ref = -1;
        clk.lap(4);
        return true;
    };
    auto take_run = [&](int ref, DevSet& S, size_t r0, size_t r1) -> bool {
        if (r1 <= r0) return true;
        if (emitted_refs.count(ref)) return true;  // (a second pass over the file: handed out by the first)
        if (have_cur && ref != cur_ref && !finish_contig()) return false;
        if (!have_cur) {
            if (!seen.insert(ref).second)
                return fail(FTK_ERR_UNSORTED, ("contig " + ref_names[ref] + " appears in two separate runs: the BAM is not coordinate-sorted").c_str());
            cur_ref = ref;
            cur.name = ref_names[ref];
            cur.length = ref_lens[ref];
            cur.dev.reset(new DevColumns());
            cur.dev->device = device;
            cur.dev->bam = true;
            have_cur = true;
        }
        if (!cur.dev->append(S.d_s + r0, S.d_e + r0, S.d_q + r0, S.d_t + r0, r1 - r0, hipMemcpyDeviceToDevice, pstream, S.d_r1s + r0,
                             S.d_r1e + r0))
            return fail(FTK_ERR_OOM, "out of device memory for the contig's columns");
        return true;
    };
    auto settle = [&](Piece& pc) -> bool {
        DevSet& S = sets[pc.slot];
        if (hipEventSynchronize(S.done) != hipSuccess) {
            (void)hipGetLastError();
            return fail(FTK_ERR_HIP, "the device record parser failed");
        }
        clk.lap(1);
        S.pending = false;
        const DevSet::Inflate verdict = S.inflate_verdict();  // (a host-inflated piece: a cleared status, no table)
        if (verdict == DevSet::Inflate::bad_block) return fail(FTK_ERR_FORMAT, "BGZF inflate failed");
        if (verdict == DevSet::Inflate::crc_mismatch) return fail(FTK_ERR_FORMAT, "BGZF block CRC mismatch (device inflate)");
        const ftk::BamSummary& B = *S.h_bsum;
        if (B.carry_overflow || !B.consistent || B.n_runs > (uint32_t)ftk::kBamMaxRuns || B.n_rows > S.max_lines) {
            if (clk.on)
                fprintf(stderr, "[ftk stream bam] piece %zu: the device could not settle the record chain (carry overflow %u, "
                                "consistent %u, runs %u, rows %u of %zu, range %u bytes in %u stretches, %u serial repairs, first "
                                "unsettled stretch %u: start %u, predecessor landed %u started %u, before it landed %u%s): the host "
                                "decoder takes over\n",
                        n_pieces, B.carry_overflow, B.consistent, B.n_runs, B.n_rows, S.max_lines, B.m, B.n_stretch, B.n_repairs,
                        B.first_unsettled, B.dbg[0], B.dbg[1], B.dbg[2], B.dbg[3], pc.on_host ? ", host-inflated" : "");
            want_host_restart = true;  // the host decoder takes the file (contigs handed out so far are skipped)
            return false;
        }
        if (B.bad) return fail(FTK_ERR_FORMAT, "corrupt BAM record");
        if (pc.eof && B.landing != B.m && !partial_tail_ok) return fail(FTK_ERR_FORMAT, "truncated BAM record");
        std::vector<std::pair<uint32_t, int>> runs(B.n_runs);
        for (uint32_t r = 0; r < B.n_runs; ++r) runs[r] = {B.run_row[r], B.run_ref[r]};
        std::sort(runs.begin(), runs.end());
        for (size_t r = 0; r < runs.size(); ++r) {
            const size_t r0 = runs[r].first, r1 = r + 1 < runs.size() ? runs[r + 1].first : (size_t)B.n_rows;
            if (!take_run(runs[r].second, S, r0, r1)) return false;
        }
        ++n_pieces;
        n_rows_total += B.n_rows;
        n_records += B.n_records;
        skipped[0] += B.n_unrepresentable;
        skipped[1] += B.n_nocigar_reverse;
        last_key = std::max(last_key, (unsigned long long)B.last_key);
        S.freed_valid = hipEventRecord(S.freed, pstream) == hipSuccess;
        if (!S.freed_valid) {
            (void)hipGetLastError();
            return fail(FTK_ERR_HIP, "cannot record a buffer set's release");
        }
        clk.lap(2);
        return true;
    };

    for (;;) {
        // The backs go onto the parse stream in file order: curp's now (waiting for the host threads if they hold
        // it), the following ones as far as they are ready without waiting.  BEFORE any new front: the piece read
        // next goes into the slot of the piece settled last, whose text the parse of ITS successor (curp) still
        // reads the carry from - submit_back re-records that slot's `freed` behind curp's parse.
        if (!curp.back_done && !submit_back(curp)) return false;
        for (auto& pc : ahead) {
            if (pc.back_done) continue;
            if (pc.on_host && host_job[pc.slot].valid() &&
                host_job[pc.slot].wait_for(std::chrono::seconds(0)) != std::future_status::ready)
                break;
            if (!submit_back(pc)) return false;
        }
        // read and enqueue the next pieces before this one is settled
        if (!read_ahead_fronts()) return false;
        for (auto& pc : ahead) {  // (the fronts just enqueued: GPU pieces' backs follow at once)
            if (pc.back_done) continue;
            if (pc.on_host && host_job[pc.slot].valid() &&
                host_job[pc.slot].wait_for(std::chrono::seconds(0)) != std::future_status::ready)
                break;
            if (!submit_back(pc)) return false;
        }
        clk.lap(5);
        if (!settle(curp)) return false;
        if (curp.eof) {
            // (region reads) the read stopped at the linear index's hint: complete when the last record lies at or behind
            // the region's end or on a later reference; else a record longer than an index window hid the true end
            const bool soft = has_region && read_end >= 0 && read_end < hard_read_end && curp.file_off >= 0 &&
                              curp.file_off + (long long)curp.n >= read_end;
            if (!soft) break;
            const long long lref = (long long)(uint32_t)(last_key >> 32), lpos = (long long)(uint32_t)last_key;
            const bool complete = last_key != 0 && (lref != (long long)region_ref || lpos >= reg_stop);
            if (clk.on)
                fprintf(stderr, "[ftk stream bam] region %lld-%lld: piece ends at file offset %lld (hint %lld, contig ends %lld): %s\n",
                        reg_start, reg_stop, curp.file_off + (long long)curp.n, read_end, hard_read_end,
                        complete ? "complete" : "a long record hides the end, reading on");
            if (complete) break;
            read_end = std::min(hard_read_end, read_end + (long long)(size_t(8) << 20));
            curp.eof = false;
            if (!read_ahead_fronts()) return false;
        }
        if (ahead.empty()) return fail(FTK_ERR_HIP, "piece queue out of step");
        curp = std::move(ahead.front());
        ahead.pop_front();
        {
            std::lock_guard<std::mutex> lk(mu);
            if (stop) return false;
        }
    }
    if (!finish_contig()) return false;
    clk.lap(4);
    clk.report("bam, records parsed on the device (inflate = waiting for a piece, parse = appends, merge = sort)");
    if (clk.on)
        fprintf(stderr, "[ftk stream bam] %zu pieces, %zu records, %zu fragments parsed on the device (stretch %u bytes); of \"other\": "
                        "header piece %.1f ms, fronts enqueued %.1f ms, waiting for the host threads' inflate %.1f ms\n",
                n_pieces, n_records, n_rows_total, stretch_bytes, t_header, t_front, t_jobwait);
    return true;
}
