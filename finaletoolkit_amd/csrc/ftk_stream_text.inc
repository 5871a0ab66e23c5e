// Part of ftk_decode.cpp's translation unit (#included there, in this order: core, sets, text, bam, api) - text streams: `run_text` (host inflate + host row parser) and `run_text_device` (device inflate + the one-pass row parser of ftk_textparse.hip, the slot ring of buffer sets, device-resident contig tables).

bool ftk_fragstream::run_text(RawBuf& buf, size_t n) {
    StageClock clk(this);
    std::vector<Block> blocks;
    RawBuf text;                  // carry (incomplete last line) + this piece's inflated text
    size_t text_carry = 0;
    bool layout_known = false;
    Contig cur;
    bool have_cur = false;
    std::set<std::string> seen;
    bool eof = n < last_want;
    for (;;) {
        size_t used = 0, total = 0;
        if (!whole_blocks(buf.data(), n, eof, &blocks, &used, &total)) return fail(FTK_ERR_FORMAT, "corrupt BGZF block");
        if (!text.reserve(text_carry + total + 1)) return fail(FTK_ERR_OOM, "out of host memory");
        clk.lap(5);
        if (!blocks.empty() && inflate_block_list(buf.data(), blocks, n_threads, text.data() + text_carry) != FTK_OK)
            return fail(FTK_ERR_FORMAT, "BGZF inflate failed");
        clk.lap(1);
        const char* b = (const char*)text.data();
        const char* e = b + text_carry + total;
        if (first_skip) {  // after an index seek: the contig starts inside the first block
            b += std::min<size_t>(first_skip, (size_t)(e - b));
            first_skip = 0;
        }
        if (!layout_known) layout_known = sniff_bed6(b, e, true, &bed6);
        // complete lines only; the rest waits for the next piece
        const char* last = e;
        if (!eof) {
            while (last > b && last[-1] != '\n') --last;
        }
        std::vector<Run> runs;
        if (last > b) parse_text_parallel(b, last, bed6, has_only ? only.c_str() : nullptr, n_threads, &runs);
        clk.lap(2);
        for (auto& r : runs) {
            if (have_cur && r.name != cur.name) {
                clk.lap(3);
                if (!emit(std::move(cur))) return false;
                clk.lap(4);
                cur = Contig{};
                have_cur = false;
            }
            if (!have_cur) {
                if (!seen.insert(r.name).second)
                    return fail(FTK_ERR_UNSORTED, ("contig " + r.name + " appears in two separate runs: the file is not sorted").c_str());
                cur.name = r.name;
                have_cur = true;
            }
            cur.parts.push_back(std::move(r.c));
        }
        clk.lap(3);
        text_carry = (size_t)(e - last);
        if (text_carry) memmove(text.data(), last, text_carry);
        if (eof) break;
        const size_t raw_carry = n - used;
        if (raw_carry) memmove(buf.data(), buf.data() + used, raw_carry);
        clk.lap(5);
        n = fill(buf, raw_carry);
        clk.lap(0);
        eof = n - raw_carry < last_want;
        {
            std::lock_guard<std::mutex> lk(mu);
            if (stop) return false;
        }
    }
    clk.lap(5);
    if (have_cur && !emit(std::move(cur))) return false;
    clk.lap(4);
    clk.report("text");
    return true;
}

// run_text with the row parser on the GPU.  Per piece: inflate into page-locked text (host threads), one
// DMA, four kernels, 8 KB of summary back - all asynchronous on the parse stream, and while they run the
// host already inflates the next piece into the other buffer set.  When a piece's summary says "plain
// rows only" its columns are appended to the current contig device-to-device, split at the contig runs the
// kernel listed (the names are read from the host copy of the text); any other piece goes through the
// host's field-rule parser (parse_text_parallel) and its columns are uploaded - same rows either way.
bool ftk_fragstream::run_text_device(RawBuf& buf, size_t n) {
    StageClock clk(this);
    if (hipSetDevice(device) != hipSuccess || (!pstream && (pstream = stream_pool().take(device)) == nullptr)) {
        (void)hipGetLastError();
        return fail(FTK_ERR_HIP, "cannot create the parse stream");
    }
    // Four buffer sets in a ring, settled two pieces behind the one being launched: while the parse stream works on
    // piece k-1 (set-up, row parser, the appends of k-2), the FRONT of piece k - compressed bytes up, inflate and CRC
    // kernels, nothing that depends on another piece - runs on the set's own stream beside piece k-1's front.
    // With the host threads taking a share of the pieces (below) the ring is longer: a host piece's parse - and, the
    // parse stream being in file order, those of the pieces behind it - goes onto the stream when its inflate is done,
    // at the latest kHostLag pieces later.
    constexpr int kSets = 12, kHostLag = 8;
    DevSet sets[kSets];
    for (auto& S : sets) S = devset_pool().take(device);
    FrontStreams<kSets> fstream;
    fstream.device = device;
    fstream.fallback = pstream;
    fstream.prefill(std::min(pieces_expected(), kSets) - 1);
    // FTK_DECODE_TIMING: the device time of every piece's front (copy up + inflate + CRC) and back (set-up + rows)
    hipEvent_t tev[kSets][5] = {};  // front start, front end, back start, back end, bytes up
    double front_ms = 0, front_max = 0, back_ms = 0, back_max = 0;
    size_t n_timed = 0;
    const auto t_begin = std::chrono::steady_clock::now();
    auto now_ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); };
    std::string trail;  // FTK_DECODE_TIMING=2: one line per settled piece, and the producer's own steps
    const bool trail_on = clk.on && atoi(getenv("FTK_DECODE_TIMING")) >= 2;
    auto mark = [&](int piece, const char* what) {
        if (!trail_on) return;
        char line[120];
        snprintf(line, sizeof line, "  piece %d %s at %.2f ms\n", piece, what, now_ms());
        trail += line;
    };
    if (clk.on)
        for (auto& row : tev)
            for (auto& ev : row) (void)hipEventCreate(&ev);
    AtExit drop_tev{[&] {
        for (auto& row : tev)
            for (hipEvent_t ev : row)
                if (ev) (void)hipEventDestroy(ev);
    }};
    RingCleanup<kSets> cleanup{sets, device, pstream, &fstream};
    std::vector<Block> blocks;
    size_t carry = 0;
    const uint8_t* carry_src = nullptr;
    bool layout_known = false;
    Contig cur;
    bool have_cur = false;
    bool saw_other = false;
    std::set<std::string> seen;
    size_t gpu_pieces = 0, host_pieces = 0;
    // The BGZF blocks are inflated on the GPU too (ftk_inflate.hip): the host only reads the file and copies it into
    // page-locked memory.  FTK_DEVICE_INFLATE=0 keeps the inflate on the host threads (libdeflate / zlib).
    static const bool dev_inflate_env = !(getenv("FTK_DEVICE_INFLATE") && atoi(getenv("FTK_DEVICE_INFLATE")) == 0);
    const bool dev_inflate = dev_inflate_env && !host_inflate_only;
    // The host threads CAN inflate pieces beside the GPU (a host piece's text goes up in one DMA before its parse; they
    // take the next piece whenever their previous one is done, so the split follows the two rates).  That was worth 18 %
    // when the chip turned fragment rows over at ~30 GB/s (round 3) and 3-5 % at 87 GB/s (round 4); with round 5's
    // symbol loop (185 GB/s, DESIGN 3.5c) the pieces they take arrive LATER than the GPU would have had them:
    // whole-genome pass 0.089-0.109 s with, 0.078-0.089 s without (tools/env_ab.sh text).  Off by default since.
    // FTK_TEXT_HOST_SHARE=<n>: 0 none (the default), 1 as the threads are free, n > 1 every n-th piece.
    static const int host_share_env = [] {
        const char* e = getenv("FTK_TEXT_HOST_SHARE");
        return e ? atoi(e) : -1;
    }();
    const int host_share = !dev_inflate ? 0 : host_share_env >= 0 ? host_share_env : 0;
    static const int lag_env = [] {
        const char* e = getenv("FTK_TEXT_LAG");
        return e ? atoi(e) : -1;
    }();
    // (pieces the producer lets the GPU fall behind before it waits: FTK_TEXT_LAG; without host pieces 2 until round 5 -
    // 0.078-0.089 s per genome pass - now 4: 0.074-0.085 s; 6 and 9 the same)
    const int kLag = lag_env >= 1 ? std::min(lag_env, kHostLag + 1) : host_share > 0 ? kHostLag + 1 : 4;
    struct PieceMeta {
        bool on_host = false, eof = false, has_prev = false, back_done = true;
        size_t total = 0;
        uint32_t first_skip = 0;
    } meta[kSets];
    std::future<int> host_job[kSets];
    JobGuard job_guard{host_job, kSets};
    double t_jobwait = 0;
    size_t host_inflated = 0;
    RestGuard rest_guard{this};
    long long piece_off = first_piece_off;  // where buf's first byte lies in the file (-1: unknown)
    int settled = 0, backs = 0;  // pieces settled / pieces whose back is on the parse stream
    int last_host_set = -1;  // the set of the piece the host threads took last
    auto host_takes = [&](int k) -> bool {
        if (host_share <= 0 || k == 0) return false;
        if (host_share > 1) return (k % host_share) == host_share - 1;
        // (only with a backlog on the GPU: the first pieces of a stream - all of a small file - are back sooner from the
        // chip, 3 ms a piece against the threads' 12)
        if (k - settled < 3) return false;
        // (and only pieces of three of the twelve sets: a host piece needs 250 MB of page-locked text behind its set -
        // 25 ms to lock - and at the two rates the threads take about every fifth piece anyway)
        if ((k & 3) != 0) return false;
        return last_host_set < 0 || !host_job[last_host_set].valid() ||
               host_job[last_host_set].wait_for(std::chrono::seconds(0)) == std::future_status::ready;
    };

    // one contig run of a piece: n rows at the given column pointers (device or host)
    auto take_run = [&](const std::string& name, const int32_t* s0, const int32_t* e0, const uint8_t* q0, const uint8_t* t0,
                        size_t rows, hipMemcpyKind kind) -> bool {
        if (has_only && name != only) {
            saw_other = true;  // (rows behind the wanted contig's: a region read is complete)
            return true;
        }
        if (host_inflate_only && emitted_names.count(name)) return true;  // second pass: handed out by the first
        if (have_cur && name != cur.name) {
            if (!emit_device(std::move(cur), false)) return false;
            cur = Contig{};
            have_cur = false;
        }
        if (!have_cur) {
            if (!seen.insert(name).second)
                return fail(FTK_ERR_UNSORTED, ("contig " + name + " appears in two separate runs: the file is not sorted").c_str());
            cur.name = name;
            cur.dev.reset(new DevColumns());
            cur.dev->device = device;
            have_cur = true;
        }
        if (!cur.dev->append(s0, e0, q0, t0, rows, kind, pstream)) return fail(FTK_ERR_OOM, "out of device memory for the contig's columns");
        return true;
    };

    auto collect_rows = [&](DevSet& S) -> bool {
        if (!S.host_only && hipEventSynchronize(S.done) != hipSuccess) {
            (void)hipGetLastError();
            return fail(FTK_ERR_HIP, "the device row parser failed");
        }
        S.pending = false;
        const ftk::TextSummary& sum = *S.h_sum;
        if (S.inflated) {
            const DevSet::Inflate verdict = S.inflate_verdict();
            if (verdict == DevSet::Inflate::bad_block)
                return fail(FTK_ERR_FORMAT, ("BGZF inflate failed: a block did not decode to its ISIZE (device inflate, reason " +
                                             std::to_string(S.h_ist->reason) + ")").c_str());
            if (verdict == DevSet::Inflate::crc_mismatch) return fail(FTK_ERR_FORMAT, "BGZF block CRC mismatch (device inflate)");
            if (sum.carry_overflow) {  // a line too long for the device carry: the host-inflate pass takes the file
                want_host_restart = true;
                return false;
            }
            if (sum.text_len == 0) return true;
            const bool drop_last = S.cut_tail && sum.last_line_bad && sum.n_bad == 1;  // the row the read stopped in
            const size_t n_rows = (size_t)sum.n_lines - (drop_last ? 1 : 0);
            const bool plain_d = !sum.overflow && (sum.n_bad == 0 || drop_last) && sum.n_runs >= 1 &&
                                 sum.n_runs <= (unsigned)ftk::kTextNamedRuns && !sum.name_overflow && sum.n_lines <= S.max_lines;
            if (plain_d) {
                ++gpu_pieces;
                std::vector<std::pair<unsigned, unsigned>> runs(sum.n_runs);  // (first line, slot)
                for (unsigned r = 0; r < sum.n_runs; ++r) runs[r] = {sum.run_line[r], r};
                std::sort(runs.begin(), runs.end());
                for (size_t r = 0; r < runs.size(); ++r) {
                    const size_t l0 = runs[r].first, l1 = r + 1 < runs.size() ? runs[r + 1].first : n_rows;
                    if (!take_run(std::string((const char*)sum.run_name[runs[r].second]), S.d_s + l0, S.d_e + l0, S.d_q + l0,
                                  S.d_t + l0, l1 - l0, hipMemcpyDeviceToDevice))
                        return false;
                }
                return true;
            }
            // anything but plain rows: the host's field-rule parser reads the text (copied back for this piece only)
            ++host_pieces;
            if (!S.ensure_host_text(sum.text_len + 64)) return fail(FTK_ERR_OOM, "out of page-locked memory for a text piece");
            if (hipMemcpyAsync(S.h_text, S.d_text + sum.text_off, sum.text_len, hipMemcpyDeviceToHost, pstream) != hipSuccess ||
                hipStreamSynchronize(pstream) != hipSuccess) {
                (void)hipGetLastError();
                return fail(FTK_ERR_HIP, "cannot copy a text piece back");
            }
            std::vector<Run> runs;
            const char* tb = (const char*)S.h_text;
            parse_text_parallel(tb, tb + sum.text_len, bed6, has_only ? only.c_str() : nullptr, n_threads, &runs);
            for (auto& r : runs)
                if (!take_run(r.name, r.c.start.data(), r.c.end.data(), r.c.mapq.data(), r.c.strand.data(), r.c.start.size(),
                              hipMemcpyHostToDevice))
                    return false;
            return true;
        }
        const char* b = (const char*)S.h_text + S.off;
        const bool drop_last_h = S.cut_tail && sum.last_line_bad && sum.n_bad == 1;  // the row an index-driven read stopped in
        const bool plain = !S.host_only && !sum.overflow && (sum.n_bad == 0 || drop_last_h) && sum.n_runs >= 1 &&
                           sum.n_runs <= (unsigned)ftk::kTextMaxRuns && sum.n_lines <= S.max_lines;
        if (plain) {
            ++gpu_pieces;
            std::vector<std::pair<unsigned, unsigned>> runs(sum.n_runs);
            for (unsigned r = 0; r < sum.n_runs; ++r) runs[r] = {sum.run_line[r], sum.run_off[r]};
            std::sort(runs.begin(), runs.end());
            for (size_t r = 0; r < runs.size(); ++r) {
                const char* nb = b + runs[r].second;
                const char* tab = (const char*)memchr(nb, '\t', S.len - runs[r].second);
                if (!tab) return fail(FTK_ERR_FORMAT, "device row parser: run without a name");
                const size_t l0 = runs[r].first,
                             l1 = r + 1 < runs.size() ? runs[r + 1].first : (size_t)sum.n_lines - (drop_last_h ? 1 : 0);
                if (!take_run(std::string(nb, (size_t)(tab - nb)), S.d_s + l0, S.d_e + l0, S.d_q + l0, S.d_t + l0, l1 - l0,
                              hipMemcpyDeviceToDevice))
                    return false;
            }
        } else {
            ++host_pieces;
            std::vector<Run> runs;
            parse_text_parallel(b, b + S.len, bed6, has_only ? only.c_str() : nullptr, n_threads, &runs);
            for (auto& r : runs)
                if (!take_run(r.name, r.c.start.data(), r.c.end.data(), r.c.mapq.data(), r.c.strand.data(), r.c.start.size(),
                              hipMemcpyHostToDevice))
                    return false;
        }
        return true;
    };

    // settle a piece: its rows to the current contig (device to device, on the parse stream), and behind them the
    // event the set's next front waits for before it overwrites the buffers
    auto collect = [&](DevSet& S) -> bool {
        if (!collect_rows(S)) return false;
        if (clk.on && S.inflated) {
            const int j = (int)(&S - sets);
            float f = 0, bk = 0, gap = 0;
            if (hipEventElapsedTime(&f, tev[j][0], tev[j][1]) == hipSuccess && hipEventElapsedTime(&bk, tev[j][2], tev[j][3]) == hipSuccess) {
                float up = 0;
                (void)hipEventElapsedTime(&gap, tev[j][1], tev[j][2]);
                (void)hipEventElapsedTime(&up, tev[j][0], tev[j][4]);
                char line[200];
                snprintf(line, sizeof line, "  settled at %.1f ms: front %.2f (bytes up %.2f), front end -> back start %.2f, back %.2f ms\n", now_ms(), f, up, gap, bk);
                trail += line;
                front_ms += f; front_max = std::max(front_max, (double)f);
                back_ms += bk; back_max = std::max(back_max, (double)bk);
                ++n_timed;
            } else {
                (void)hipGetLastError();
            }
        }
        S.freed_valid = hipEventRecord(S.freed, pstream) == hipSuccess;
        if (!S.freed_valid) {
            (void)hipGetLastError();
            return fail(FTK_ERR_HIP, "cannot record a buffer set's release");
        }
        return true;
    };
    // Settle, in file order, every piece up to k whose results are already back, and wait for those that are kLag
    // or more behind (their sets come up for reuse).
    auto settle = [&](int k, bool all) -> bool {
        while (settled <= k && settled < backs) {
            DevSet& Q = sets[settled % kSets];
            if (Q.pending) {
                const bool must = all || settled <= k - kLag;
                if (!must) {  // ahead of need only while the consumer is blocked waiting for a contig
                    std::lock_guard<std::mutex> lk(mu);
                    if (!consumer_waiting) break;
                }
                if (!must && !Q.host_only && hipEventQuery(Q.done) != hipSuccess) {
                    (void)hipGetLastError();  // (not ready is no error)
                    break;
                }
                if (!collect(Q)) return false;
            }
            ++settled;
        }
        return true;
    };
    // The back of piece j (the parse stream, piece after piece): a host piece's text up first (on the set's own stream,
    // behind the appends that read the set last), then carry from the previous piece, line ends, rows.
    auto submit_back = [&](int j) -> bool {
        const int sj = j % kSets;
        DevSet& S = sets[sj];
        PieceMeta& M = meta[sj];
        DevSet* P = M.has_prev ? &sets[(j - 1) % kSets] : nullptr;
        bool ok = true;
        if (M.on_host) {
            hipStream_t front = fstream.get(sj);
            const auto t0 = std::chrono::steady_clock::now();
            const int jrc = host_job[sj].valid() ? host_job[sj].get() : (int)FTK_OK;
            t_jobwait += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (jrc != FTK_OK) return fail(FTK_ERR_FORMAT, "BGZF inflate failed or block CRC mismatch (host share of a device stream)");
            ok = upload_host_piece(front, S, ftk::kTextCarryMax, M.total, clk.on ? tev[sj] : nullptr);
        }
        ok = ok && hipMemsetAsync(S.d_sum, 0, sizeof(ftk::TextSummary), pstream) == hipSuccess &&
             hipStreamWaitEvent(pstream, S.front, 0) == hipSuccess && (!clk.on || hipEventRecord(tev[sj][2], pstream) == hipSuccess);
        if (ok) {
            ftk::textparse_launch_inflated(pstream, S.d_text, ftk::kTextCarryMax, (uint32_t)M.total, P ? P->d_text : nullptr,
                                           P ? P->d_sum : nullptr, M.first_skip, M.eof, bed6, S.d_blocks, S.max_lines,
                                           S.d_s, S.d_e, S.d_q, S.d_t, S.d_sum);
            ok = hipGetLastError() == hipSuccess &&
                 hipMemcpyAsync(S.h_sum, S.d_sum, sizeof(ftk::TextSummary), hipMemcpyDeviceToHost, pstream) == hipSuccess &&
                 hipMemcpyAsync(S.h_ist, S.d_ist, sizeof(ftk::InflateStatus), hipMemcpyDeviceToHost, pstream) == hipSuccess &&
                 (S.n_tab == 0 || hipMemcpyAsync(S.h_crc, S.d_crc, S.n_tab * 4, hipMemcpyDeviceToHost, pstream) == hipSuccess) &&
                 (!clk.on || hipEventRecord(tev[sj][3], pstream) == hipSuccess) && hipEventRecord(S.done, pstream) == hipSuccess;
        }
        if (ok && P) {
            // the previous piece's text has been read (the carry): its set may take a new piece behind THIS point,
            // wherever the piece itself was settled
            P->freed_valid = hipEventRecord(P->freed, pstream) == hipSuccess;
            ok = P->freed_valid;
        }
        if (!ok) {
            (void)hipGetLastError();
            return fail(FTK_ERR_HIP, "cannot launch the device row parser");
        }
        S.pending = true;
        M.back_done = true;
        return true;
    };
    // backs up to piece k, in file order; a host piece whose job is still running holds them up until it is kHostLag
    // pieces behind (or `all`)
    auto submit_backs = [&](int k, bool all) -> bool {
        while (backs <= k) {
            const int sj = backs % kSets;
            if (!all && meta[sj].on_host && backs > k - kHostLag && host_job[sj].valid() &&
                host_job[sj].wait_for(std::chrono::seconds(0)) != std::future_status::ready)
                break;
            if (!meta[sj].back_done && !submit_back(backs)) return false;
            ++backs;
        }
        return true;
    };
    bool eof = n < last_want;
    // (region reads) this short read stopped at the linear index's hint, not at the end of the contig's rows: the piece
    // is parsed as one with more behind it, and the rows then say whether to read on
    auto at_soft_end = [&](size_t n_now) {
        return eof && has_region && read_end >= 0 && read_end < hard_read_end && piece_off >= 0 &&
               piece_off + (long long)n_now >= read_end;
    };
    bool soft = at_soft_end(n);
    int k = 0;
    for (;; ++k) {
        size_t used = 0, total = 0;
        if (!whole_blocks(buf.data(), n, eof, &blocks, &used, &total)) return fail(FTK_ERR_FORMAT, "corrupt BGZF block");
        DevSet& S = sets[k % kSets];
        if (S.pending) return fail(FTK_ERR_HIP, "buffer ring out of step");
        if (dev_inflate && total + ftk::kTextCarryMax + 64 < (size_t(1) << 32)) {
            // ---- the piece is inflated ON THE DEVICE: compressed bytes up, one wave per BGZF block, then the carry /
            // line-end set-up and the row parser on the text where it lies; the host never sees the text
            if (!layout_known) {  // BED6 or not: the first data row, from the first blocks inflated here
                std::vector<uint8_t> head;
                size_t nb = 0, bytes = 0;
                while (nb < blocks.size() && bytes < (size_t(1) << 18)) bytes += blocks[nb++].out_len;
                head.resize(bytes + 1);
                std::vector<Block> first(blocks.begin(), blocks.begin() + nb);
                if (nb && inflate_block_list(buf.data(), first, n_threads, head.data()) != FTK_OK)
                    return fail(FTK_ERR_FORMAT, "BGZF inflate failed");
                // (a row the head ends in counts only at the end of the file: elsewhere the next piece decides)
                const char* hb = (const char*)head.data();
                layout_known = sniff_bed6(hb + std::min(first_skip, bytes), hb + bytes, eof, &bed6);
            }
            // h_text also stages the piece's COMPRESSED bytes on their way up: many tiny blocks (or small ISIZE
            // trailers) make `used` larger than the text, so the buffer is sized for whichever is larger
            const bool to_host = host_takes(k);
            // a GPU piece goes up straight from the read buffer when that is page-locked; the host threads work on their
            // own copy of theirs, which they read from the file (page cache) themselves when its offset is known
            hipEvent_t up_ev = (buf.pinned && !to_host) ? take_up_event() : nullptr;
            const bool direct = up_ev != nullptr;
            const bool job_reads = to_host && piece_off >= 0;
            if (!S.ensure(std::max(ftk::kTextCarryMax + total + 64, used + 64), false) || !S.ensure_inflate(used, blocks.size()) ||
                (to_host && (!S.ensure_host_comp(used + 64) || !S.ensure_host_text(ftk::kTextCarryMax + total + 64))) ||
                (!to_host && !direct && !S.ensure_host_text(used + 64)))
                return fail(FTK_ERR_OOM, "out of page-locked / device memory for the text piece");
            clk.lap(5);
            mark(k, to_host ? "(host) blocks listed, buffers ready" : "blocks listed, buffers ready");
            if (!direct && !job_reads) stage_bytes(to_host ? S.h_comp : S.h_text, buf.data(), used, n_threads);
            S.set_block_table(blocks, buf.data(), ftk::kTextCarryMax);
            S.cut_tail = eof && !soft && partial_tail_ok;
            S.inflated = true;
            S.host_only = false;
            mark(k, "staged");
            PieceMeta& M = meta[k % kSets];
            M = PieceMeta{};
            M.on_host = to_host;
            M.eof = eof && !soft;
            M.has_prev = k > 0 && sets[(k - 1) % kSets].inflated;
            M.back_done = false;
            M.total = total;
            M.first_skip = (uint32_t)std::min<size_t>(first_skip, total);
            hipStream_t front = fstream.get(k % kSets);  // (a host piece's too: its text goes up on it, see submit_back)
            bool ok = true;
            if (M.on_host) {
                // (the job owns its block list and works from its own copy of the bytes - the staging above - straight
                // into the set's page-locked text buffer; CRCs checked like the GPU's pieces)
                S.n_tab = 0;
                ++host_inflated;
                last_host_set = k % kSets;
                host_job[k % kSets] = start_host_inflate(blocks, S.h_comp, S.h_text + ftk::kTextCarryMax, n_threads, fileno(fp), used,
                                                         job_reads ? piece_off : -1);
            } else {
                // front (this set's stream): behind the appends that read the set last, bytes up, inflate, CRC
                ok = enqueue_front(front, S, direct ? buf.data() : S.h_text, used, blocks.size(), up_ev, false,
                                   clk.on ? tev[k % kSets] : nullptr);
                if (direct) buf_in_flight = up_ev;  // (fill() parks the buffer behind it; an unrecorded event reads as done)
            }
            if (!ok) {
                const hipError_t he = hipGetLastError();
                return fail(FTK_ERR_HIP, (std::string("cannot launch the device inflate (") + hipGetErrorName(he) + ", piece " +
                                          std::to_string(k) + ", " + std::to_string(blocks.size()) + " blocks, " +
                                          std::to_string(used) + " bytes)").c_str());
            }
            // the backs, in file order: every piece whose text is (about to be) on the device - a host piece when its
            // job is done, or kHostLag pieces later at the latest
            mark(k, "front enqueued");
            if (!submit_backs(k, false)) return false;
            first_skip = 0;
            clk.lap(1);
            mark(k, "backs enqueued");
            // this piece is on its way: settle what is back already, and the piece two back in any case (its set is
            // the one piece k+2 stages into)
            if (!settle(k, false)) return false;
            clk.lap(3);
            mark(k, "settle done");
            if (eof) {
                if (!soft) break;
                // the region's rows so far: complete when a row starts at or behind the region's end (or another
                // contig's rows came); else a row longer than an index window hid the true end - read on
                if (!submit_backs(k, true) || !settle(k, true)) return false;
                bool complete = saw_other;
                if (!complete && have_cur && cur.dev->rows) {
                    int32_t last = 0;
                    if (hipMemcpyAsync(&last, cur.dev->start + (cur.dev->rows - 1), 4, hipMemcpyDeviceToHost, pstream) != hipSuccess ||
                        hipStreamSynchronize(pstream) != hipSuccess) {
                        (void)hipGetLastError();
                        return fail(FTK_ERR_HIP, "cannot read the last row of a region");
                    }
                    complete = (long long)last >= reg_stop;
                }
                if (clk.on)
                    fprintf(stderr, "[ftk stream text] region %lld-%lld: piece %d ends at file offset %lld (hint %lld, contig ends %lld): %s\n",
                            reg_start, reg_stop, k, piece_off + (long long)n, read_end, hard_read_end,
                            complete ? "complete" : "a long row hides the end, reading on");
                if (complete) break;
                read_end = std::min(hard_read_end, read_end + (long long)(size_t(8) << 20));
            }
            const size_t raw_carry_d = n - used;
            if (piece_off >= 0) piece_off += (long long)used;
            // (with a copy of buf in flight the carried bytes are only read here: fill() moves them into the next buffer)
            if (raw_carry_d && !buf_in_flight) memmove(buf.data(), buf.data() + used, raw_carry_d);
            clk.lap(5);
            n = fill(buf, raw_carry_d, buf_in_flight ? used : 0);
            clk.lap(0);
            mark(k, "next piece read");
            eof = n - raw_carry_d < last_want;
            soft = at_soft_end(n);
            {
                std::lock_guard<std::mutex> lk(mu);
                if (stop) return false;
            }
            continue;
        }
        if (!submit_backs(k - 1, true)) return false;
        backs = k + 1;  // (this piece goes onto the parse stream right here)
        meta[k % kSets] = PieceMeta{};
        S.inflated = false;
        if (!S.ensure(carry + total + 2)) return fail(FTK_ERR_OOM, "out of page-locked / device memory for the text piece");
        if (carry) memcpy(S.h_text, carry_src, carry);
        clk.lap(5);
        if (!blocks.empty() && inflate_block_list(buf.data(), blocks, n_threads, S.h_text + carry, false, true) != FTK_OK)
            return fail(FTK_ERR_FORMAT, "BGZF inflate failed or block CRC mismatch");  // (CRCs checked like the GPU's pieces)
        clk.lap(1);
        char* b = (char*)S.h_text;
        char* e = b + carry + total;
        if (first_skip) {  // after an index seek: the contig starts inside the first block
            b += std::min<size_t>(first_skip, (size_t)(e - b));
            first_skip = 0;
        }
        if (!layout_known) layout_known = sniff_bed6(b, e, true, &bed6);
        char* last = e;
        if (!eof) {
            while (last > b && last[-1] != '\n') --last;
        } else if (e > b && e[-1] != '\n') {
            *e++ = '\n';  // the last row of the file has no line end: give it one (the buffer has the room)
            last = e;
        }
        if (last > b) {
            S.cut_tail = eof && partial_tail_ok;
            S.off = (size_t)(b - (char*)S.h_text);
            S.len = (size_t)(last - b);
            S.host_only = S.len >= (size_t(1) << 32) - 4096;
            bool ok = S.host_only || (hipMemsetAsync(S.d_sum, 0, sizeof(ftk::TextSummary), pstream) == hipSuccess &&
                                      hipMemcpyAsync(S.d_text, b, S.len, hipMemcpyHostToDevice, pstream) == hipSuccess);
            if (ok && !S.host_only) {
                ftk::textparse_launch(pstream, S.d_text, S.len, bed6, S.d_blocks, S.max_lines, S.d_s, S.d_e, S.d_q,
                                      S.d_t, S.d_sum);
                ok = hipGetLastError() == hipSuccess &&
                     hipMemcpyAsync(S.h_sum, S.d_sum, sizeof(ftk::TextSummary), hipMemcpyDeviceToHost, pstream) == hipSuccess &&
                     hipEventRecord(S.done, pstream) == hipSuccess;
            }
            if (!ok) {
                (void)hipGetLastError();
                return fail(FTK_ERR_HIP, "cannot launch the device row parser");
            }
            S.pending = true;
        }
        clk.lap(2);
        carry = (size_t)(e - last);
        carry_src = (const uint8_t*)last;
        if (!settle(k, false)) return false;
        clk.lap(3);
        if (eof) break;
        const size_t raw_carry = n - used;
        if (raw_carry) memmove(buf.data(), buf.data() + used, raw_carry);
        clk.lap(5);
        n = fill(buf, raw_carry);
        clk.lap(0);
        eof = n - raw_carry < last_want;
        {
            std::lock_guard<std::mutex> lk(mu);
            if (stop) return false;
        }
    }
    if (!submit_backs(k, true) || !settle(k, true)) return false;  // the pieces still in flight, in file order
    clk.lap(3);
    if (have_cur && !emit_device(std::move(cur), false)) return false;
    clk.lap(4);
    clk.report("text, device rows (parse = launch, merge = collect)");
    if (clk.on)
        fprintf(stderr, "[ftk stream text] %zu pieces parsed on the device, %zu by the host; %zu inflated by the host threads beside the GPU "
                        "(waited %.1f ms for them)\n", gpu_pieces, host_pieces, host_inflated, t_jobwait);
    if (clk.on && n_timed)
        fprintf(stderr, "[ftk stream text] device time per piece: front (copy up, inflate, CRC) avg %.2f max %.2f ms, back (set-up, rows) avg %.2f max %.2f ms, %zu pieces\n",
                front_ms / n_timed, front_max, back_ms / n_timed, back_max, n_timed);
    if (clk.on && atoi(getenv("FTK_DECODE_TIMING")) >= 2) fputs(trail.c_str(), stderr);
    return true;
}
