/*
 * ftk.h -- C ABI of the MI355X fragment-feature engine (libftk_hip.so).
 *
 * This is the drop-in boundary for FinaleToolkit's per-window hot path.  The
 * reference (epifluidlab/FinaleToolkit 1.1.0) is pure Python and has no FFI of
 * its own; every entry point below names the reference loop it replaces
 * (paths relative to the reference checkout, `src/finaletoolkit/...`).
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no C++/torch types.
 *  - Every call returns an int: FTK_OK (0) or a negative FTK_ERR_* code.
 *    ftk_last_error(ctx) returns a message owned by the library, valid until
 *    the next call on that ctx (ctx may be NULL for context-less calls).
 *  - One ftk_ctx per GPU.  A ctx is single-threaded (caller serialises);
 *    different ctxs may be driven from different threads.
 *  - Coordinates are 0-based half-open int32 (same as the reference's
 *    Fragment record, io/alignment.py:25-54).  Fragments of one contig are
 *    held as a start-sorted SoA (start i32, end i32, mapq u8, strand u8) in
 *    HBM: 10 bytes per fragment.
 *  - "in" pointers for windows/intervals and "out" pointers for results may be
 *    host OR device pointers; the library detects which and copies only when
 *    it has to.  Results are complete when the call returns for host
 *    pointers; for device pointers they are ordered on the ctx stream
 *    (ftk_ctx_sync / ftk_timer_stop to wait).
 *  - There is NO CPU fallback inside this library: without a usable gfx950
 *    device ftk_ctx_create fails with FTK_ERR_NO_DEVICE.
 */
#ifndef FTK_H
#define FTK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FTK_OK 0
#define FTK_ERR_INVALID (-1)   /* bad argument / out-of-domain input       */
#define FTK_ERR_NO_DEVICE (-2) /* no usable HIP device                      */
#define FTK_ERR_HIP (-3)       /* a HIP runtime call failed                 */
#define FTK_ERR_OOM (-4)       /* host or device allocation failed          */
#define FTK_ERR_IO (-5)        /* file could not be opened / read           */
#define FTK_ERR_FORMAT (-6)    /* file is not BGZF/gzip fragment text or BAM */
#define FTK_ERR_NO_CONTIG (-7) /* contig id / name not loaded               */
#define FTK_ERR_UNSORTED (-8)  /* fragments not sorted by start             */

/* Open window bounds (the reference's `start=None` / `stop=None`,
 * utils/_frag_generator.py:35-50). */
#define FTK_OPEN_LO INT32_MIN
#define FTK_OPEN_HI INT32_MAX
/* Open length bound (`min_length=None` / `max_length=None`,
 * utils/_comparison.py:13-24). */
#define FTK_LEN_OPEN (-1)

#define FTK_POLICY_MIDPOINT 0 /* utils/_frag_generator.py:35-42 */
#define FTK_POLICY_ANY 1      /* utils/_frag_generator.py:44-50 */
#define FTK_POLICY_FETCH 2    /* no intersect test: whatever the index query returns (AlignmentWrapper.fetch,
                               * io/alignment.py:216-240); taken by ftk_frag_select / ftk_frag_lengths only */

#define FTK_FETCH_TABIX 0     /* io/alignment.py:270-302: rows overlapping the window */
#define FTK_FETCH_BAM_READ1 1 /* io/alignment.py:242-268: read1 alignments overlapping the window */

#define FTK_MAX_TELOMERES 8

typedef struct ftk_ctx ftk_ctx;
typedef struct ftk_fragtable ftk_fragtable;

/* The shared per-fragment predicate of utils/_frag_generator.py:117-130 plus
 * the mapq cut of io/alignment.py:291 / :60-71. */
typedef struct ftk_filter {
    int32_t mapq_min;   /* keep mapq >= mapq_min                               */
    int32_t min_len;    /* keep len >= min_len; FTK_LEN_OPEN = no bound        */
    int32_t max_len;    /* keep len <= max_len; FTK_LEN_OPEN = no bound        */
    int32_t policy;     /* FTK_POLICY_*                                        */
    int32_t fetch_mode; /* FTK_FETCH_*                                         */
} ftk_filter;

/* Per-contig centromere/telomere constants of genome/gaps.py:202-267
 * (ContigGaps).  has_gaps == 0 means `contig_gaps is None`
 * (frag/_delfi.py:416-428,464). */
typedef struct ftk_gaps {
    int32_t has_gaps;
    int32_t cen_start, cen_stop;
    int32_t n_telo;
    int32_t telo_start[FTK_MAX_TELOMERES];
    int32_t telo_stop[FTK_MAX_TELOMERES];
} ftk_gaps;

/* ---- library / device ---------------------------------------------------- */
const char* ftk_version(void);
int ftk_device_count(int* n_out);
int ftk_ctx_create(int device_id, ftk_ctx** out);
void ftk_ctx_destroy(ftk_ctx* ctx);
const char* ftk_last_error(ftk_ctx* ctx);
/* Launch on a caller-provided hipStream_t (e.g. torch's current stream);
 * NULL restores the ctx's own stream. */
int ftk_ctx_set_stream(ftk_ctx* ctx, void* hip_stream);
int ftk_ctx_sync(ftk_ctx* ctx);

/* ---- diagnostics ----
 * Every call carves its temporaries, and the device stand-ins of host outputs, out of one scratch block per ctx that is
 * never cleared between calls; a call may assume nothing about what the block holds.  ftk_ctx_scratch_fill makes that
 * testable: byte in [0, 255] enqueues one memset of the whole block as it stands on the ctx stream, byte == -1 fills
 * nothing; either way *bytes_out (if not NULL) receives the block's size.  Any other byte: FTK_ERR_INVALID.  Nothing is
 * allocated, the block never moves, and no other memory of the ctx (contigs, reference images, weights, the asynchronous
 * result buffers) is touched. */
int ftk_ctx_scratch_fill(ftk_ctx* ctx, int byte, int64_t* bytes_out);
/* HIP-event stopwatch on the ctx stream (used by bench.py for per-kernel
 * durations).  ftk_timer_stop waits for the stop event. */
int ftk_timer_start(ftk_ctx* ctx);
int ftk_timer_stop(ftk_ctx* ctx, float* ms_out);
/* Event slots for timing individual launches without draining the stream:
 * record any number of slots inside a timed region, read the differences
 * afterwards (ftk_event_elapsed_ms waits for slot_b). */
#define FTK_MAX_EVENTS 4096
int ftk_event_record(ftk_ctx* ctx, int slot);
int ftk_event_elapsed_ms(ftk_ctx* ctx, int slot_a, int slot_b, float* ms_out);

/* ---- fragments: SoA residency in HBM -------------------------------------
 * Replaces the per-window `AlignmentWrapper.fetch` re-open + Fragment tuple
 * stream (io/alignment.py:217-302, utils/_frag_generator.py:112-116): one
 * contig is decoded once and stays resident. */
int ftk_frags_from_host(ftk_ctx* ctx, int contig_id, const int32_t* start, const int32_t* end,
                        const uint8_t* mapq, const uint8_t* strand, int64_t n);
/* Same, sources already in device memory (copied device-to-device into the
 * library's padded SoA). */
int ftk_frags_from_device(ftk_ctx* ctx, int contig_id, const int32_t* d_start, const int32_t* d_end,
                          const uint8_t* d_mapq, const uint8_t* d_strand, int64_t n);
/* BAM only: read1 alignment span per fragment, needed for FTK_FETCH_BAM_READ1
 * (io/alignment.py:245: pysam fetch returns read1 alignments overlapping the
 * window).  Arrays are parallel to the fragment arrays. */
int ftk_frags_set_read1(ftk_ctx* ctx, int contig_id, const int32_t* r1_start, const int32_t* r1_end, int64_t n);
/* BAM only, optional: file-order rank per fragment (ftk_fragtable_order).  With it ftk_frag_lengths /
 * ftk_frag_select return their rows in file order (pysam's iteration order) instead of start order. */
int ftk_frags_set_order(ftk_ctx* ctx, int contig_id, const int32_t* order, int64_t n);
int ftk_frags_info(ftk_ctx* ctx, int contig_id, int64_t* n_out, int32_t* max_len_out, int32_t* max_end_out);
/* Read-only query of the contig's packed (length, mapq) column: *present_out = 1 when the contig holds it (every
 * fragment is at most *len_max_out long and the contig has no read1 columns), *launches_out = calls of this process that
 * read it instead of the end and mapq columns so far (FTK_PACKED=0 keeps that at zero).  Any pointer may be NULL. */
int ftk_frags_packed(ftk_ctx* ctx, int contig_id, int32_t* present_out, int32_t* len_max_out, int64_t* launches_out);
int ftk_frags_release(ftk_ctx* ctx, int contig_id);

/* ---- fragment-file decoder (host only; no ctx / GPU needed) ---------------
 * io/alignment.py:270-302 (_fetch_tabix): BGZF/gzip text rows -> fragments.
 * Column layout: FinaleDB `chrom start stop mapq strand`; BED6 when the first
 * data row has > 5 columns (io/alignment.py:143-156) -> mapq = col 4, strand =
 * col 5.  Rows that do not parse are skipped (io/alignment.py:301-302).  No
 * mapq filtering here: mapq is a column, the cut is applied by the kernels.
 * io/alignment.py:242-268 (_fetch_sam): BAM records -> fragments (flag filter,
 * read1 only, TLEN reconstruction: TLEN > 0 -> [pos, pos + TLEN), CIGAR or not; TLEN < 0 ->
 * [end + TLEN, end) with end = htslib's bam_endpos = pos + max(reference length of the CIGAR, 1));
 * the read1 span kept for region queries is [pos, bam_endpos); rows sorted by fragment start. */
int ftk_fragfile_decode(const char* path, const char* contig /* NULL = all */, int n_threads, ftk_fragtable** out);
int ftk_bam_decode(const char* path, const char* contig /* NULL = all */, int n_threads, ftk_fragtable** out);
/* The same decoders as a stream: a producer thread decodes the file piece by piece (BGZF blocks in
 * parallel on n_threads) and hands over every finished contig as a one-contig table in page-locked
 * memory, at most max_queued contigs ahead of the caller -- so the caller uploads and computes on
 * contig k while contig k+1 is being decoded, and host memory stays bounded for any file size.
 * ftk_fragstream_next returns FTK_OK with *out == NULL at the end of the file; tables are freed with
 * ftk_fragtable_free.  Input must keep each contig's rows together (coordinate-sorted), else
 * FTK_ERR_UNSORTED.  BAM: ftk_fragstream_n_refs / _ref_name / _ref_length give the header's @SQ list
 * (they wait for the header). */
/* Contigs of a tabix-indexed fragment file according to its .tbi (those holding rows, newline-separated,
 * NUL-terminated; *needed_out = bytes required) and the layout of its first data row -- enough to open a
 * file lazily and decode single contigs on demand (a single-contig ftk_fragstream_open seeks through the
 * index).  FTK_ERR_FORMAT when there is no usable index (callers then decode the file in one pass). */
int ftk_fragfile_index_contigs(const char* path, char* names_out, int64_t cap, int64_t* needed_out, int* is_bed6_out);
typedef struct ftk_fragstream ftk_fragstream;
/* ftk_fragstream_open_device: the same stream with the ROW PARSER ON THE GPU for text files (BAM records stay
 * on the host): the host threads only inflate, each piece of text goes to device `device_id` in one DMA, four
 * small kernels find the lines and parse the plain rows, and the tables handed out hold DEVICE columns
 * (ftk_fragtable_is_device; ftk_fragtable_columns then returns device pointers, ftk_fragtable_columns_to_host
 * copies them out).  A piece that holds anything but plain rows (comments, signs, blanks, short lines ...) is
 * parsed by the host's field-rule parser, so the rows are the same as ftk_fragstream_open's.  ftk_frags_from_table
 * takes both kinds.  FTK_DEVICE_PARSE=0 makes it behave like ftk_fragstream_open. */
int ftk_fragstream_open_device(int device_id, const char* path, const char* contig /* NULL = all */, int is_bam,
                               int n_threads, int max_queued, ftk_fragstream** out);

/* A stream over the rows of ONE REGION of a contig (the reference's per-window `fetch(contig, start, stop)`,
 * io/alignment.py:205-268, at the granularity a rank of a multi-GPU run needs: frag/_delfi.py's ranks each take a
 * window-aligned share of the genome).  The single table it hands out holds EVERY row of `contig` that overlaps
 * [start, stop) - for a BAM: every fragment whose read1 record overlaps it - and may hold more (rows before the region
 * from the first block read; the whole contig for files whose index has no linear index, streams without a device or
 * with FTK_DEVICE_INFLATE=0 / FTK_DEVICE_BAM_PARSE=0).  With a tabix index (a BAI for BAM input) the
 * read starts at the linear index's offset for `start` and ends where the parsed rows say the region is complete: a
 * row that starts at or behind `stop`, or another contig's rows, were seen (the index's 16 kb windows give a first
 * guess; a row longer than a window makes the read go on in 8 MB steps).  Arguments otherwise as
 * ftk_fragstream_open_device. */
int ftk_fragstream_open_region(int device_id, const char* path, const char* contig, int64_t start, int64_t stop, int is_bam,
                               int n_threads, int max_queued, ftk_fragstream** out);
int ftk_fragtable_is_device(const ftk_fragtable* t, int i);
/* hipEvent_t recorded behind the last write to a device table's columns (NULL for host tables) */
void* ftk_fragtable_ready_event(const ftk_fragtable* t, int i);
int ftk_fragtable_columns_to_host(const ftk_fragtable* t, int i, int32_t* start, int32_t* end, uint8_t* mapq,
                                  uint8_t* strand);
/* The read1 span and the file-order rank of a BAM table's rows into host arrays (any may be NULL), wherever the
 * table's columns live (BAM records parsed on the device hand out device columns: ftk_fragtable_is_device). */
int ftk_fragtable_read1_to_host(const ftk_fragtable* t, int i, int32_t* r1_start, int32_t* r1_end, int32_t* order);
int ftk_fragstream_open(const char* path, const char* contig /* NULL = all */, int is_bam, int n_threads,
                        int max_queued, ftk_fragstream** out);
int ftk_fragstream_next(ftk_fragstream* s, ftk_fragtable** out);
int ftk_fragstream_n_refs(ftk_fragstream* s);
const char* ftk_fragstream_ref_name(ftk_fragstream* s, int i);
int64_t ftk_fragstream_ref_length(ftk_fragstream* s, int i);
/* Wall time (ms) the stream's producer thread spent per stage, complete once ftk_fragstream_next has returned the
 * end of the file: out[0..5] = file read, BGZF inflate, row / record parse (device parser: launch), run merge /
 * collect, hand-over (pack + waiting for queue space), everything else.  The stages of one piece run one after
 * the other on the producer; their work is spread over n_threads (and the GPU for the device row parser). */
int ftk_fragstream_stage_ms(ftk_fragstream* s, double out[6]);
/* BAM records met so far (cumulative; read it after every ftk_fragstream_next, the final one included) that the
 * reference does NOT simply skip and this library cannot turn into a row (csrc/ftk_bamrule.h):
 *   out[0]  read1 records whose fragment the columns cannot hold - a NEGATIVE start (reference_end + TLEN < 0,
 *           io/alignment.py:257), or a fragment or read1 alignment that ends at or beyond 2^30 (the largest end a
 *           contig's columns hold: ftk_frags_from_host refuses a contig beyond it).  The reference yields such a fragment; here it is dropped and
 *           counted (the Python surface issues a UserWarning) and the rest of its contig loads.
 *   out[1]  read1 records WITHOUT a CIGAR and TLEN < 0.  pysam's reference_end is None for them and the reference
 *           raises TypeError at io/alignment.py:257; here they are dropped and counted (the Python surface raises
 *           TypeError).  A CIGAR-less read1 with TLEN > 0 is a fragment, as in the reference (:253-255).
 * ftk_fragtable_skipped: the same two numbers for a table of the whole-file decoder ftk_bam_decode. */
int ftk_fragstream_skipped(ftk_fragstream* s, int64_t out[2]);
int ftk_fragtable_skipped(const ftk_fragtable* t, int64_t out[2]);
void ftk_fragstream_close(ftk_fragstream* s);
const char* ftk_fragtable_error(void); /* message for a failed decode call (thread-local) */
int ftk_fragtable_is_bed6(const ftk_fragtable* t);
int ftk_fragtable_n_contigs(const ftk_fragtable* t);
const char* ftk_fragtable_contig_name(const ftk_fragtable* t, int i);
int64_t ftk_fragtable_contig_length(const ftk_fragtable* t, int i); /* BAM @SQ LN, -1 for text */
int64_t ftk_fragtable_contig_rows(const ftk_fragtable* t, int i);
int ftk_fragtable_columns(const ftk_fragtable* t, int i, const int32_t** start, const int32_t** end,
                          const uint8_t** mapq, const uint8_t** strand,
                          const int32_t** r1_start /* NULL for text */, const int32_t** r1_end);
/* 1 when contig i's columns sit in page-locked host memory (a HIP device was present at decode time). */
/* BAM tables: rank of each fragment's read1 record in the file (pysam iterates in that order, the
 * columns are sorted by fragment start); NULL for text tables, whose rows already are in file order. */
int ftk_fragtable_order(const ftk_fragtable* t, int i, const int32_t** order);
int ftk_fragtable_is_pinned(const ftk_fragtable* t, int i);
void ftk_fragtable_free(ftk_fragtable* t);

/* Page-locked host memory for large result arrays (the per-base scores of frag/_wps.py:181-188 are
 * 8 bytes a base): a device -> host copy into it is one DMA at PCIe speed, into pageable memory a staged
 * copy at a third to half of that.  Blocks are recycled by ftk_host_free (a fresh one is a 2 MB-page mapping touched by
 * a few threads and registered with the driver: ~0.01 ms per MB; hipHostMalloc, the fall-back, ~0.2 ms per MB).
 * FTK_ERR_NO_DEVICE without a HIP device; FTK_ERR_OOM when the driver refuses or more than 8 GB
 * (FTK_PINNED_RESULT_LIMIT_MB) would be outstanding - the caller then uses ordinary memory. */
int ftk_host_alloc(int64_t bytes, void** out);
/* The same recycling for a result the DEVICE never writes: ordinary (pageable) memory, 2 MB-aligned.  ftk_wps with a
 * host output of 4 M positions or more sends the scores across the link as int16 and the host threads widen them into
 * the output (see ftk_wps) - page-locking such an output buys nothing and took 0.2 ms per MB when this entry point was added (0.4 s for a chr1 of scores, paid
 * by the first call of a process = by every command-line call); the widening threads fault this one in in parallel.
 * Works without a device.  Freed with ftk_host_free like the page-locked blocks. */
int ftk_host_alloc_pageable(int64_t bytes, void** out);
void ftk_host_free(void* p);
/* Give back everything the library keeps for reuse between calls - idle page-locked blocks (decoded tables, result
 * arrays from ftk_host_alloc), idle device blocks of contigs parsed on the GPU, the streaming decoders' idle buffer
 * sets (up to four per process, ~1 GB of page-locked and ~2 GB of device memory after a large text stream).  Blocks
 * in use are not touched.  Returns the bytes released (a lower bound).  For long-lived processes between jobs; the
 * next call that needs a block allocates it again (~0.01 ms per MB for the page-locked ones). */
int64_t ftk_cache_trim(void);
/* Upload contig i of a decoded table (including the BAM read1 columns) as contig_id: the
 * decode -> pinned SoA -> hipMemcpyAsync leg of the pipeline, without a detour through the caller. */
int ftk_frags_from_table(ftk_ctx* ctx, int contig_id, const ftk_fragtable* t, int i);

/* File -> HBM in one call, for hosts that do not want to handle tables: the streaming decoder feeds
 * every contig of the file (or only `contig`) to ftk_frags_from_table as it is decoded; contig ids are
 * first_contig_id, first_contig_id + 1, ... in file order (BAM: contigs that have usable reads, in
 * header order), *n_loaded_out of them; ftk_frags_name gives the contig name behind an id loaded this
 * way.  (io/alignment.py:160-203 opens the same two kinds of input.) */
int ftk_frags_load_fraggz(ftk_ctx* ctx, const char* path, const char* contig /* NULL = all */, int n_threads,
                          int first_contig_id, int* n_loaded_out);
int ftk_frags_load_bam(ftk_ctx* ctx, const char* path, const char* contig /* NULL = all */, int n_threads,
                       int first_contig_id, int* n_loaded_out);
const char* ftk_frags_name(ftk_ctx* ctx, int contig_id);

/* ---- a5: coverage --------------------------------------------------------
 * frag/_coverage.py:117-130 (`for _ in frags: coverage += 1`) over
 * utils/_frag_generator.py:117-130, for n_win windows of one contig at once.
 * Windows may overlap and come in any order.  count_out[i] = number of
 * fragments passing `f` for window i. */
int ftk_window_counts(ftk_ctx* ctx, int contig_id, const int32_t* w_start, const int32_t* w_end, int64_t n_win,
                      const ftk_filter* f, int64_t* count_out);

/* ---- a10/a11: DELFI short/long counts ------------------------------------
 * frag/_delfi.py:443-472 per window: mapq >= mapq_min, 100 <= len <= 220,
 * midpoint in [w_start, w_end), not inside a blacklist region that lies fully
 * inside the window (frag/_delfi.py:110-126,455-462), not
 * ContigGaps.in_tcmere (genome/gaps.py:217-237; note the all() over
 * telomeres); len >= 151 -> long, else short; nfrag = short + long.
 * bl_start/bl_end: the contig's blacklist, sorted by (start, stop)
 * (frag/_delfi.py:85-107); may be NULL when n_bl == 0.  The window-level
 * NOARM gate (frag/_delfi.py:423-428) is the caller's.  Windows and blacklist
 * are HOST arrays; their device form (windows + per-window blacklist CSR) is
 * cached in the ctx by content, so repeated calls with the same bins upload
 * nothing.  Outputs may be host or device pointers; nfrag_out may be NULL. */
int ftk_delfi_counts(ftk_ctx* ctx, int contig_id, const int32_t* w_start, const int32_t* w_end, int64_t n_win,
                     int32_t mapq_min, const int32_t* bl_start, const int32_t* bl_end, int64_t n_bl,
                     const ftk_gaps* gaps, int64_t* short_out, int64_t* long_out, int64_t* nfrag_out);

/* ---- a9: fragment-length histogram per window -----------------------------
 * frag/_frag_length.py:147-153 (_distribution_from_gen) for n_win windows:
 * hist_out[i * n_bins + (len - len_lo)] counts fragments of window i passing
 * `f`; lengths outside [len_lo, len_lo + n_bins) are tallied in
 * overflow_out[i].  The statistics of frag/_frag_length.py:175-238 are host
 * arithmetic on these histograms. */
int ftk_fraglen_hist(ftk_ctx* ctx, int contig_id, const int32_t* w_start, const int32_t* w_end, int64_t n_win,
                     const ftk_filter* f, int32_t len_lo, int32_t n_bins, uint32_t* hist_out, int64_t* overflow_out);
/* a9, the statistics themselves (frag/_frag_length.py:156-172 `_find_median`, :202-224 `_frag_length_stats`): the same
 * pass as ftk_fraglen_hist over lengths [len_lo, len_lo + n_bins), then per window - on the device, from the histogram
 * rows, which never leave it - stats_out[w][7] = mean, median, stdev (population), min, max, count, #(len <= short_cut)
 * as float64 (the integers are exact).  count 0: the window holds no passing fragment (the other six are 0; the
 * reference reports -1 for all).  The length range must hold every length the filter passes (the caller takes
 * [max(min_len, 0), min(max_len, longest fragment of the contig)]); n_bins as in ftk_fraglen_hist.  stats_out may be
 * host or device memory. */
int ftk_fraglen_stats(ftk_ctx* ctx, int contig_id, const int32_t* w_start, const int32_t* w_end, int64_t n_win,
                      const ftk_filter* f, int32_t len_lo, int32_t n_bins, int32_t short_cut, double* stats_out);

/* ---- fused pass: any combination of the three window features in ONE sweep over
 * the contig's fragments (one plan, one launch pair instead of three): coverage
 * (count_out) and length histogram (hist_out/overflow_out) under `f`, DELFI
 * short/long under the rules of ftk_delfi_counts.  A NULL output switches its
 * feature off; windows and blacklist must be host arrays when DELFI is on. */
int ftk_window_features(ftk_ctx* ctx, int contig_id, const int32_t* w_start, const int32_t* w_end, int64_t n_win,
                        const ftk_filter* f, int64_t* count_out, int32_t len_lo, int32_t n_bins, uint32_t* hist_out,
                        int64_t* overflow_out, int32_t delfi_mapq_min, const int32_t* bl_start, const int32_t* bl_end,
                        int64_t n_bl, const ftk_gaps* gaps, int64_t* short_out, int64_t* long_out);

/* The same pass for the windows of SEVERAL contigs in ONE launch (a genome-wide bin set: the
 * reference's delfi() / coverage() loop over contigs, frag/_delfi.py:289-300, frag/_coverage.py:244-248).
 * Item i holds contig items[i].contig_id's windows (host arrays; blacklist / gaps only matter for the
 * DELFI outputs).  Outputs are concatenated in item order: row = sum of n_win of the items before + w.
 * One block per window: meant for bin tilings (many windows of similar length). */
typedef struct ftk_feature_item {
    int32_t contig_id;
    int64_t n_win;
    const int32_t* w_start;
    const int32_t* w_end;
    const int32_t* bl_start; /* sorted by start; NULL = no blacklist */
    const int32_t* bl_end;
    int64_t n_bl;
    const ftk_gaps* gaps;    /* NULL = no gap annotation */
} ftk_feature_item;
int ftk_window_features_batch(ftk_ctx* ctx, const ftk_feature_item* items, int32_t n_items, const ftk_filter* f,
                              int64_t* count_out, int32_t len_lo, int32_t n_bins, uint32_t* hist_out,
                              int64_t* overflow_out, int32_t delfi_mapq_min, int64_t* short_out, int64_t* long_out);

/* frag/_frag_length.py:290-305 (frag_length): lengths of the fragments of ONE
 * window passing `f`, in file order.  Writes at most cap values to len_out
 * and always the true count to n_out. */
int ftk_frag_lengths(ftk_ctx* ctx, int contig_id, int32_t w_start, int32_t w_end, const ftk_filter* f,
                     int32_t* len_out, int64_t cap, int64_t* n_out);

/* utils/utils.py:186-255 (frag_array) / utils/_frag_generator.py:58-141: the
 * passing fragments of ONE window in file order (any column pointer may be
 * NULL). */
int ftk_frag_select(ftk_ctx* ctx, int contig_id, int32_t w_start, int32_t w_end, const ftk_filter* f,
                    int32_t* start_out, int32_t* end_out, uint8_t* mapq_out, uint8_t* strand_out, int64_t cap,
                    int64_t* n_out);

/* ---- a7/a8: Windowed Protection Score --------------------------------------
 * frag/_wps.py:25-53,156-188 for every base c in [start, stop):
 *   ws = rint(c - W/2), we = rint(c + W/2 - 1)   (numpy rint: half to even)
 *   WPS(c) = #{fs < ws and fe > we} - #{ws <= fs <= we or ws <= fe <= we}
 * over the fragments with mapq >= mapq_min, min_len <= len <= max_len whose
 * midpoint lies in [max(start - max_len, 0), min(stop + max_len, chrom_size))
 * (frag/_wps.py:156-169).  wps_out has stop - start entries. */
int ftk_wps(ftk_ctx* ctx, int contig_id, int64_t start, int64_t stop, int64_t chrom_size, int32_t window_size,
            int32_t min_len, int32_t max_len, int32_t mapq_min, int64_t* wps_out);
/* frag/_multi_wps.py:196-198: the same for n_iv intervals of one contig in
 * one launch; interval i writes iv_stop[i] - iv_start[i] values at
 * wps_out + out_offset[i].  iv_* / out_offset are host arrays. */
int ftk_wps_intervals(ftk_ctx* ctx, int contig_id, const int64_t* iv_start, const int64_t* iv_stop, int64_t n_iv,
                      const int64_t* out_offset, int64_t chrom_size, int32_t window_size, int32_t min_len,
                      int32_t max_len, int32_t mapq_min, int64_t* wps_out);

/* ftk_wps with the copy-back taken off the caller's path: returns once the kernel (ctx stream) and the copy of
 * the scores into wps_out_host (the ctx's copy stream, behind the kernel) are enqueued; the next calls on the ctx
 * - loading and scoring the next contig - overlap the copy.  *token_out identifies the result: the array is
 * valid after ftk_result_wait(ctx, token) (or ftk_ctx_sync).  Two results can be in flight; a third call
 * waits for the older one's copy.  Tokens count up and are never reused: waiting for an old token whose buffer has
 * been taken over by a later call returns at once (that call waited for the old copy before it reused the buffer); a
 * token that was never handed out is FTK_ERR_INVALID.  wps_out_host should come from ftk_host_alloc (a pageable array
 * is copied through a staging buffer and gains nothing).  A degenerate interval gives token -1 (nothing to wait for). */
int ftk_wps_async(ftk_ctx* ctx, int contig_id, int64_t start, int64_t stop, int64_t chrom_size, int32_t window_size,
                  int32_t min_len, int32_t max_len, int32_t mapq_min, int64_t* wps_out_host, int* token_out);
int ftk_result_wait(ftk_ctx* ctx, int token);

/* ftk_window_features (all arguments as there) FOLLOWED BY ftk_wps (all arguments as there) on the same contig, as
 * ONE launch when the feature request takes the FAST block path (midpoint policy, no length bounds on the coverage
 * filter, one mapq cut, a bin tiling; tabix fetch or - on a contig with read1 columns - the BAM read1 fetch rule):
 * the grid holds the feature blocks first and the WPS tiles behind them, so the feature pass's tail and the WPS ramp
 * overlap and WPS finds the contig's columns in the Infinity Cache.  wps_out may be device memory or a host array
 * (the scores then cross the link like ftk_wps': 16 bits each when they fit).  Any other request runs as the two
 * launches.  Results are those of the two calls (reference: frag/_coverage.py:117-130, _frag_length.py:147-153,
 * _delfi.py:443-472, _wps.py:156-188; BAM fetch rule: io/alignment.py:242-268). */
int ftk_window_features_wps(ftk_ctx* ctx, int contig_id, const int32_t* w_start, const int32_t* w_end, int64_t n_win,
                            const ftk_filter* f, int64_t* count_out, int32_t len_lo, int32_t n_bins, uint32_t* hist_out,
                            int64_t* overflow_out, int32_t delfi_mapq_min, const int32_t* bl_start, const int32_t* bl_end,
                            int64_t n_bl, const ftk_gaps* gaps, int64_t* short_out, int64_t* long_out, int64_t start,
                            int64_t stop, int64_t chrom_size, int32_t window_size, int32_t min_len, int32_t max_len,
                            int32_t mapq_min, int64_t* wps_out);

/* WPS of a whole contig AND the window features of a regular bin tiling in ONE pass over the fragments
 * (BASELINE config 5: coverage + WPS + length histogram + DELFI fused): bin k = [win_start + k * win_len,
 * win_start + (k + 1) * win_len), k < n_win, midpoint policy, tabix fetch semantics.  The block that scores
 * a 4096-base tile also classifies the fragments starting in it, so [start, stop) must cover every
 * fragment start of the contig (start <= 0, stop > last start) and win_len must be at least 4096 + the
 * longest fragment.  Outputs as in ftk_wps / ftk_window_features (NULL switches a feature off; results are
 * identical to the separate calls). */
int ftk_wps_window_features(ftk_ctx* ctx, int contig_id, int64_t start, int64_t stop, int64_t chrom_size,
                            int32_t window_size, int32_t min_len, int32_t max_len, int32_t mapq_min, int64_t* wps_out,
                            int32_t win_start, int32_t win_len, int32_t n_win, const ftk_filter* f, int64_t* count_out,
                            int32_t len_lo, int32_t n_bins, uint32_t* hist_out, int64_t* overflow_out,
                            int32_t delfi_mapq_min, const int32_t* bl_start, const int32_t* bl_end, int64_t n_bl,
                            const ftk_gaps* gaps, int64_t* short_out, int64_t* long_out);

/* Intervals of SEVERAL contigs in one launch: interval i is [iv_start[i], iv_stop[i]) of contig
 * contig_ids[i] (length chrom_size[i]) and writes its scores at wps_out + out_offset[i].  All arrays
 * except wps_out (host or device) are host arrays of n_iv entries (n_iv <= 64: whole contigs or large ranges). */
int ftk_wps_batch(ftk_ctx* ctx, const int32_t* contig_ids, const int64_t* iv_start, const int64_t* iv_stop,
                  const int64_t* chrom_size, const int64_t* out_offset, int64_t n_iv, int32_t window_size,
                  int32_t min_len, int32_t max_len, int32_t mapq_min, int64_t* wps_out);

/* ---- next row: cleavage profile ----------------------------------
 * frag/_cleavage_profile.py:33-90,204-216 for every base of [start, stop) (already
 * expanded by left/right and clipped by the caller, :201-202): fragments selected
 * like frag_array(start, stop, intersect_policy="any") with mapq >= mapq_min and
 * min_len <= len <= max_len (FTK_LEN_OPEN = no bound); depth = fragments covering the
 * base, ends = + fragments starting there plus - fragments whose stop is there;
 * prop_out = ends / depth * 100 (float64, 0 where depth == 0).
 * ftk_cleavage_intervals: n_iv intervals of one contig in one launch (host interval
 * arrays), interval i written at prop_out + out_offset[i]. */
int ftk_cleavage(ftk_ctx* ctx, int contig_id, int64_t start, int64_t stop, int32_t min_len, int32_t max_len,
                 int32_t mapq_min, double* prop_out);
int ftk_cleavage_intervals(ftk_ctx* ctx, int contig_id, const int64_t* iv_start, const int64_t* iv_stop, int64_t n_iv,
                           const int64_t* out_offset, int32_t min_len, int32_t max_len, int32_t mapq_min,
                           double* prop_out);

/* ---- per-base depth track ----------------------------------------------------------
 * depth(b) of a base b of [start, stop) = fragments of the contig with start <= b < end, mapq >= mapq_min and
 * min_len <= end - start <= max_len (FTK_LEN_OPEN = no bound): what `genomecov -bg` / a coverage track holds.
 * Fragments that reach beyond the region count on its bases only; zero-length fragments cover nothing.
 *   ftk_depth        one int32 per base into depth_out (stop - start values; a host or a device array)
 *   ftk_depth_runs   the run-length encoding, built on the device: the maximal intervals of constant depth inside
 *                    [start, stop) as run_start[i], run_end[i], run_depth[i] - sorted, disjoint, two runs that touch
 *                    differ in depth.  include_zero == 0 omits the runs of depth 0 (-bg); otherwise they are kept and
 *                    the runs tile the region (-bga).  The three arrays are library-owned host memory
 *                    (ftk_buffer_free each; NULL when *n_runs == 0).
 * start == stop is valid (no values, no runs).  FTK_ERR_INVALID: a NULL argument, start < 0, stop < start,
 * stop >= 2^30. */
int ftk_depth(ftk_ctx* ctx, int contig_id, int64_t start, int64_t stop, int32_t min_len, int32_t max_len,
              int32_t mapq_min, int32_t* depth_out);
int ftk_depth_runs(ftk_ctx* ctx, int contig_id, int64_t start, int64_t stop, int32_t min_len, int32_t max_len,
                   int32_t mapq_min, int include_zero, int32_t** run_start, int32_t** run_end, int32_t** run_depth,
                   int64_t* n_runs);

/* ---- next row: WPS post-processing (adjust_wps) ---------------------
 * frag/_adjust_wps.py:25-50,119-140 for n_iv score runs laid end to end in `scores`
 * (run i = scores[offsets[i] .. offsets[i+1]), offsets is a host array of n_iv + 1):
 *   x      = scores - edge_sub[i]                      (edge_sub NULL = no subtraction; host array)
 *   adj[o] = x[o + W/2] - stat(x[o .. o+W))            o in [0, len_i - W), stat = median, or mean
 *                                                      when use_mean; W = median_window, even, 2..2048
 *   out    = adj, or savgol_filter(adj, savgol_window, mode="interp") when savgol_window > 0:
 *            interior o: sum_j coef[j] * adj[o - h + j]            (h = savgol_window / 2, window odd)
 *            first h   : sum_j edge[o][j]     * adj[j]             (polynomial edge fit as a matrix)
 *            last h    : sum_j edge[h + k][j] * adj[m - window + j], o = m - h + k
 *            coef [savgol_window] and edge [2*h][savgol_window] are host arrays prepared by the caller.
 * Run i writes len_i - W values at out + offsets[i] - i*W.  Every run needs len_i >= W and, with the
 * Savitzky-Golay pass, len_i - W >= savgol_window (the reference raises ValueError in both cases).
 * The median is exact (selection, no arithmetic besides the final (a+b)/2). */
int ftk_wps_adjust(ftk_ctx* ctx, const double* scores, const int64_t* offsets, int64_t n_iv, int32_t median_window,
                   int use_mean, const double* edge_sub, int32_t savgol_window, const double* savgol_coef,
                   const double* savgol_edge, double* out);

/* ---- next row: DELFI per-bin GC count on the device ------------------
 * frag/_delfi.py:476-490 counts G + C of the upper-cased window sequence
 * (io/reference.py:120-189) once per bin on the host.  Here a contig's reference image
 * is uploaded once and every bin is counted in one launch:
 *   FTK_REF_FASTA_TEXT  the contig's raw FASTA text (bases and line breaks, no header line);
 *                       ranges are BYTE offsets into the image (faidx arithmetic is the caller's);
 *   FTK_REF_2BIT        the packed DNA of a .2bit record (T=0 C=1 A=2 G=3, first base in the high
 *                       bits); ranges are BASE positions; N / mask blocks are the caller's to subtract.
 * gc_out[i] = number of G/C (either case) in [range_lo[i], range_hi[i]). */
#define FTK_REF_FASTA_TEXT 0
#define FTK_REF_2BIT 1
int ftk_ref_upload(ftk_ctx* ctx, int ref_id, const uint8_t* image, int64_t n_bytes, int kind);
/* The same image read straight from a file: n_bytes at file_offset of `path` (the packed DNA of a 2bit record, the
 * text of a FASTA record), through page-locked chunks on several read threads, copies asynchronous on the ctx
 * stream.  Device blocks of released images are recycled (no device-wide synchronisation per contig). */
int ftk_ref_upload_file(ftk_ctx* ctx, int ref_id, const char* path, int64_t file_offset, int64_t n_bytes, int kind);
int ftk_ref_release(ftk_ctx* ctx, int ref_id);
int ftk_ref_gc_counts(ftk_ctx* ctx, int ref_id, const int64_t* range_lo, const int64_t* range_hi, int64_t n,
                      int64_t* gc_out);

/* ---- next row: end-motif / breakpoint-motif k-mer histograms ----------
 * frag/_end_motifs.py:51-187 (region_end_motifs) and frag/_breakpoint_motifs.py:53-196
 * (region_breakpoint_motifs) per window: every fragment the index query returns for the window
 * (overlap, or read1 overlap for BAM, and mapq >= mapq_min -- the reference applies NO length
 * filter here) adds
 *    forward: the k-mer ref[start + fwd_offset, +k)
 *    reverse: the reverse complement of ref[stop + rev_offset, +k)
 * to the window's histogram of 4^k bins in ACGT order (utils/utils.py:388-410, gen_kmers).
 *    both_strands            both k-mers of every fragment
 *    else negative_strand    only the reverse k-mer, of every fragment
 *    else                    only the forward k-mer, of forward-strand fragments
 * A k-mer holding anything but A/C/G/T (either case) is not counted.  A forward k-mer that falls
 * off the contig drops the fragment; a reverse one that does is counted in err_out when
 * rev_oob_is_error (the reference raises RuntimeError there, _end_motifs.py:137-145) and skipped
 * otherwise.  guard > 0 drops fragments with start - guard < 0 or start + guard >= chrom_len
 * (_breakpoint_motifs.py:127-135).
 *   end motifs:        k,  fwd_offset 0,     rev_offset -k,    guard 0,   rev_oob_is_error = both_strands
 *   breakpoint motifs: k (even), fwd_offset -k/2, rev_offset -k/2, guard k/2, rev_oob_is_error 0
 * The reference image needs its geometry first (ftk_ref_set_layout): contig length, and the FASTA
 * line layout (bases per line, bytes per line) or the 2bit record's N blocks (host arrays). */
typedef struct ftk_motif {
    int32_t k; /* 1..7 */
    int32_t fwd_offset, rev_offset;
    int32_t both_strands, negative_strand;
    int32_t guard;
    int32_t rev_oob_is_error;
} ftk_motif;
int ftk_ref_set_layout(ftk_ctx* ctx, int ref_id, int64_t chrom_len, int32_t line_bases, int32_t line_width,
                       const int32_t* nblock_start, const int32_t* nblock_end, int64_t n_nblocks);
int ftk_motif_counts(ftk_ctx* ctx, int contig_id, int ref_id, const int32_t* w_start, const int32_t* w_end,
                     int64_t n_win, const ftk_motif* motif, int32_t mapq_min, int32_t fetch_mode,
                     uint32_t* counts_out /* [n_win][4^k] */, int64_t* nfrag_out /* [n_win] or NULL */,
                     int64_t* err_out /* [n_win] */);

/* ---- fragment length x GC tables (csrc/ftk_gcbias.hip) ---------------------------------------------
 * What deepTools computeGCBias, Griffin and GCparagon measure.  A base IS GC when it is G, C, g or c.  A base IS N
 * when, in a 2bit image, it lies inside one of the record's N blocks, or, in a FASTA image, it is any sequence byte
 * other than ACGTacgt (line terminators are not bases).  gc(a, b) = GC bases of seq[a:b]; it is UNDEFINED when
 * a < 0, b > chrom_len, b - a > FTK_GC_MAX_LEN or seq[a:b] holds an N base.  The image needs its geometry
 * (ftk_ref_set_layout).
 *   ftk_frag_gc        gc_out[i] = gc(start, end) of fragment i of the resident contig (resident order), or -1 when
 *                      the fragment is not kept (mapq < mapq_min, length outside [min_len, max_len], FTK_LEN_OPEN =
 *                      no bound) or its gc is undefined (lengths above FTK_GC_MAX_LEN and below 1 included).
 *   ftk_frag_gc_table  observed: table[L - len_lo][g] = fragments with mapq >= mapq_min, L = end - start in
 *                      [len_lo, len_hi] and gc(start, end) == g; *n_skipped = fragments that pass the MAPQ and length
 *                      rule with gc undefined.
 *   ftk_ref_gc_table   expected: table[L - len_lo][g] = positions p of [pos_lo, pos_hi) with p % stride == 0 (on the
 *                      absolute coordinate: the tables of two halves of a range sum to the table of the range) and
 *                      gc(p, p + L) == g.  pos_hi > chrom_len is allowed: such windows are undefined.
 * Tables are int64, row-major, (len_hi - len_lo + 1) x (len_hi + 1), host or device; every cell is written by the
 * call.  An empty contig or range gives zeros.  FTK_ERR_INVALID: a NULL pointer, a reference without layout,
 * len_lo < 1, len_hi < len_lo, len_hi > FTK_GC_MAX_LEN, stride < 1, pos_lo < 0, pos_hi < pos_lo, chrom_len >= 2^30;
 * FTK_ERR_NO_CONTIG: an unknown contig or reference. */
#define FTK_GC_MAX_LEN 1000
int ftk_frag_gc(ftk_ctx* ctx, int contig_id, int ref_id, int32_t min_len, int32_t max_len, int32_t mapq_min,
                int16_t* gc_out /* n fragments of the contig; host or device */);
int ftk_frag_gc_table(ftk_ctx* ctx, int contig_id, int ref_id, int32_t len_lo, int32_t len_hi, int32_t mapq_min,
                      int64_t* table_out, int64_t* n_skipped);
int ftk_ref_gc_table(ftk_ctx* ctx, int ref_id, int64_t pos_lo, int64_t pos_hi, int32_t len_lo, int32_t len_hi,
                     int64_t stride, int64_t* table_out);

/* ---- per-fragment weights and their sums per window (csrc/ftk_weights.hip) -------------------------
 * A resident contig can carry ONE weight per fragment: a uint32 in units of 2^-16 (FTK_WEIGHT_ONE = 1.0), in resident
 * order, kept on the device until ftk_frags_release or until the contig id is loaded again.  Window sums are int64
 * sums of those units (fewer than 2^31 fragments times a weight below 2^32 cannot overflow), so every result is exact
 * and independent of the order of arrival.
 *   ftk_frags_set_weights     attaches an arbitrary column: n = the contig's fragment count, w a host or device array.
 *   ftk_frags_weights         reads the column back into a host or device array of as many elements;
 *                             FTK_ERR_INVALID ("... no weights column") when the contig has none.
 *   ftk_frags_set_gc_weights  GC-bias weights: w[i] = table[L - len_lo][g] for a fragment with mapq >= mapq_min,
 *                             L = end - start in [len_lo, len_hi] and g = gc(start, end) defined as for ftk_frag_gc
 *                             (above); every other fragment gets 0.  `table` is a HOST array of shape
 *                             [len_hi - len_lo + 1][len_hi + 1], the layout of ftk_frag_gc_table's output; lengths and
 *                             image as there (1 <= len_lo <= len_hi <= FTK_GC_MAX_LEN, a layout, chrom_len < 2^30).
 *                             *n_zero_out (host or device) = fragments that pass the MAPQ and length rule and got
 *                             weight 0: gc undefined, or a table cell of 0.  Replaces a column already attached.
 *   ftk_weighted_window_sums  sum_out[i] = sum of w over the fragments ftk_window_counts counts for window i under the
 *                             same filter `f` - FTK_POLICY_FETCH is accepted too: the index query alone;
 *                             n_weighted_out[i] (may be NULL) = how many of them have w > 0.  Windows are host
 *                             arrays, may overlap and come in any order, FTK_OPEN_LO / FTK_OPEN_HI as there; outputs
 *                             are host or device arrays and are overwritten.  n_win == 0 is FTK_OK; a contig without
 *                             a column is FTK_ERR_INVALID.
 * A failing call writes to none of its outputs. */
#define FTK_WEIGHT_ONE 65536u
int ftk_frags_set_weights(ftk_ctx* ctx, int contig_id, const uint32_t* w, int64_t n);
int ftk_frags_weights(ftk_ctx* ctx, int contig_id, uint32_t* w_out);
int ftk_frags_set_gc_weights(ftk_ctx* ctx, int contig_id, int ref_id, int32_t len_lo, int32_t len_hi, int32_t mapq_min,
                             const uint32_t* table, int64_t* n_zero_out);
int ftk_weighted_window_sums(ftk_ctx* ctx, int contig_id, const int32_t* w_start, const int32_t* w_end, int64_t n_win,
                             const ftk_filter* f, int64_t* sum_out, int64_t* n_weighted_out /* may be NULL */);

/* ---- site-aggregated midpoint profiles (csrc/ftk_siteprofile.hip) ---------------------------------
 * The profile of a resident contig's fragment midpoints around n_sites sites, aggregated per group of sites: site i has a
 * centre centre[i] in [0, 2^30), a flip flag flip[i] (non-zero for a site on the - strand; NULL: none is flipped) and a
 * group group[i] in [0, n_groups) (NULL: all in group 0).  n_bins = 2 * half_width / bin_size, which bin_size must
 * divide; 1 <= half_width <= 2^20, n_bins <= 4096, n_groups * n_bins <= 2^28, 0 <= n_sites < 2^31.
 *   A fragment passes with mapq >= mapq_min and min_len <= end - start <= max_len (closed; FTK_LEN_OPEN = no bound).
 *   Its midpoint is m = (start + end) >> 1.  It contributes to site i when d = m - centre[i] lies in
 *   [-half_width, half_width), in bin k = (d + half_width) / bin_size - bin n_bins - 1 - k of a flipped site:
 *   count[group[i]][k] += 1 and sum[group[i]][k] += w, w being the fragment's weight (above) with use_weights, else
 *   FTK_WEIGHT_ONE.
 * Sites are independent: a fragment near two sites counts for both, a site listed twice counts twice; sites come in
 * any order.  Every fragment of the contig is eligible - the read1 columns of a BAM contig play no part.  Bins that lie
 * outside the contig stay 0.  The sites are HOST arrays; sum_out and count_out (may be NULL) are host or device arrays of
 * n_groups * n_bins int64, row-major, overwritten (all 0 for n_sites == 0 or an empty contig).  The sums are integers, so
 * every result is exact and independent of the order of arrival.
 * FTK_ERR_INVALID for arguments outside the ranges above, a NULL centre (n_sites > 0) or sum_out, n_sites < 0, and for
 * use_weights on a contig without a weights column; FTK_ERR_NO_CONTIG for an unknown contig.  A failing call writes to
 * none of its outputs. */
int ftk_site_profile(ftk_ctx* ctx, int contig_id, const int32_t* centre, const uint8_t* flip /* NULL: none */,
                     const int32_t* group /* NULL: all 0 */, int64_t n_sites, int32_t n_groups, int32_t half_width,
                     int32_t bin_size, int32_t mapq_min, int32_t min_len, int32_t max_len, int use_weights,
                     int64_t* sum_out, int64_t* count_out /* may be NULL */);

/* ---- fragment length x midpoint offset maps around sites: the V-plot (csrc/ftk_vplot.hip) ----------
 * ftk_site_profile with a second axis.  Sites are as there: centre centre[i] in [0, 2^30), flip flag flip[i], group
 * group[i] in [0, n_groups).
 *   Offset axis: half_width = H lies in [1, 2^20]; bin_size = b divides 2 H; n_bins = 2 H / b <= 4096.
 *   Length axis: closed bounds 0 <= len_lo <= len_hi < 2^16; len_bin = lb >= 1 divides len_hi - len_lo + 1; n_rows =
 *   (len_hi - len_lo + 1) / lb <= 4096; n_groups * n_rows * n_bins <= 2^28.
 *   A fragment passes with mapq >= mapq_min and len_lo <= L = end - start <= len_hi.  Its midpoint is m = (start + end)
 *   >> 1.  It contributes to site i when d = m - centre[i] lies in [-H, H): to row r = (L - len_lo) / lb and column k =
 *   (d + H) / b - column n_bins - 1 - k when flip[i] is set; the flip reverses the offset axis only, never the length
 *   axis.  count[group[i]][r][k] += 1 and sum[group[i]][r][k] += w, w being the weight column's entry with use_weights,
 *   else FTK_WEIGHT_ONE.
 * Everything else is as in ftk_site_profile: sites are independent, repeats count twice, a fragment near two sites
 * counts for both; cells with nothing in them stay 0; there is no read1 fetch rule, so a BAM and the fragment file
 * exported from it give the same matrix; the sums are integers and exact whatever the order of arrival.  The sites are
 * HOST arrays; sum_out and count_out (may be NULL) are host or device arrays of n_groups * n_rows * n_bins int64,
 * row-major [group][row][bin], overwritten (all 0 for n_sites == 0 or an empty contig).
 * FTK_ERR_INVALID for arguments outside the ranges above, a NULL centre (n_sites > 0) or sum_out, n_sites < 0, and for
 * use_weights on a contig without a weights column; FTK_ERR_NO_CONTIG for an unknown contig.  A failing call writes to
 * none of its outputs. */
int ftk_site_vplot(ftk_ctx* ctx, int contig_id, const int32_t* centre, const uint8_t* flip /* NULL: none */,
                   const int32_t* group /* NULL: all 0 */, int64_t n_sites, int32_t n_groups, int32_t half_width,
                   int32_t bin_size, int32_t len_lo, int32_t len_hi, int32_t len_bin, int32_t mapq_min, int use_weights,
                   int64_t* sum_out, int64_t* count_out /* may be NULL */);

/* ---- fragment-end profiles and OCF window sums around sites (csrc/ftk_siteends.hip) -----------------
 * Where fragments END relative to a site: what orientation-aware cfDNA fragmentation (OCF, Sun et al., Genome Research
 * 2019) is computed from.  Sites, groups and the offset axis are as in ftk_site_profile: centre centre[i] in [0, 2^30),
 * flip flag flip[i], group group[i] in [0, n_groups); half_width = H in [1, 2^20]; bin_size = b divides 2 H; n_bins =
 * 2 H / b <= 4096; n_groups * 2 * n_bins <= 2^28; 0 <= n_sites < 2^31.
 *   A fragment [start, end) passes with mapq >= mapq_min and min_len <= end - start <= max_len (closed; FTK_LEN_OPEN =
 *   no bound).  A passing fragment has two ends: its U end on base `start` and its D end on base `end - 1`; a fragment
 *   of length 1 has both on one base and counts in both tracks.  (A fragment that holds no base, end <= start, has no
 *   ends.)
 *   Group profile.  For site i, each end at position x with d = x - centre[i] in [-H, H) falls in bin k = (d + H) / b:
 *   count[group[i]][track][k] += 1 and sum[group[i]][track][k] += w, w being the fragment's weight with use_weights,
 *   else FTK_WEIGHT_ONE; track is 0 for a U end and 1 for a D end.  A flipped site uses bin n_bins - 1 - k AND THE OTHER
 *   TRACK: what is upstream on the genome is downstream of a site on the - strand.  The two ends of a fragment are
 *   independent events: either, both or neither may fall in the window.
 *   Per-site window sums (site_sum_out != NULL).  With peak = p and flank = w, 0 <= w < p and p + w < H, every site i
 *   gets four sums in GENOME orientation - the flip flag is not applied:
 *     left_up, left_down    the U ends and the D ends with d in [-p - w, -p + w]
 *     right_up, right_down  the U ends and the D ends with d in [ p - w,  p + w]      (both ranges closed)
 *   site_sum_out[i][0..3] = their weights summed in that order, site_count_out[i][0..3] (may be NULL) = how many they
 *   are, rows in the CALLER'S order of the sites.  The score is OCF_i = (left_down - left_up) + (right_up - right_down).
 *   Mirroring a site - d -> -d with U and D swapped, which is what the - strand does to it - maps left_down <-> right_up
 *   and left_up <-> right_down, and so OCF_i onto itself: the score does not depend on the strand, which is why no
 *   flip is applied.  With site_sum_out == NULL, peak, flank and site_count_out are ignored.
 * Sites are independent: a fragment near two sites counts for both, a site listed twice counts twice (and has two rows);
 * sites come in any order.  The read1 columns of a BAM contig play no part.  The sites are HOST arrays; sum_out and
 * count_out (may be NULL) are host or device arrays of n_groups * 2 * n_bins int64, row-major [group][track][bin];
 * site_sum_out and site_count_out host or device arrays of n_sites * 4 int64; all overwritten (all 0 for n_sites == 0 or
 * an empty contig).  The sums are integers, so every result is exact and independent of the order of arrival.
 * FTK_ERR_INVALID for arguments outside the ranges above, a NULL centre (n_sites > 0) or sum_out, n_sites < 0, sites that
 * are device arrays, and for use_weights on a contig without a weights column (the message names ftk_frags_set_weights
 * and ftk_frags_set_gc_weights); FTK_ERR_NO_CONTIG for an unknown contig.  A failing call writes to none of its outputs. */
int ftk_site_ends(ftk_ctx* ctx, int contig_id, const int32_t* centre, const uint8_t* flip /* NULL: none */,
                  const int32_t* group /* NULL: all 0 */, int64_t n_sites, int32_t n_groups, int32_t half_width,
                  int32_t bin_size, int32_t mapq_min, int32_t min_len, int32_t max_len, int use_weights, int32_t peak,
                  int32_t flank, int64_t* sum_out, int64_t* count_out /* may be NULL */, int64_t* site_sum_out /* may be NULL */,
                  int64_t* site_count_out /* may be NULL */);

/* ---- BGZF inflate on the device -------------------------------------------------------------------
 * The streaming decoder's host threads spend most of a fragment file's decode in DEFLATE; BGZF blocks are
 * independent streams of at most 64 KB of data, decoded here one wavefront per block (csrc/ftk_inflate.hip).
 * This entry point inflates a whole BGZF image (every block a BGZF member, as bgzip / htslib write them) held
 * in host memory and returns the data in host memory: *n_out = sum of the blocks' ISIZE fields; FTK_ERR_INVALID
 * when cap is too small (with *n_out set), FTK_ERR_FORMAT for anything that is not BGZF or does not decode to
 * its ISIZE.  An image of up to 4 GB of data (compressed and inflated) per call; compressed bytes beyond 2^28 go in
 * further launches of the kernel, which addresses its input by 32-bit bit positions.  (The fragment stream uses the
 * same kernel on device-resident pieces: FTK_DEVICE_INFLATE.) */
int ftk_bgzf_inflate_device(ftk_ctx* ctx, const uint8_t* file_bytes, int64_t n, uint8_t* out, int64_t cap, int64_t* n_out);

/* ---- fragment export: columns -> rows -> BGZF on the device (csrc/ftk_fragtext.hip) -------------------
 * The write direction of the decoders above: a resident contig's fragments that pass the keep rule
 * (mapq >= mapq_min, min_len <= end - start <= max_len, FTK_LEN_OPEN = no bound: the length / MAPQ half of
 * ftk_filter) as text rows in resident order (sorted by start, equal starts in the order they are held), the
 * file the decoders read (io/alignment.py:270-302):
 *   FTK_LAYOUT_FRAG  "<contig>\t<start>\t<end>\t<mapq>\t<+|->\n"
 *   FTK_LAYOUT_BED6  the same with a "." name column before mapq
 *   FTK_LAYOUT_BED3  "<contig>\t<start>\t<end>\n"
 * `name` is the contig name to print (1..255 bytes).  A contig's text must stay below 4 GB.  The `_masked` forms
 * below add a whitelist / blacklist of regions to the keep rule.
 *   ftk_frags_format_rows    the formatter alone: the rows in library-owned host memory (*out, ftk_buffer_free;
 *                            NUL-terminated), *out_len bytes, *n_rows kept rows (may be NULL).  The bytes are those of
 *                            ftk_format_frag_rows for the kept rows (bed3: its first three columns).
 *   ftk_bgzf_deflate_device  the mirror of ftk_bgzf_inflate_device: n host bytes in, a BGZF image out - one member
 *                            per 0xFF00 bytes (18-byte header with BSIZE, raw DEFLATE: per block the smallest of
 *                            stored / fixed / dynamic codes, CRC-32, ISIZE), the 28-byte EOF block when write_eof.
 *                            *n_out = bytes of the image; FTK_ERR_INVALID (with *n_out set) when cap is too small.
 *                            block_offsets (may be NULL): ceil(n / 0xFF00) + 1 entries, as ftk_bgzf_write's.  The
 *                            image depends on the input alone.  At most 4 GB per call.
 *   ftk_frags_write          format, deflate, compact on the device, one copy to the host, one write: the contig's
 *                            members are appended to `path` (append == 0: the file is created / truncated first) and
 *                            the EOF block behind them when write_eof; the text never visits the host.  A contig
 *                            starts on a fresh block, so its virtual offset is its first member's file offset.
 *                            deflate_on_host != 0 or FTK_EXPORT_DEFLATE=host: the same text goes through
 *                            ftk_bgzf_write at level 1 instead (the A/B and size yardstick).  *res receives what a
 *                            tabix index needs; its four arrays are library-owned (ftk_buffer_free each; NULL when
 *                            the contig keeps no row - such a contig writes no member). */
#define FTK_LAYOUT_FRAG 0
#define FTK_LAYOUT_BED6 1
#define FTK_LAYOUT_BED3 2
typedef struct ftk_export_result {
    int64_t n_rows;     /* kept rows                                                             */
    int64_t text_bytes; /* bytes of their text                                                   */
    int64_t first_off;  /* file offset of the contig's first member                              */
    int64_t end_off;    /* file offset behind its last member                                    */
    int64_t n_linear;   /* 16 kb windows up to the last one a kept row reaches                   */
    uint64_t* linear;   /* virtual offset of the first row overlapping each window (a window
                         * without one takes the next window's, as htslib writes it)             */
    int64_t n_runs;     /* runs of consecutive rows with one bin (reg2bin: 14-bit shift, 5 levels) */
    int32_t* run_bin;   /* the run's bin                                                         */
    uint64_t* run_beg;  /* virtual offsets of its first byte and behind its last byte            */
    uint64_t* run_end;
    double stage_ms[5]; /* format kernels, deflate + CRC kernels, scan + compaction (HIP events);
                         * device -> host copy, file write (wall clock)                          */
} ftk_export_result;
int ftk_frags_format_rows(ftk_ctx* ctx, int contig_id, const char* name, int32_t mapq_min, int32_t min_len,
                          int32_t max_len, int layout, char** out, int64_t* out_len, int64_t* n_rows);
int ftk_bgzf_deflate_device(ftk_ctx* ctx, const uint8_t* data, int64_t n, uint8_t* out, int64_t cap, int64_t* n_out,
                            int64_t* block_offsets, int write_eof);
int ftk_frags_write(ftk_ctx* ctx, int contig_id, const char* name, int32_t mapq_min, int32_t min_len, int32_t max_len,
                    int layout, const char* path, int append, int write_eof, int deflate_on_host, ftk_export_result* res);

/* Region masks in front of the formatter (csrc/ftk_fragtext.hip, mask_keep_kernel): a whitelist and / or a
 * blacklist of one contig as sorted, disjoint HOST intervals [start, end) with start < end (touching ones are
 * accepted and differ from their union for a zero-length fragment at the touch point; the Python loader merges
 * overlapping intervals only).  A fragment [s, e) is IN a mask when one interval [a, b) of it holds
 *   FTK_POLICY_MIDPOINT  a <= (s + e) / 2 < b        (utils/_frag_generator.py:35-42)
 *   FTK_POLICY_ANY       e > a and s < b             (utils/_frag_generator.py:44-50)
 * and a row is kept when it passes the MAPQ / length rule, is in the whitelist (if one is given) and is not in the
 * blacklist (if one is given).  Rows stay whole fragments, each written at most once, in resident order.  The
 * library checks order, start < end and the policy (FTK_ERR_INVALID), and copies the arrays to the device.
 *   ftk_frags_mask_keep          the mask test alone: keep_out[i] = 1 / 0 per resident row (n host bytes, n as
 *                                ftk_frags_info reports it), *n_kept their sum (may be NULL)
 *   ftk_frags_format_rows_masked / ftk_frags_write_masked
 *                                ftk_frags_format_rows / ftk_frags_write with the mask in the keep rule; mask ==
 *                                NULL is the unmasked call (the two are thin calls of these).  The mask kernel's
 *                                time (and the intervals' copy) counts into stage_ms[0].
 *   ftk_mask_lds_intervals       intervals of one mask a workgroup (1024 rows) keeps in LDS; a tile whose rows can
 *                                touch more searches the global arrays instead (same result) */
typedef struct ftk_region_mask {
    const int32_t *wl_start, *wl_end;
    int64_t n_wl; /* < 0: no whitelist; 0: a whitelist that holds nothing on this contig */
    const int32_t *bl_start, *bl_end;
    int64_t n_bl; /* <= 0: no blacklist */
    int32_t policy; /* FTK_POLICY_MIDPOINT | FTK_POLICY_ANY */
} ftk_region_mask;
int ftk_mask_lds_intervals(void);
int ftk_frags_mask_keep(ftk_ctx* ctx, int contig_id, const ftk_region_mask* mask, uint8_t* keep_out, int64_t* n_kept);
int ftk_frags_format_rows_masked(ftk_ctx* ctx, int contig_id, const char* name, int32_t mapq_min, int32_t min_len,
                                 int32_t max_len, int layout, char** out, int64_t* out_len, int64_t* n_rows,
                                 const ftk_region_mask* mask);
int ftk_frags_write_masked(ftk_ctx* ctx, int contig_id, const char* name, int32_t mapq_min, int32_t min_len,
                           int32_t max_len, int layout, const char* path, int append, int write_eof, int deflate_on_host,
                           ftk_export_result* res, const ftk_region_mask* mask);

/* ---- output writers (host only; no ctx / GPU needed) ---------------------------------------------
 * The reference prints per-base results one Python f-string at a time (frag/_wps.py:208-229 WIG,
 * frag/_multi_wps.py:328-341 bedGraph) and hands bigWig entries to pyBigWig (:300-325).  These format the
 * same bytes on all host threads.  Buffers and arrays returned through `out` pointers are owned by the
 * library until ftk_buffer_free.  n_threads <= 0: all usable cores.  Errors: ftk_fragtable_error().
 * Several results are laid end to end as RUNS: run k = values[offsets[k] .. offsets[k+1]) starts at base
 * iv_start[k] (what ftk_wps_intervals / ftk_cleavage_intervals produce; one run = one interval).
 *   ftk_format_wig_i64       "<v>\n" per value (the body of a fixedStep WIG)
 *   ftk_format_bedgraph_i64  "<contig>\t<pos>\t<pos+1>\t<v>\n" per value of every run
 *   ftk_format_bedgraph_f64  the same for float64 values printed as Python's repr(float) prints them
 *                            (shortest round-trip digits; exponent form outside 1e-4 <= |v| < 1e16)
 *   ftk_format_bedgraph_runs "<contig>\t<start>\t<end>\t<depth>\n" per run of a depth track (ftk_depth_runs)
 *   ftk_file_write           data -> path (truncate or append); gzip_level > 0 writes gzip members of 1 MB
 *                            of text each, compressed in parallel (a valid multi-member .gz: gzip.open,
 *                            zcat, bgzip -d read it as one stream)
 *   ftk_gzip_members         the same gzip members into memory (*out, ftk_buffer_free): what a rank that does
 *                            not own the output file hands to the rank that writes it (multi-GPU runs of
 *                            multi_wps / multi_cleavage_profile: every rank formats and compresses the rows of
 *                            its own contigs, rank 0 concatenates the members in order)
 *   ftk_bigwig_fixedstep_sections  the data sections of one `addEntries(chrom, start, values=..., span=1,
 *                            step=1)` call PER RUN: values (value_kind 0 = int64, 1 = float64) cut into
 *                            sections of items_per_section float32 items (never across runs), each with
 *                            its 24-byte section header, zlib-compressed; *out holds the sections back to
 *                            back; section_table_out[3s..3s+2] = chromStart, chromEnd, compressed bytes of
 *                            section s; section_stats_out[4s..4s+3] = min, max, sum, sum of squares of its
 *                            float32 values (inputs of the zoom level and the total summary). */
int ftk_format_wig_i64(const int64_t* values, int64_t n, int n_threads, char** out, int64_t* out_len);
int ftk_format_bedgraph_i64(const char* contig, const int64_t* iv_start, const int64_t* offsets, int64_t n_iv,
                            const int64_t* values, int n_threads, char** out, int64_t* out_len);
int ftk_format_bedgraph_f64(const char* contig, const int64_t* iv_start, const int64_t* offsets, int64_t n_iv,
                            const double* values, int n_threads, char** out, int64_t* out_len);
int ftk_format_bedgraph_runs(const char* contig, const int32_t* run_start, const int32_t* run_end,
                             const int32_t* run_depth, int64_t n, int n_threads, char** out, int64_t* out_len);
void ftk_buffer_free(void* p);
int ftk_file_write(const char* path, const char* data, int64_t n, int gzip_level, int n_threads, int append);
int ftk_gzip_members(const char* data, int64_t n, int gzip_level, int n_threads, char** out, int64_t* out_len);
/* The array frag/_wps.py:181-188 returns -- numpy records ('contig', 'U16'), ('start', 'i8'), ('wps', 'i8'), 80 bytes
 * each: contig name as 16 UCS-4 code points (zero padded), start + i, values[i] -- filled by the host threads (for a
 * chromosome that array is gigabytes; one numpy thread takes longer over it than the GPU over the scores). */
int ftk_fill_wps_records(void* dst, int64_t n, const uint32_t contig_ucs4[16], int64_t start, const int64_t* values,
                         int n_threads);
/* Fragment-file output (what the decoders read, io/alignment.py:270-302): rows "<contig>\t<start>\t<end>\t<mapq>\t<+|->\n"
 * (bed6: a "." name column before mapq), and a BGZF container writer (blocks of 0xFF00 bytes of data compressed in
 * parallel, the standard EOF block when write_eof): block_offsets[k] = file offset of the block holding data bytes
 * [k * 0xFF00, ...), block_offsets[n_blocks] = offset behind the last data block -- what a tabix / BAI index needs. */
int ftk_format_frag_rows(const char* contig, const int32_t* start, const int32_t* end, const uint8_t* mapq,
                         const uint8_t* strand, int64_t n, int bed6, int n_threads, char** out, int64_t* out_len);
int ftk_bgzf_write(const char* path, const char* data, int64_t n, int level, int n_threads, int append, int write_eof,
                   int64_t* block_offsets);
/* Test / bench tooling (BASELINE config 5 reads a whole-genome 60x BAM: ~1.2 G records): appends to `path` -- which
 * already holds the BAM header's BGZF blocks -- the coordinate-sorted paired-end records of ONE contig, two per
 * fragment (read1: flag 99 / 83, at the fragment's start when strand != 0, else at its end; the mate mirrored;
 * TLEN = +-(end - start); one `read_len`M CIGAR; name = the fragment's index in `name_len - 1` decimal digits), built,
 * sorted (position, read1 before read2, fragment index) and deflated by the host threads in windows of 512 kb, so memory
 * stays bounded and the rate is libdeflate's.  Fragments must be sorted by start with end >= start + read_len.
 * linear (may be NULL): the contig's 16 kb BAI linear index, n_linear >= ((contig_len + read_len) >> 14) + 1 entries
 * preset to all-ones; entry w receives the virtual offset of the first record overlapping window w.  first_off / end_off:
 * file offsets of the contig's first block and behind its last one (-1 / unchanged file end when it has no records).
 * What the reference reads these files with: pysam.AlignmentFile.fetch, io/alignment.py:242-268. */
int ftk_synth_bam_contig(const char* path, int32_t ref_id, int64_t contig_len, const int32_t* start, const int32_t* end,
                         const uint8_t* mapq, const uint8_t* strand, int64_t n, int32_t read_len, int32_t name_len,
                         uint64_t seed, int level, int n_threads, uint64_t* linear, int64_t n_linear,
                         int64_t* first_off, int64_t* end_off, int64_t* n_records_out);
int ftk_bigwig_fixedstep_sections(uint32_t chrom_id, const int64_t* iv_start, const int64_t* offsets, int64_t n_iv,
                                  const void* values, int value_kind, int32_t items_per_section, int level,
                                  int n_threads, char** out, int64_t* out_len, int64_t* n_sections_out,
                                  int64_t** section_table_out, double** section_stats_out);

/* ---- spectrum: the periodogram of integer score runs at integer periods ----------------------------
 * What the WPS is read for downstream of the per-base track: its periodicity over a gene body (the intensity at
 * 120-280 bp, the 193-199 bp band above all).  Computed on the device, so that no per-base value crosses to the host.
 *
 * THE RULE.  A run is N integer scores v[0..N) of one region, n = base - region start.  For an integer period p in bases:
 *     m    = detrend ? (sum v) / N : 0             (the sum exact in int64, one float64 division)
 *     w[n] = split cosine bell of fraction a:      M = floor(a * N);
 *            w[n] = w[N-1-n] = 0.5 * (1 - cos(pi * (2n + 1) / (2M)))  for n < M, 1 elsewhere   (a = 0: all 1)
 *     x[n] = (v[n] - m) * w[n]
 *     j    = n mod p                               (the angle is ALWAYS formed from n mod p, never from n)
 *     re_p =  sum_n x[n] * cos(2 pi j / p)
 *     im_p = -sum_n x[n] * sin(2 pi j / p)
 *     ssw  =  sum_n w[n]^2
 * All of it in float64: x, the twiddles and the accumulators.  The twiddles of a period come from a p-entry table.
 * N == 0 gives zeros (ssw included).  Each (run, period) sum is formed in an order that depends on N and p alone - not on
 * the other runs or periods of the call, their order, the launch or any atomic - so a result is the same bits in every
 * call that asks for it (csrc/ftk_spectrum.hip says how).
 *
 * ftk_track_spectrum: run i is scores[offsets[i], offsets[i+1]) (scores: host or device; offsets: host, n_iv + 1 entries,
 * non-negative and non-decreasing); out[(i * n_per + k) * 2 + {0, 1}] = (re, im) of run i at periods[k] (host or device),
 * ssw_out[i] (host or device, may be NULL) its ssw.
 * ftk_wps_spectrum: the runs are the WPS of the intervals [iv_start[i], iv_stop[i]) of a resident contig - the scores of
 * the interval form of the WPS call with the same arguments, written to device scratch and transformed there.  The
 * intervals are taken in consecutive batches of at most batch_bases bases (0: the library's choice, 2^25; an interval
 * longer than that is a batch of its own); every batch reuses the scratch, 16 bytes per base.  Interval validity is that of
 * the interval form; a degenerate interval (stop <= start) is an empty run.
 * FTK_ERR_INVALID: a NULL argument (ssw_out excepted), device pointers for offsets / periods / the interval arrays,
 * decreasing offsets, a run longer than 2^22, a score with |v| >= 2^31 (found on the device: the outputs are written, the
 * call fails), n_per outside 0..1024, a period outside 2..4096, taper outside [0, 0.5], a negative batch_bases.  n_iv == 0
 * or n_per == 0 is valid and writes nothing. */
int ftk_track_spectrum(ftk_ctx* ctx, const int64_t* scores, const int64_t* offsets, int64_t n_iv, const int32_t* periods,
                       int32_t n_per, double taper, int detrend, double* out, double* ssw_out);
int ftk_wps_spectrum(ftk_ctx* ctx, int contig_id, const int64_t* iv_start, const int64_t* iv_stop, int64_t n_iv,
                     int64_t chrom_size, int32_t window_size, int32_t min_len, int32_t max_len, int32_t mapq_min,
                     const int32_t* periods, int32_t n_per, double taper, int detrend, int64_t batch_bases, double* out,
                     double* ssw_out);

/* ---- peaks: nucleosome calls from the adjusted WPS -----------------------------------------------------
 * The step the per-base WPS, its adjustment (ftk_wps_adjust) and its periodogram lead up to in Snyder et al. 2016: the
 * positions of nucleosomes, called on the device so that no per-base value crosses to the host.  A call set is small,
 * about one record per 190 bases.
 *
 * THE RULE.  The input is a run a[0..n) of finite float64 adjusted scores.  Parameters: skip >= 0, 0 <= max_gap <=
 * FTK_PEAKS_MAX_GAP, 1 <= min_region <= short_max <= max_region <= FTK_PEAKS_MAX_REGION.
 *  1. Callable track: [lo, hi) = [skip, n - skip), empty when hi <= lo.  (The fused call takes skip = savgol_window / 2,
 *     the points of the polynomial edge fit, and 0 without Savitzky-Golay.)
 *  2. Regions: take the positions of the track with a > 0.  Two neighbouring positive positions belong to one region
 *     when at most max_gap positions lie between them.  A region [r0, r1) begins and ends on a positive position.
 *  3. Open regions: r0 - lo <= max_gap or hi - r1 <= max_gap - positions outside the track could still join it.  Not called.
 *  4. Length L = r1 - r0.  L < min_region: short, not called.  L > max_region: long, not called.
 *  5. Median m of the L values of the region, the gap values included: the middle element of the sorted values for odd
 *     L, (s[L/2 - 1] + s[L/2]) / 2 in float64 for even L.
 *  6. Windows: the maximal runs of positions of the region with a > m, strictly.  None (all values equal): the region
 *     is flat, not called.
 *  7. A window's area: the sum of its values in float64, added to 0 left to right, one addition per value, never reassociated.
 *  8. L <= short_max: the one window of largest area, the leftmost of equals, whatever its own length.
 *     L >  short_max: every window whose length lies in [min_region, short_max].
 *  9. A call is (run, start, stop, summit, height, area): [start, stop) the window, summit the leftmost position of the
 *     window's largest value, height that value.  Calls come ordered by (run, start).
 * 10. Per run six int64 counters, in this order: regions, open, short, long, flat, calls.
 * A closed region and its calls depend on the scores within max_gap + 1 positions of it alone, and a run of n scores
 * yields at most n / (max_gap + 2) + 1 regions and n / (min_region + 1) + 1 calls: the room for both is reserved from the
 * lengths, nothing waits for the device between the passes, and a call is the same bits in every call that asks for it.
 *
 * ftk_track_peaks: run r is scores[offsets[r], offsets[r+1]) (scores: host or device; offsets: host, n_runs + 1 entries,
 * non-negative and non-decreasing).  start / stop / summit count from the run's first score.  The six columns come back
 * in host blocks of the library's, *n_calls entries each (NULL when there is no call), to be released with
 * ftk_buffer_free; stats: n_runs * 6 counters of the caller's (host or device).
 * ftk_wps_peaks: the runs are the adjusted WPS of the intervals [iv_start[i], iv_stop[i]) of a resident contig - the
 * scores of the interval form of the WPS call, converted to float64, put through ftk_wps_adjust's running median
 * (median_window) and Savitzky-Golay pass (savgol_window with its coef / edge arrays; 0: none) and called with skip =
 * savgol_window / 2, all in device scratch, in consecutive batches of at most batch_bases bases (0: the library's
 * choice, 2^25; an interval longer than that is a batch of its own).  run is the interval's number; start / stop /
 * summit are contig positions (interval start + median_window / 2 + position in the adjusted run).  An interval shorter
 * than median_window + max(savgol_window, 1) has no callable track: no call, zero counters, no error.  stats: n_iv * 6
 * counters in host memory.  The same calls as the three calls in a row, without a per-base value reaching the host.
 * FTK_ERR_INVALID: a NULL argument, device pointers for offsets / the interval, savgol and (fused call) stats arrays,
 * decreasing offsets, a parameter outside the ranges above, the median / savgol window rules of ftk_wps_adjust, a
 * negative batch_bases, a score that is not finite (found on the device: the call fails after the passes have run).
 * A failing call hands out no block.  n_runs == 0 / n_iv == 0 is valid. */
#define FTK_PEAKS_MAX_REGION 1024
#define FTK_PEAKS_MAX_GAP 63
#define FTK_PEAKS_REGIONS 0
#define FTK_PEAKS_OPEN 1
#define FTK_PEAKS_SHORT 2
#define FTK_PEAKS_LONG 3
#define FTK_PEAKS_FLAT 4
#define FTK_PEAKS_CALLS 5
int ftk_track_peaks(ftk_ctx* ctx, const double* scores, const int64_t* offsets, int64_t n_runs, int64_t skip, int32_t max_gap,
                    int32_t min_region, int32_t short_max, int32_t max_region, int32_t** run, int64_t** start, int64_t** stop,
                    int64_t** summit, double** height, double** area, int64_t* n_calls, int64_t* stats);
int ftk_wps_peaks(ftk_ctx* ctx, int contig_id, const int64_t* iv_start, const int64_t* iv_stop, int64_t n_iv,
                  int64_t chrom_size, int32_t window_size, int32_t min_len, int32_t max_len, int32_t mapq_min,
                  int32_t median_window, int32_t savgol_window, const double* savgol_coef, const double* savgol_edge,
                  int32_t max_gap, int32_t min_region, int32_t short_max, int32_t max_region, int64_t batch_bases,
                  int32_t** run, int64_t** start, int64_t** stop, int64_t** summit, double** height, double** area,
                  int64_t* n_calls, int64_t* stats);

/* ---- preferred ends: Poisson-tested fragment-end calls --------------------------------------------------
 * The end-signature feature of Chan et al. 2016 / Jiang et al. 2018 (one combined track) and Sun et al. 2019 (U and D
 * ends apart): the contig positions on which significantly more fragments end than the end density of the window
 * centred on them predicts.  Every base is tested on the device and only the calls reach the host - under a uniform
 * null at 30x and alpha = 0.01 about 0.6 % of the positions.
 *
 * THE RULE.  Everything in it is an integer.
 *  1. Ends: a fragment [start, end) of the resident contig passes with mapq >= mapq_min, min_len <= end - start <=
 *     max_len (FTK_LEN_OPEN = no bound) and end > start.  Its U end is on base start, its D end on base end - 1 (the
 *     convention of ftk_site_ends); a fragment of length 1 puts both on one base.  u(b) / d(b) count the U / D ends on
 *     base b of [0, chrom_size); ends on bases outside that range do not exist.  The read1 columns of a BAM contig play
 *     no part.
 *  2. Tracks: mode FTK_PREFENDS_COMBINED has one track e = u + d of kind FTK_PREFENDS_KIND_B (2); mode
 *     FTK_PREFENDS_SPLIT has two, e = u of kind FTK_PREFENDS_KIND_U (0) and e = d of kind FTK_PREFENDS_KIND_D (1), each
 *     tested against its own window total.
 *  3. Window: with half = h, 1 <= h <= FTK_PREFENDS_MAX_HALF: w_lo = max(b - h, 0), w_hi = min(b + h, chrom_size - 1),
 *     n_w = w_hi - w_lo + 1, T(b) = the sum of e over [w_lo, w_hi], the base itself included.  The window reads the
 *     contig and never stops at the bounds of the interval being called: whether a position is called does not depend
 *     on how the caller cuts the contig.
 *  4. Decision: with the caller's table thr[0 .. n_thr), 2 <= n_thr <= FTK_PREFENDS_MAX_THR, every entry < 2^40, a
 *     position is called on a track iff, in unsigned 64-bit arithmetic,
 *         e(b) >= min_count                                        (min_count >= 1)   and
 *         T(b) * 2^20 <= thr[min(e(b), n_thr - 1)] * n_w(b).
 *     Nothing overflows: T < 2^32 and n_w <= 4097.  thr[k] is the largest mean, in units of 2^-20 ends per base, at
 *     which k ends on one base are still significant; an entry of 0 means "never".  The library does not interpret the
 *     table (finaletoolkit_amd.utils.preferred_end_thresholds builds the Poisson one).
 *  5. A call is (run, pos, kind, count, total, n_w): run the interval's number, pos a contig position, count = e,
 *     total = T.  Calls come ordered by (run, pos, kind).
 *  6. Per interval six int64 counters, in this order: U ends on its positions, D ends on its positions, positions
 *     tested on track a (e >= min_count), positions tested on track b, calls on track a, calls on track b.  Split mode:
 *     a = U, b = D.  Combined mode: a is the combined track and the b slots hold 0.
 * Intervals [iv_start[i], iv_stop[i]) may overlap, touch, be empty or come in any order; each is a run of its own.
 *
 * ftk_preferred_ends: the six columns come back in host blocks of the library's, *n_calls entries each (NULL when there
 * is no call), to be released with ftk_buffer_free; stats: n_iv * 6 counters in host memory.  The intervals are walked
 * tile by tile in batches whose device scratch is bounded, so a whole chromosome may be one interval.  The call reads
 * the packed (length, mapq) column of the contig where the filter allows it and the wide columns otherwise, with the
 * same calls either way.  A call is the same bytes in every call that asks for it.
 * FTK_ERR_INVALID: a NULL argument (the interval and stats arrays may be NULL when n_iv == 0), device pointers for the
 * interval, table or stats arrays, n_iv < 0, an interval with start < 0, stop < start or stop > chrom_size, chrom_size
 * outside [0, 2^30), half, mode, min_count, n_thr or a table entry outside the ranges above.  FTK_ERR_NO_CONTIG: an
 * unknown contig.  A failing call hands out no block and writes no counter.  n_iv == 0, empty intervals and an empty
 * contig are valid: no calls, zero counters. */
#define FTK_PREFENDS_MAX_HALF 2048
#define FTK_PREFENDS_MAX_THR 4096
#define FTK_PREFENDS_COMBINED 0
#define FTK_PREFENDS_SPLIT 1
#define FTK_PREFENDS_KIND_U 0
#define FTK_PREFENDS_KIND_D 1
#define FTK_PREFENDS_KIND_B 2
int ftk_preferred_ends(ftk_ctx* ctx, int contig_id, const int64_t* iv_start, const int64_t* iv_stop, int64_t n_iv,
                       int64_t chrom_size, int32_t half, int32_t mode, int32_t min_count, const uint64_t* thr, int32_t n_thr,
                       int32_t min_len, int32_t max_len, int32_t mapq_min, int32_t** run, int64_t** pos, int32_t** kind,
                       int32_t** count, int64_t** total, int32_t** n_w, int64_t* n_calls, int64_t* stats /* n_iv * 6, host */);

/* ---- IFS hotspots: fragmentation hotspot calls from the Integrated Fragmentation Score ----------------------
 * The Integrated Fragmentation Score of Zhou et al. 2022 (CRAG): in a window sliding over the contig, IFS = n * (1 + mean
 * fragment length in the window / mean fragment length on the chromosome) over the fragments whose midpoint lies in the
 * window; a window whose IFS is significantly LOW against its local backgrounds and the chromosome is called, and
 * neighbouring called windows are merged into a hotspot.  Every window is scored and tested on the device and only the
 * called windows reach the host - about one in 10^4 at alpha = 1e-5.
 *
 * THE RULE.  Everything in it is an integer.
 *  1. Bins: with step = s, 1 <= s <= 65535, n_bins = ceil(chrom_size / s) and bin j is [j s, (j + 1) s); the last bin
 *     may be short.  A fragment [start, end) of the resident contig passes with mapq >= mapq_min, min_len <= end - start
 *     <= max_len (FTK_LEN_OPEN = no bound) and end > start.  Its midpoint is (start + end) >> 1 (the convention of
 *     ftk_site_profile); midpoints outside [0, chrom_size) do not exist.  c(j) counts the midpoints in bin j, l(j) sums
 *     their fragments' lengths, and with the caller's mean length L = mean_len, 1 <= L <= 65535, i(j) = c(j) L + l(j) is
 *     the bin's IFS in units of 1 / L.  The read1 columns of a BAM contig play no part.
 *  2. Windows: m bins per window, 1 <= m <= FTK_IFS_MAX_WINDOW_BINS.  Window k, 0 <= k <= n_bins - m, is bins k .. k + m -
 *     1 and spans [k s, min((k + m) s, chrom_size)).  n(k) = the sum of c and I(k) = the sum of i over those bins;
 *     q(k) = I(k) / L (floor) is the integer IFS.  A contig with n_bins < m has no window.  Window k belongs to interval
 *     [a, b) iff a <= k s and its span's end <= b.  Intervals [iv_start[i], iv_stop[i]) may overlap, touch, be empty or
 *     come in any order; each is a run of its own.
 *  3. Backgrounds: two half-widths in bins, h1 >= 1 and h2 (h2 == 0: the second is off; otherwise h2 >= h1), with
 *     max(h1, h2) + m <= FTK_IFS_MAX_REACH.  For half-width h the background of window k is bins [max(k - h, 0),
 *     min(k + m - 1 + h, n_bins - 1)], n_b their number and B the sum of i over them, the window's own bins included.
 *     The background reads the contig and never stops at the bounds of the interval being called: whether a window is
 *     called does not depend on how the caller cuts the contig.
 *  4. Decision: with the caller's table thr[0 .. n_thr), 1 <= n_thr <= FTK_IFS_MAX_THR, every entry < 2^32 - thr[q] a
 *     mean IFS per window in units of 2^-10 - a window is TESTED iff n(k) >= min_count (min_count >= 0), and a tested
 *     window is CALLED iff, with q = q(k) and in unsigned 64-bit arithmetic,
 *         q < n_thr   and   t = thr[q] != 0   and
 *         B_h m 2^10 >= t n_b_h L   for every active h   and
 *         (global_mean == 0  or  t <= global_mean)      (global_mean >= 0: the caller's, in the same 2^-10 units).
 *     There is no shared last entry: a window with q >= n_thr is never significantly low.  Nothing overflows: the
 *     device counters are 32 bits wide and sums are only ever differences of prefix sums, so every B < 2^32 is exact (the
 *     caller keeps a background's IFS below 2^32 / L); the left side is < 2^32 2^6 2^10 = 2^48 and the right side
 *     < 2^32 2^12 2^16 = 2^60.  thr[q] is the smallest mean at which an IFS of q is significantly low.  The library
 *     does not interpret the table (finaletoolkit_amd.utils.ifs_thresholds builds the Poisson one).
 *  5. A called window is (run, pos = k s, count = n, ifs = I, bg1 = B_h1, nb1 = n_b_h1, bg2, nb2): run the interval's
 *     number; bg2 and nb2 are 0 when h2 is off.  Called windows come ordered by (run, pos).
 *  6. Hotspots: two called windows k1 < k2 of one run with no called window between them belong to one hotspot iff
 *     k2 - k1 <= join, 1 <= join <= FTK_IFS_MAX_JOIN.  A hotspot of fewer than min_windows (>= 1) called windows is
 *     dropped.  A hotspot is (run, start = k_first s, stop = the span end of k_last, n_windows, summit, ifs, count, bg1,
 *     nb1): summit is the pos of its called window of smallest I, the leftmost of equals, and ifs, count, bg1 and nb1
 *     are that window's.  Hotspots come ordered by (run, start), never join across runs, and are the same however the
 *     library tiles and batches a run.
 *  7. Per interval six int64 counters, in this order: windows, tested windows, called windows, hotspots kept, hotspots
 *     dropped, bases covered by the kept hotspots (the bases of the union of their [start, stop)).
 *
 * ftk_ifs_hotspots: the eight called-window columns (w_*, *n_windows entries each) and the nine hotspot columns (h_*,
 * *n_hotspots entries each) come back in host blocks of the library's (NULL when there is none), to be released with
 * ftk_buffer_free; stats: n_iv * 6 counters in host memory.  The intervals are walked tile by tile in batches whose
 * device scratch is bounded, so a whole chromosome may be one interval; the merge runs on the host as the called windows
 * come home.  The call reads the packed (length, mapq) column of the contig where the filter allows it and the wide
 * columns otherwise, with the same bytes either way.
 * FTK_ERR_INVALID: a NULL argument (the interval and stats arrays may be NULL when n_iv == 0), device pointers for the
 * interval, table or stats arrays, n_iv < 0, an interval with start < 0, stop < start or stop > chrom_size, chrom_size
 * outside [0, 2^30), step, m, mean_len, h1, h2, min_count, n_thr, a table entry, global_mean, join or min_windows outside
 * the ranges above.  FTK_ERR_NO_CONTIG: an unknown contig.  A failing call hands out no block and writes no counter.
 * n_iv == 0, empty intervals and an empty contig are valid: nothing called, zero counters.
 *
 * ftk_ifs_track: the per-window form without the test - n(k) (int32) and I(k) (int64) of the windows of interval i, in
 * window order, at n_out / ifs_out[out_offset[i] ...] (the arrays: host or device; out_offset: host, n_iv non-negative
 * entries, laid out by the caller as for the interval form of the WPS call).  The same errors as above for the arguments
 * it has.
 * ftk_ifs_totals: the number and the length sum of the passing fragments with a midpoint in [0, chrom_size), reduced on
 * the device - what a caller needs for mean_len and global_mean. */
#define FTK_IFS_MAX_WINDOW_BINS 64
#define FTK_IFS_MAX_REACH 1024
#define FTK_IFS_MAX_THR 4096
#define FTK_IFS_MAX_JOIN 1024
int ftk_ifs_hotspots(ftk_ctx* ctx, int contig_id, const int64_t* iv_start, const int64_t* iv_stop, int64_t n_iv,
                     int64_t chrom_size, int32_t step, int32_t m, int32_t mean_len, int32_t h1, int32_t h2, int32_t min_count,
                     const uint64_t* thr, int32_t n_thr, int64_t global_mean, int32_t join, int32_t min_windows, int32_t min_len,
                     int32_t max_len, int32_t mapq_min, int32_t** w_run, int64_t** w_pos, int32_t** w_count, int64_t** w_ifs,
                     int64_t** w_bg1, int32_t** w_nb1, int64_t** w_bg2, int32_t** w_nb2, int64_t* n_windows, int32_t** h_run,
                     int64_t** h_start, int64_t** h_stop, int32_t** h_n_windows, int64_t** h_summit, int64_t** h_ifs,
                     int32_t** h_count, int64_t** h_bg1, int32_t** h_nb1, int64_t* n_hotspots, int64_t* stats /* n_iv * 6, host */);
int ftk_ifs_track(ftk_ctx* ctx, int contig_id, const int64_t* iv_start, const int64_t* iv_stop, int64_t n_iv,
                  const int64_t* out_offset, int64_t chrom_size, int32_t step, int32_t m, int32_t mean_len, int32_t min_len,
                  int32_t max_len, int32_t mapq_min, int32_t* n_out, int64_t* ifs_out);
int ftk_ifs_totals(ftk_ctx* ctx, int contig_id, int64_t chrom_size, int32_t min_len, int32_t max_len, int32_t mapq_min,
                   int64_t* n_frags, int64_t* len_sum);

/* ---- end context: nucleotide and dinucleotide profiles around fragment ends (csrc/ftk_endcontext.hip) --------
 * The figure cfDNA cleavage papers start from: the frequency of every base and base pair at each position of a window
 * around the fragment ends (or centres), in front of and inside the fragment, per fragment length class.
 *
 * Bases.  base(q) of a reference image that has its layout (ftk_ref_set_layout) is A = 0, C = 1, G = 2, T = 3 (either
 * case; the ACGT order of gen_kmers), and 4, written N, when q < 0, q >= chrom_len, or the base IS N by the rule of the
 * GC section above (a base of a 2bit N block; a FASTA byte other than ACGTacgt).  comp(x) = 3 - x for x < 4, comp(4) = 4.
 *
 * Which fragments count.  len_edges holds n_classes + 1 strictly ascending values, 1 <= len_edges[0] and
 * len_edges[n_classes] <= 2^30 (a HOST array).  A fragment [s, e) with L = e - s is kept when mapq >= mapq_min and
 * len_edges[0] <= L < len_edges[n_classes]; its class c is the one with len_edges[c] <= L < len_edges[c + 1].  There is
 * no other length bound: only the neighbourhood of the anchors is read.
 *
 * Readings.  Every kept fragment gives two oriented readings, for o in [-W, W], W = half_width:
 *    kind 0:  r0(o) = base(a0 + o)
 *    kind 1:  r1(o) = comp(base(a1 - o))
 *    FTK_CONTEXT_ENDS     a0 = s,            a1 = e - 1              the U end read 5'->3' on the + strand, the D end
 *                                                                    read 5'->3' on the - strand
 *    FTK_CONTEXT_CENTRE   a0 = s + (L >> 1), a1 = e - 1 - (L >> 1)   the same readings around the fragment's centre
 * In both modes o >= 0 lies inside the fragment and o < 0 in front of it; for kind 1 this is the orientation
 * ftk_motif_counts uses for its reverse k-mer.  Offsets may run past the fragment's other end (L < W): that is reference
 * sequence and is counted.
 *
 * The table.  out[c][k][o + W][5 rk(o) + rk(o + 1)] += 1 for every o of [-W, W): int64 of shape [n_classes][2][2 W][25].
 * The mononucleotide profile is the marginal over the second base, the dinucleotide profile the 16 cells with both bases
 * below 4.  n_kept_out[c] = kept fragments of class c, so every row out[c][k][j] sums to n_kept_out[c].
 *   ftk_end_context   the table and n_kept_out[n_classes] of a resident contig; outputs host or device, every cell
 *                     written by the call; an empty contig gives zeros.
 *   ftk_ref_context   the background: out25[5 a + b] = positions p of [pos_lo, pos_hi) within [0, chrom_len) with
 *                     base(p) = a and base(p + 1) = b.  The tables of two halves of a range sum to the table of the
 *                     range; pos_hi > chrom_len is allowed.
 *   ftk_end_context_lds_classes   classes one workgroup keeps in LDS at that width (the further classes of a call go to
 *                     further rows of the grid); 0 for a width outside [1, FTK_CONTEXT_MAX_HALF].
 * FTK_ERR_INVALID: a NULL pointer, a reference without layout, chrom_len >= 2^30, half_width outside
 * [1, FTK_CONTEXT_MAX_HALF], n_classes outside [1, FTK_CONTEXT_MAX_CLASSES], edges not strictly ascending or outside
 * their bounds, an unknown anchor, pos_lo < 0, pos_hi < pos_lo; FTK_ERR_NO_CONTIG: an unknown contig or reference.  A
 * failing call writes nothing. */
#define FTK_CONTEXT_MAX_HALF 128
#define FTK_CONTEXT_MAX_CLASSES 8
#define FTK_CONTEXT_ENDS 0
#define FTK_CONTEXT_CENTRE 1
int ftk_end_context(ftk_ctx* ctx, int contig_id, int ref_id, int32_t half_width, const int32_t* len_edges /* host */,
                    int32_t n_classes, int32_t mapq_min, int32_t anchor, int64_t* out, int64_t* n_kept_out);
int ftk_ref_context(ftk_ctx* ctx, int ref_id, int64_t pos_lo, int64_t pos_hi, int64_t* out25);
int ftk_end_context_lds_classes(int32_t half_width);

/* ---- co-fragmentation: pairwise KS distances between fragment-length histograms (csrc/ftk_cofrag.hip) ---------
 * The co-fragmentation map of Liu et al. 2019: a contig is cut into large bins, the fragment-length distributions of
 * every pair of bins are compared with the two-sample Kolmogorov-Smirnov statistic, and the rows of that distance
 * matrix are correlated (the host's part).  Everything the device returns is an integer.
 *
 *  1. Input: hist is N rows of n_bins uint32 cells, 1 <= N <= FTK_COFRAG_MAX_BINS, 1 <= n_bins <=
 *     FTK_COFRAG_MAX_LEN_BINS.  n(i) is the sum of row i, C(i, l) the sum of its cells 0 .. l.  Every n(i) must be
 *     < 2^31: a larger row sum is FTK_ERR_INVALID naming the first such row, found on the device before anything is
 *     written.
 *  2. Statistic: K(i, j) = max over l of |C(i, l) n(j) - C(j, l) n(i)|; the KS statistic is D = K / (n(i) n(j)).  Both
 *     products are below 2^62 and their difference fits a signed 64-bit word: nothing overflows.  K(i, i) = 0.  A pair
 *     with n(i) = 0 or n(j) = 0 has K = 0 by the formula; the caller masks it.  at(i, j) is the SMALLEST l at which the
 *     maximum is attained, 0 when K = 0.
 *  3. Outputs: k_out int64 [N][N], full and symmetric; at_out int32 [N][N], symmetric, NULL switches it off; n_out
 *     int64 [N].  Each may be host or device memory.  The call writes every cell; a failing call writes nothing.
 *
 * ftk_hist_ks        the rule over any histogram rows (host or device).
 * ftk_cofrag         exactly what ftk_hist_ks gives on the rows ftk_fraglen_hist returns for the same windows (1 <=
 *                    n_win <= FTK_COFRAG_MAX_BINS), filter, len_lo and n_bins - lengths outside [len_lo, len_lo +
 *                    n_bins) take no part - with overflow_out [n_win] (host or device) ftk_fraglen_hist's overflow
 *                    column.  The rows are built in the scratch and never leave the device.
 * ftk_hist_ks_shape  two constants of the tiled pair kernel: the edge T of the pair tile one workgroup computes and
 *                    the lengths it stages per LDS chunk (tests place their shapes around them).
 * FTK_COFRAG_ARRANGE=0 (read at every call) selects the thread-per-pair kernel instead of the tiled one; both give the
 * same cells.  FTK_ERR_INVALID: a NULL argument, N or n_bins out of range, a row sum >= 2^31, a bad filter;
 * FTK_ERR_NO_CONTIG: an unknown contig. */
#define FTK_COFRAG_MAX_BINS 4096
#define FTK_COFRAG_MAX_LEN_BINS 4096
int ftk_hist_ks(ftk_ctx* ctx, const uint32_t* hist /* host or device */, int64_t n_rows, int32_t n_bins, int64_t* k_out,
                int32_t* at_out /* NULL: off */, int64_t* n_out);
int ftk_cofrag(ftk_ctx* ctx, int contig_id, const int32_t* w_start, const int32_t* w_end, int64_t n_win, const ftk_filter* f,
               int32_t len_lo, int32_t n_bins, int64_t* k_out, int32_t* at_out, int64_t* n_out, int64_t* overflow_out);
int ftk_hist_ks_shape(int32_t* tile_out, int32_t* chunk_out);

/* ---- motif x length: end-motif counts per fragment length (csrc/ftk_motiflen.hip) -----------------------------
 * The joint table behind "motif frequency against fragment size" and the motif diversity score per length: what
 * ftk_motif_counts gives per window without a length filter, per length row of one contig, in one pass.
 *
 * Bases.  base(q) and comp(x) are those of the "end context" section above: A C G T = 0 .. 3, N = 4 (outside
 * [0, chrom_len), inside a 2bit N block, a FASTA byte other than ACGTacgt), comp(x) = 3 - x for x < 4, comp(4) = 4.
 *
 * Which fragments count.  A fragment [s, e) with L = e - s is KEPT when mapq >= mapq_min and len_lo <= L <= len_hi.  Its
 * row is r = (L - len_lo) / len_bin; there are n_rows = (len_hi - len_lo) / len_bin + 1 rows (the last one may be
 * narrower than len_bin).
 *
 * Readings.  Every kept fragment gives two readings of k bases; `shift` moves the anchor:
 *    kind 0 (U end, + strand):  u_i = base(s + shift + i),             i = 0 .. k-1
 *    kind 1 (D end, - strand):  d_i = comp(base(e - 1 - shift - i)),   i = 0 .. k-1
 * The code of a reading is sum x_i 4^(k-1-i): the first base is most significant, in the ACGT order of gen_kmers.  When
 * any base of the reading is 4 the reading goes to column 4^k ("undefined") instead.  shift = 0 gives the end motifs,
 * shift = -k/2 the breakpoint motifs: with fwd_offset = shift and rev_offset = -k - shift these are exactly the two k-mers
 * ftk_motif_counts reads.  Readings may run past the fragment's other end (L < k): that is reference sequence and it is
 * counted.
 *
 * The table.
 *    out[kind][r][code] += 1      int64, shape [2][n_rows][4^k + 1]
 *    n_kept_out[r]                int64, kept fragments of row r
 * Every row out[kind][r] therefore sums to n_kept_out[r], for both kinds.  Unlike ftk_motif_counts nothing is dropped and
 * nothing is an error at the contig's ends: an off-contig base makes the reading undefined, and that is all.
 *   ftk_motif_length_table      the table and n_kept_out[n_rows] of a resident contig; outputs host or device, every cell
 *                               written by the call; an empty contig gives zeros.
 *   ftk_motif_length_lds_rows   rows one workgroup keeps in LDS (the further rows of a call go to further rows of the
 *                               grid); 0 for k outside [1, FTK_MOTIFLEN_MAX_K].
 * FTK_ERR_INVALID: a NULL pointer, a reference without layout, chrom_len >= 2^30, k outside [1, FTK_MOTIFLEN_MAX_K],
 * |shift| > 4, len_lo < 1, len_hi < len_lo, len_hi > 2^30, len_bin < 1, n_rows > FTK_MOTIFLEN_MAX_ROWS;
 * FTK_ERR_NO_CONTIG: an unknown contig or reference.  A failing call writes nothing. */
#define FTK_MOTIFLEN_MAX_K 4
#define FTK_MOTIFLEN_MAX_ROWS 1024
int ftk_motif_length_table(ftk_ctx* ctx, int contig_id, int ref_id, int32_t k, int32_t shift, int32_t len_lo, int32_t len_hi,
                           int32_t len_bin, int32_t mapq_min, int64_t* table_out, int64_t* n_kept_out);
int ftk_motif_length_lds_rows(int32_t k);

/* ---- multi-GPU (SURVEY 8-e, 8-b's export list) -------------------------------------------------
 * One process and one ftk_ctx per GPU.  Contigs / genome runs are dealt to the ranks by the host and every window,
 * bin and base depends on its own contig's fragments only, so the data path has no collective.  What remains are the
 * two exchanges that stand where the reference collects its Pool's results: the all-gather of the per-bin DELFI /
 * per-interval rows (frag/_delfi.py:289-300: pool.starmap's result list; frag/_coverage.py:212-248) and the all-reduce
 * of the genome-wide total of coverage(normalize=True) (frag/_coverage.py:215-227) -- RCCL over xGMI, here behind the
 * C ABI so that a host in any language can shard (finaletoolkit_amd/comm.py is the ctypes host).  librccl is resolved
 * when the first communicator is created (dlopen "librccl.so.1": a copy already in the process, e.g. torch's, is
 * re-used); one-GPU hosts never load it.
 *
 * ftk_comm_create: rank `rank` of `world` joins the job's communicator on ctx's device.  `id_hex_or_path` is what the
 * ranks have in common: the 256 hex digits of an RCCL unique id (ftk_comm_unique_id on one rank, handed to the others
 * by the host's own means), or a FILE PATH all ranks can reach -- rank 0 creates the id and writes it there (atomic
 * rename), the others wait for it (FTK_COMM_TIMEOUT_S, default 600), rank 0 removes it as soon as the communicator is
 * up (every rank has read it by then).  RCCL's start-up banner is kept off stdout (FTK_COMM_BANNER=1 lets it through).
 * NULL is accepted for world == 1.  A collective runs on the communicator's own HIP stream behind the work the ctx stream
 * holds at the call, so later launches on the ctx stream overlap it.  Buffers may be host or device memory: with a
 * host buffer the call returns when the result is there; with device buffers it returns at once and ftk_comm_join
 * makes the ctx stream wait for the result (no host wait).  Every rank must make the same calls in the same order. */
typedef struct ftk_comm ftk_comm;
int ftk_comm_unique_id(char* hex_out /* [257] */);
int ftk_comm_create(ftk_ctx* ctx, int rank, int world, const char* id_hex_or_path, ftk_comm** out);
int ftk_comm_size(const ftk_comm* comm, int* rank_out, int* world_out);
/* recv[r * n + i] = rank r's send[i]; n equal on all ranks */
int ftk_allgather_i64(ftk_comm* comm, const int64_t* send, int64_t n, int64_t* recv);
/* values[i] = sum over ranks, in place */
int ftk_allreduce_sum_i64(ftk_comm* comm, int64_t* values, int64_t n);
/* point to point (the compressed output sections a rank hands to the writing rank, frag/_multi_wps.py:300-341's
 * parent-side writer): matching send / recv pairs, any size */
int ftk_comm_send(ftk_comm* comm, int dst, const void* data, int64_t n_bytes);
int ftk_comm_recv(ftk_comm* comm, int src, void* data, int64_t n_bytes);
int ftk_comm_join(ftk_comm* comm);
void ftk_comm_destroy(ftk_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* FTK_H */
