// The write direction: fragment columns -> text rows -> DEFLATE -> BGZF members, on the device (ftk_fragtext.hip).
// The inverse of ftk_textparse.hip (rows -> columns) and ftk_inflate.hip (BGZF -> text).
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime_api.h>

#include "ftk_inflate.h"

namespace ftk {

constexpr int kBgzfData = 0xFF00;  // text bytes per BGZF member (htslib's block size)
constexpr int kBgzfSlot = 65536;   // bytes of a member's slot before compaction: 2 bytes of padding, then the member
constexpr int kRowsPerBlock = 1024;  // rows per workgroup of the formatter (256 threads x 4 rows)
constexpr int kDeflateLanes = 8192;  // BGZF blocks compressed side by side (one lane each)
constexpr int kDeflateHash = 4096;   // hash table entries per lane (uint32)
constexpr int kDeflateTokens = 8192; // LZ77 tokens per DEFLATE block (uint32 each)
// Intervals of ONE region mask a formatter workgroup stages in LDS (starts and ends: 8 bytes each).  Two masks take
// 16 KiB per workgroup, so the eight workgroups of 256 threads that fill a CU's wave slots fit its 160 KiB together.
constexpr int kMaskLdsIntervals = 1024;

enum : int { kLayoutFrag = 0, kLayoutBed6 = 1, kLayoutBed3 = 2 };

struct RowParams {
    int32_t mapq_min, min_len, max_len;  // keep rule (FTK_LEN_OPEN = no bound)
    int32_t layout;
    int32_t name_len;
    char name[256];
};

// What a range of rows adds up to; combine(a, b) with a in front of b is associative, so the per-thread, per-workgroup
// and device-wide prefix of it place every row (text offset, bin run, first row of a 16 kb window) without atomics.
struct RowAgg {
    unsigned long long bytes;  // text bytes of the kept rows
    uint32_t rows;             // kept rows
    uint32_t runs;             // kept rows whose bin differs from the kept row in front of them (within the range)
    int32_t first_bin;         // bin of the first / last kept row; -1: no kept row
    int32_t last_bin;
    int32_t max_win;           // last 16 kb window a kept row reaches; -1: none
    int32_t pad_;
};

// Region masks of one contig on the device: sorted, disjoint intervals, both arrays padded to a multiple of four
// entries (starts with INT32_MAX, ends with 0) and 16-byte aligned.  n_wl < 0: no whitelist, n_wl == 0: a whitelist
// that holds nothing; n_bl <= 0: no blacklist.  policy: FTK_POLICY_MIDPOINT / FTK_POLICY_ANY.
struct MaskView {
    const int32_t *wl_start, *wl_end;
    int32_t n_wl;
    const int32_t *bl_start, *bl_end;
    int32_t n_bl;
    int32_t policy;
};
inline size_t mask_words(int64_t n) { return (size_t)((n + 63) / 64); }
// keep_bits[i >> 6] bit (i & 63) = row i is in the whitelist (or there is none) and not in the blacklist; the unused
// bits of the last word are zero.  The MAPQ / length rule is not looked at here.
void mask_keep(hipStream_t s, const int32_t* start, const int32_t* end, int64_t n, const MaskView& m,
               unsigned long long* keep_bits);

size_t format_agg_bytes(int64_t n);  // scratch for the two RowAgg arrays + the total
// pass 1 (row lengths, per-workgroup sums) + the device-wide scan: block_prefix[b] = everything in front of workgroup b
void format_pass1(hipStream_t s, const int32_t* start, const int32_t* end, const uint8_t* mapq, int64_t n,
                  const RowParams& p, RowAgg* block_agg, RowAgg* block_prefix, RowAgg* total,
                  const unsigned long long* keep_bits = nullptr);
// pass 2: the bytes, the bin runs (run r: bin run_bin[r], first text byte run_off[r]) and, for every 16 kb window, the
// text offset of the first kept row that overlaps it (lin[w]; preset to all-ones by the caller).
// keep_bits (both passes; nullptr = none): mask_keep's bitmap, ANDed into the keep rule
void format_pass2(hipStream_t s, const int32_t* start, const int32_t* end, const uint8_t* mapq, const uint8_t* strand,
                  int64_t n, const RowParams& p, const RowAgg* block_prefix, uint8_t* text, int32_t* run_bin,
                  uint32_t* run_off, uint32_t* lin, int32_t n_lin, const unsigned long long* keep_bits = nullptr);

// BGZF members of `n` bytes of device text (n < 2^32 - 65536): scratch sizes and the launch sequence.  d_out receives
// the members back to back; d_offs[k] = offset of member k in d_out, d_offs[n_blocks] = their total size.
struct DeflateScratch {
    uint8_t* slots;     // n_blocks * kBgzfSlot
    uint32_t* sizes;    // n_blocks
    uint32_t* crc;      // n_blocks
    InflateBlock* tab;  // n_blocks (the CRC kernel's view of the text)
    uint32_t* hash;     // lanes * kDeflateHash
    uint32_t* tokens;   // lanes * kDeflateTokens
    unsigned long long* offs;  // n_blocks + 1
    uint8_t* out;       // n_blocks * (kBgzfData + 31) at most
};
inline int64_t bgzf_blocks(int64_t n) { return (n + kBgzfData - 1) / kBgzfData; }
inline int deflate_lanes(int64_t n_blocks) { return (int)(n_blocks < kDeflateLanes ? n_blocks : kDeflateLanes); }
void deflate_members(hipStream_t s, const uint8_t* text, int64_t n, const DeflateScratch& sc);
void deflate_compact(hipStream_t s, int64_t n_blocks, const DeflateScratch& sc);

// CRC-32 of n_blocks byte ranges of `data` (tab[k].out_off / out_len), ftk_inflate.hip's kernel
void crc_launch(hipStream_t s, const InflateBlock* d_tab, int n_blocks, const uint8_t* data, uint32_t* d_crc);

}  // namespace ftk
