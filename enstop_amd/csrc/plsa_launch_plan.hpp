// plsa_launch_plan.hpp -- the arithmetic behind how a fused pass is launched, free of HIP: lane shape from k, item lengths,
// grids, the two-stage switch of the norm, the XCD stretches and their balance controller, the wide-table rule, and what the
// structure builders compute on the host: sort bits, the E-step's piece length, the packing rule.  Plain values in, plain
// values out: no context, no device memory, no environment.  plsa_hip.hip's prepare_row_pass / prepare_col_pass turn these
// into the structures (built by plsa_structures.hpp), scratch and grids of one pass (the fit, the batched members and the
// NMF all launch from those); tests/launch_plan_host.cpp runs every function on a CPU (the line layout of the packed
// streams: tests/line_stream_plan_host.cpp).
#pragma once

#include <algorithm>
#include <cstdint>

namespace plsa {
namespace plan {

// lane decomposition of a k-vector (see plsa_kernels.hpp): the column pass' shape (lpn x ch) and the document pass'
struct LaneShape { int kp, lpn, ch, row_lpn, row_ch; };
inline LaneShape lane_shape(int k, int chunks_per_lane, bool row_shape_8x2) {
    LaneShape s;
    s.kp = (k + 3) / 4 * 4;
    int lpn = 1;
    while (lpn < s.kp / 4 && lpn < 64) lpn *= 2;
    // k >= 128: 8 floats per lane (two float4 chunks) -- fewer reduction/shuffle instructions per
    // cell, each access still covers whole 128-B lines (measured: config 5 document pass -15 %)
    if (lpn >= 32 && lpn * 4 >= s.kp && chunks_per_lane == 2) lpn /= 2;
    s.lpn = lpn;
    s.ch = (s.kp / 4 + lpn - 1) / lpn;
    if (s.ch == 3) s.ch = 4;
    // k = 64: the document pass runs as 8 lanes x 2 chunks (a wave covers 8 documents, one DPP step less per group sum,
    // half the log-likelihood reductions per entry): its LL variant 1.94 -> 1.59 ms, the plain one 1.547 -> 1.530 ms at
    // config 3, while the column pass is 3.5 % SLOWER in that shape (32 items per chunk) and keeps 16 x 1
    s.row_lpn = s.lpn; s.row_ch = s.ch;
    if (row_shape_8x2 && s.lpn == 16 && s.ch == 1 && s.kp == 64) { s.row_lpn = 8; s.row_ch = 2; }
    return s;
}

// Whether the document pass runs over row items (documents cut into pieces), and the piece length.  Row ownership needs
// enough rows to fill the CUs x 32 waves x (64/LPN) groups, and rows of comparable length.
// ritems_mode: -1 auto, 0 never, 1 always; rseg_override: 0 = length by size
struct RowItems { bool use; int seg; };
inline RowItems row_items(int64_t n, int64_t nnz, int cus, int row_lpn, int ritems_mode, int rseg_override) {
    const int64_t group_slots = (int64_t)cus * 32 * (64 / std::max(1, row_lpn));
    const double avg = (double)nnz / (double)std::max<int64_t>(n, 1);
    // the decision is made for 64-entry items (documents averaging more than 128 entries: config 2's 100-entry documents
    // stay whole -- items cost it 15 % in the two-stream schedule); the item LENGTH then follows the size of the corpus:
    // about one item per group slot, a power of two in [16, 64] (20NG shape: 45 entries per slot -> 32; with the final
    // kernels of round 4 row items of 16 / 24 / 32 / 40 / 48 / 64 entries give 9.9 / 10.7 / 11.1 / 11.1 / 10.9 / 10.4 k
    // iterations/s at config 1, profiles/r04_small_corpus_item_lengths.txt)
    const int rseg_decide = rseg_override ? rseg_override : 64;
    RowItems r;
    r.use = ritems_mode == 1 || (ritems_mode < 0 && n < 2 * group_slots && avg > 2.0 * rseg_decide);
    r.seg = rseg_override;
    if (!rseg_override) {
        const int64_t per_slot = nnz / std::max<int64_t>(group_slots, 1);
        r.seg = 16;
        while (r.seg * 2 <= per_slot && r.seg < 64) r.seg *= 2;
    }
    return r;
}

// Entries per column item: a group walks seg/LPN dependent gather batches per item, so small problems want
// short items (enough items to fill the chip: config 1 0.244 -> 0.094 ms at 16) and large
// ones long items (fewer partial rows: 256 measured best at config 3).  seg_override: 0 = by size
inline int col_item_len(int64_t nnz, int cus, int lpn, int seg_override) {
    const int64_t slots = (int64_t)cus * 32 * (64 / std::max(1, lpn));
    // (round 4, final kernels: about 1.25 group slots per item instead of 4 -- config 1 now cuts its columns into
    //  32-entry items, 16 / 32 / 48 / 64 -> 10.5 / 11.1 / 11.0 / 10.9 k iterations/s with 32-entry row items; config 2
    //  64 instead of 32: the same within noise)
    const int64_t want = nnz / std::max<int64_t>(slots + slots / 4, 1);
    int seg = 16;
    // large corpora: with the XCD stretches balanced, SHORTER items win (an item then spans fewer documents
    // and stays inside the band its XCD's L2 holds): config 3 (k = 64) 256 / 128 / 96 / 64 / 48 entries ->
    // 268 / 269 / 271 / 274 / 272 iterations/s before the band-major order, flat from 48 to 128 with it; config 5
    // (k = 128) 256 / 128 / 64 -> 25.3 / 27.6 / 28.6.
    // Items of one length for every column: a chunk's groups (and a wave's) wait for their longest item --
    // long items for the Zipf-head words only (256 entries, the others 64) cost 1.96 -> 3.0 ms at config 3
    const int cap = 64;
    while (seg * 2 <= want && seg < cap) seg *= 2;
    return seg_override ? seg_override : seg;
}

// Documents per band of the column items' visiting order (order_band_knob >= 0: that many): 2 MB of P(z|d) rows from
// k = 64 on -- half an XCD's L2; 8192 documents at config 3, 4096 at config 5.  Measured with the final kernels of round 4,
// config 3: 2048 / 6144 / 8192 / 10240 / 16384 / 32768 documents -> 313 / 318 / 319 / 316 / 303 / 254 iterations/s;
// config 5: 1024 / 3072 / 4096 / 6144 -> 29.0 / 29.4 / 29.9 / 29.8 (round 3 chose 512 KB with 256-entry items).  Narrow
// k-vectors stay at 512 KB (config 2: 8192 documents = 1 MB neutral, 16384 = 2 MB 2 % slower)
inline int order_band(int kp, int order_band_knob) {
    const int band_bytes = (kp >= 64 ? 2048 : 512) << 10;
    return order_band_knob >= 0 ? order_band_knob : std::max(64, band_bytes / (kp > 0 ? kp * 4 : 256));
}

// Bits a radix sort has to look at for keys 0 .. count - 1: the smallest b >= 1 with 2^b >= count.  One too few sorts wrongly,
// and silently.
inline int sort_bits(int64_t count) {
    int bits = 1;
    while (((int64_t)1 << bits) < count) ++bits;
    return bits;
}

// Key of the column items' visiting order (k_item_fill): band index << len_bits | inverted column length.  A column holds at
// most n entries, so len_bits are the bits of 0 .. n; above them the bits of the n / band + 1 bands (band <= 0: the key is
// the item's first document, which fits len_bits too).  len_bits goes to k_item_fill, key_bits to the sort.
struct OrderKey { int len_bits, key_bits; };
inline OrderKey order_key(int64_t n, int band) {
    OrderKey k;
    k.len_bits = sort_bits(n + 1);
    k.key_bits = k.len_bits + (band > 0 ? sort_bits(n / band + 1) : 0);
    return k;
}

// Entries per piece of the document-owned E-step (eseg_override >= 0: that many, 0 = whole documents).  Measured optimum 64
// entries at k = 64 (48: 4.86, 64: 4.61, 80: 5.03, whole documents: 5.36 ms at config 3; config 5, k = 128: flat within 1 %
// from 32 to 128), 8 entries at k = 32 (0.224 against 0.234-0.238 ms for 16-40 and 0.316 ms for whole documents at config 2)
inline int e_item_len(int lpn, int eseg_override) {
    return eseg_override >= 0 ? eseg_override : (lpn >= 16 ? 64 : (lpn == 8 ? 8 : 16));
}

// A pass runs on its packed entry stream (plsa_kernels.hpp: Packed) when there are entries, its `id_range` ids fit the word's
// 24 bits and at most 1/16 of the entries escaped to the float array.  With escaped = 0: whether packing is worth trying.
constexpr int64_t PACK_ID_RANGE = (int64_t)1 << 24;
inline bool packed_ok(int64_t nnz, int64_t id_range, uint64_t escaped) {
    return nnz > 0 && id_range <= PACK_ID_RANGE && escaped * 16 <= (uint64_t)nnz;
}

// Line layout of a packed entry stream.  The stream's OWNERS (documents, row items, column items) each start on a BLOCK of
// 4 * lpn words, lpn = the lane count of the pass that reads the stream; pad words are 0.  Lane li of a group loads ONE
// 16-byte vector per block, the words 4 * li .. 4 * li + 3, and batch c (0..3) of the block consumes component c: the word
// at 4 * li + c holds entry c * lpn + li of the block -- the entry that lane handles in that batch with one word per load.
// From 8 lanes on a group's load is one or two whole 128-byte lines.
//   documents: padded to whole blocks, one array of n + 1 block offsets (the start of document d in BLOCKS)
//   items (row items, column items): one slot of line_slot(seg, lpn) words per item, at slot index = item id
// Word offsets inside the kernels are 32-bit: a stream of more than LINE_MAX_WORDS words is not built (its pass runs on the
// two arrays).
constexpr int64_t LINE_MAX_WORDS = ((int64_t)1 << 31) - 1;
constexpr int line_block(int lpn) { return 4 * lpn; }
constexpr int64_t line_blocks(int64_t len, int lpn) { return (len + line_block(lpn) - 1) / line_block(lpn); }
constexpr int line_slot(int seg, int lpn) { return (int)(line_blocks(seg, lpn) * line_block(lpn)); }
// entry `rel` of an owner (0 = its first) <-> (block of the owner, lane, component) <-> word offset from the owner's start
struct LinePos { int64_t block; int lane, comp; };
constexpr LinePos line_pos(int64_t rel, int lpn) {
    return LinePos{rel / line_block(lpn), (int)(rel % line_block(lpn) % lpn), (int)(rel % line_block(lpn) / lpn)};
}
constexpr int64_t line_rel(const LinePos &p, int lpn) { return p.block * line_block(lpn) + (int64_t)p.comp * lpn + p.lane; }
constexpr int64_t line_word(const LinePos &p, int lpn) { return p.block * line_block(lpn) + 4 * (int64_t)p.lane + p.comp; }
constexpr LinePos line_pos_of_word(int64_t word, int lpn) {
    return LinePos{word / line_block(lpn), (int)(word % line_block(lpn) / 4), (int)(word % 4)};
}
// the most words a document stream can take (every document wastes less than a block), known before the offsets are summed;
// the words of an item stream; whether a stream of that many words is built
constexpr int64_t line_doc_words_bound(int64_t nnz, int64_t n, int lpn) { return nnz + n * (line_block(lpn) - 1); }
constexpr int64_t line_item_words(int64_t n_items, int seg, int lpn) { return n_items * line_slot(seg, lpn); }
constexpr bool line_stream_fits(int64_t words) { return words <= LINE_MAX_WORDS; }

inline int grid_for(int64_t work, int per_block, int cap) {
    int64_t need = (work + per_block - 1) / per_block;
    if (need < 1) need = 1;
    return (int)std::min<int64_t>(need, cap);
}

// Document pass: a group of row_lpn lanes per row item (`items`) or whole document; reduce_grid is the grid of the per-document
// sum of the item partials -- and of any other whole-document walk in the document pass' lane shape.
// xcd_rows (PLSA_ROW_XCD, experiment): one trip, grid a multiple of 8, XCD x takes the x-th eighth of the visiting list
struct RowPass { int grid, reduce_grid; };
inline RowPass row_pass(int64_t n, int64_t n_ritems, bool items, int row_lpn, int grid_cap, bool xcd_rows) {
    const int gpb = 256 / row_lpn;
    RowPass r;
    r.grid = grid_for(items ? n_ritems : n, gpb, grid_cap);
    if (xcd_rows) r.grid = (int)(((n + gpb - 1) / gpb + 7) / 8 * 8);
    r.reduce_grid = grid_for(n, gpb, grid_cap);
    return r;
}

// Column pass: chunks of 256 / lpn items, one float64 sum row per chunk; the per-column sums take one group per column plus
// one workgroup per heavy column; norm_pwz from the chunk rows in one stage, or -- many chunks (large corpora) -- through
// norm_blocks workgroups first (0: one stage)
struct ColPass { int n_chunks, reduce_grid, norm_blocks; };
inline ColPass col_pass(int64_t n_items, int64_t m, int lpn, int n_heavy, int grid_cap) {
    const int gpb = 256 / lpn;
    ColPass p;
    p.n_chunks = (int)((n_items + gpb - 1) / gpb);
    p.reduce_grid = grid_for(m, gpb, grid_cap) + n_heavy;
    p.norm_blocks = p.n_chunks > 2048 ? std::max(64, std::min(1024, p.n_chunks / 64)) : 0;
    return p;
}

// Whether the column pass walks its chunks in per-XCD stretches.  A P(z|d) table that fits every XCD's L2 (20NG shape:
// 1.5 MB) has no band to keep local: plain grid-stride over the list, balanced by the dispatcher (config 1: 8990 -> 9490
// iterations/s)
inline bool xcd_split(bool xcd_split_knob, int n_chunks, int64_t n, int kp) {
    const bool u_fits_l2 = (double)n * kp * 4.0 <= 2.0 * 1024 * 1024;
    return xcd_split_knob && n_chunks >= 64 && !u_fits_l2;
}

// chunk boundaries of the column pass' XCD stretches from the fractions frac[0..8]
inline void balance_lo(const double frac[9], int n_chunks, int lo[9]) {
    lo[0] = 0;
    for (int x = 1; x < 8; ++x) {
        const int v = (int)(frac[x] * n_chunks + 0.5);
        lo[x] = std::min(n_chunks, std::max(lo[x - 1], v));
    }
    lo[8] = n_chunks;
}

// Grid of the column pass: ONE chunk per workgroup (the dispatcher then walks each XCD's stretch strictly in list
// order; with a capped grid a workgroup's later chunks lay a whole grid ahead of the window its XCD was working on:
// 32 k / 64 k / 128 k workgroups at config 3 -> 1.86 / 1.83 / 1.79 ms).  With the XCD split every XCD gets grid / 8
// workgroups, so the grid is eight times the longest stretch; the others' surplus workgroups exit at once.
inline int col_grid(const int lo[9], int n_chunks, bool split) {
    int64_t g = n_chunks;
    if (split) {
        int longest = 1;
        for (int x = 0; x < 8; ++x) longest = std::max(longest, lo[x + 1] - lo[x]);
        g = 8 * (int64_t)longest;
    }
    return (int)std::max<int64_t>(1, std::min<int64_t>(g, (int64_t)1 << 22));
}

// The measured balance of the XCD stretches (plsa_structures.hpp: ensure_balance).  A timed launch of `grid` workgroups leaves
// grid + 1 stamps of the 100 MHz wall clock: workgroup b's end in stamps[b], the start in stamps[grid].  Workgroup b runs on
// XCD b % 8, an XCD's time is its last workgroup's end after the earliest stamp of the launch (a zero is a stamp never
// written: not a start), in us, at least 1; spread = (slowest - fastest) / mean.
struct XcdTimes { double us[8], spread; };
inline XcdTimes xcd_times(const unsigned long long *stamps, int grid) {
    unsigned long long t0 = ~0ull, last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b <= grid; ++b) if (stamps[b]) t0 = std::min(t0, stamps[b]);
    for (int b = 0; b < grid; ++b) last[b & 7] = std::max(last[b & 7], stamps[b]);
    XcdTimes t;
    double mean = 0.0, lo_t = 1e300, hi_t = 0.0;
    for (int x = 0; x < 8; ++x) {
        t.us[x] = std::max(1.0, (double)(last[x] - t0) / 100.0);
        mean += t.us[x] / 8.0; lo_t = std::min(lo_t, t.us[x]); hi_t = std::max(hi_t, t.us[x]);
    }
    t.spread = (hi_t - lo_t) / mean;
    return t;
}

// The next fractions from the current ones and the XCD times they gave: every stretch resized by (mean time / own time),
// damped by 0.8, never below 1e-6 of the list, and the eight renormalised to the whole list.  next may be frac itself.
inline void balance_step(const double frac[9], const double us[8], double next[9]) {
    double mean = 0.0, size[8], tot = 0.0;
    for (int x = 0; x < 8; ++x) mean += us[x] / 8.0;
    for (int x = 0; x < 8; ++x) {
        size[x] = std::max(1e-6, (frac[x + 1] - frac[x]) * (1.0 + 0.8 * (mean / us[x] - 1.0)));
        tot += size[x];
    }
    double acc = 0.0;
    next[0] = frac[0];
    for (int x = 0; x < 8; ++x) { acc += size[x]; next[x + 1] = acc / tot; }
    next[8] = 1.0;
}

// The two fused passes gather rows of a factor table by index with 32-bit byte offsets (plsa_kernels.hpp: gather_row).
// A table of 4 GB or more (rows * kp * 4 >= 2^32: e.g. 20 M documents at k = 64) takes the WIDE instantiations instead:
// 64-bit row addresses, run-time kp -- same arithmetic, same results.  `force` selects them for any size (tests).
inline bool table_is_wide(int64_t rows, int kp, bool force) { return force || (double)rows * kp * 4.0 >= 4294967296.0; }

}  // namespace plan
}  // namespace plsa
