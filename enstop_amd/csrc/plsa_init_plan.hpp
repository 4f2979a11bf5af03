// plsa_init_plan.hpp -- the arithmetic behind factor initialisation with the reference's MT19937 stream (plsa_init.hpp: mt_init),
// free of HIP: how many words the stream has, how it is cut into jump-ahead pieces and which jump every level of the tree takes,
// the sizes of the scratch buffers and where the regions of the two carved ones lie, and the grids that are computed on the
// host.  Plain integers in, plain values out: no context, no device memory, no environment.  plsa_init.hpp turns these into
// buffers and launches; tests/init_plan_host.cpp runs every function on a CPU.
#pragma once

#include <algorithm>
#include <cstdint>

namespace plsa::init {

constexpr int MT_N = 624;             // words of an MT19937 block (the generator's key)
constexpr int SEQ_L = 64;             // draws per chunk of the topic marginals = chunks per tile (the kernels' MT_SEQ_L)
constexpr int MARG_WORD = 632;        // mt_fin: 624 key words + the position, padded to an 8-byte boundary; then the marginals
constexpr int MARG_MAX = 1024;        // ... one float64 per topic, k <= 1024

namespace plan {

// The stream of one initialisation: rand(k, m) (draw_topics) then rand(n, k), two 32-bit words per double, continued from
// position pos0 of the current block.  `first` words finish that block; the rest are `total_blocks` whole blocks (the last
// one possibly cut short), which k_mt19937_fill restates on the device.  Once the stream is long enough to pay for the jumps
// (mt_min_blocks) it is cut into n_streams <= mt_streams pieces of per_stream = 2^log2_per blocks; the last piece owns at
// least one block, so the state it leaves is the stream's.  The pieces' start states come from a binary tree of `levels`
// jump levels over streams_p2 (the least power of two >= n_streams) slots: at level l every source q = 2 step(l) i creates
// stream q + step(l), 2^exponent(l) blocks further on.
struct MtStream {
    bool ok;                          // false: pos0 outside [0, 624]
    int64_t v_doubles, n_doubles, n_words, first, total_blocks, per_stream;
    int log2_per, n_streams, streams_p2, levels;
    int exponent(int l) const { return log2_per + (levels - 1 - l); }
    int step(int l) const { return streams_p2 >> (l + 1); }
    int64_t words_bytes() const { return (int64_t)sizeof(uint32_t) * n_words; }
};
inline MtStream mt_stream(int64_t n, int64_t m, int k, bool draw_topics, int64_t pos0, int mt_streams, int64_t mt_min_blocks) {
    MtStream s{};
    s.ok = pos0 >= 0 && pos0 <= MT_N;
    if (!s.ok) return s;
    s.v_doubles = draw_topics ? (int64_t)k * m : 0;
    s.n_doubles = s.v_doubles + n * (int64_t)k;
    s.n_words = 2 * s.n_doubles;
    s.first = std::min<int64_t>(MT_N - pos0, s.n_words);
    s.total_blocks = (s.n_words - s.first + MT_N - 1) / MT_N;
    s.per_stream = std::max<int64_t>(s.total_blocks, 1);
    s.n_streams = 1;
    if (mt_streams > 1 && s.total_blocks >= mt_min_blocks) {
        while (((int64_t)1 << s.log2_per) * mt_streams < s.total_blocks) ++s.log2_per;
        s.per_stream = (int64_t)1 << s.log2_per;
        s.n_streams = (int)((s.total_blocks + s.per_stream - 1) / s.per_stream);
    }
    s.streams_p2 = 1;
    while (s.streams_p2 < s.n_streams) { s.streams_p2 *= 2; ++s.levels; }
    return s;
}

// The scratch of one initialisation, in bytes.  mt_state: one block per slot of the jump tree.  mt_fin: the advanced state
// the generator hands back, the topic marginals behind it (word offset marg_word).  mt_poly: one jump polynomial per level.
// mt_seq (none with the plain chain of adds, `chain`): per topic nch chunks of SEQ_L draws in `tiles` tiles of SEQ_L chunks;
// csum [k][nch] u64 | pairs [k][nch][2] u64 | tsum [k][tiles] f64, in room for [k][nch] | guess [k][nch] int.
struct MtScratch {
    int64_t state_bytes, fin_bytes, poly_bytes;
    int marg_word;
    int nch, tiles;
    int64_t csum_off, pairs_off, tsum_off, guess_off, seq_bytes;
};
inline MtScratch mt_scratch(int k, int64_t m, int streams_p2, int levels, bool chain) {
    MtScratch s{};
    s.state_bytes = (int64_t)sizeof(uint32_t) * MT_N * streams_p2;
    s.marg_word = MARG_WORD;
    s.fin_bytes = (int64_t)sizeof(uint32_t) * (MARG_WORD + 8) + (int64_t)sizeof(double) * MARG_MAX;
    s.poly_bytes = (int64_t)sizeof(uint32_t) * MT_N * levels;
    s.nch = (int)((m + SEQ_L - 1) / SEQ_L);
    s.tiles = (s.nch + SEQ_L - 1) / SEQ_L;
    const int64_t per = (int64_t)k * s.nch;
    s.csum_off = 0;
    s.pairs_off = s.csum_off + 8 * per;
    s.tsum_off = s.pairs_off + 16 * per;
    s.guess_off = s.tsum_off + 8 * per;
    s.seq_bytes = chain ? 0 : s.guess_off + 4 * per;
    return s;
}

// grids computed on the host
struct Grid2 { unsigned x, y; };
inline Grid2 transpose_grid(int64_t m, int kp) { return {(unsigned)((m + 31) / 32), (unsigned)((kp + 31) / 32)}; }   // k_v_to_vt, k_vt_to_v: 32 x 32 tiles
inline unsigned init_u_grid(int64_t n) { return (unsigned)((n + 63) / 64); }                                          // k_mt_init_u: 64 documents per wave
inline Grid2 chunk_grid(const MtScratch &s, int k) { return {(unsigned)s.tiles, (unsigned)k}; }                      // k_mt_chunk_sums, k_mt_chunk_pairs
inline unsigned jump_grid(const MtStream &s, int l) { return (unsigned)(s.streams_p2 / (2 * s.step(l))); }           // k_mt_jump's sources (x; y: its slices)

}  // namespace plan
}  // namespace plsa::init
