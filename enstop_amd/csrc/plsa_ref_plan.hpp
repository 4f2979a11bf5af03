// plsa_ref_plan.hpp -- the arithmetic behind how the reference-arithmetic kernels (plsa_ref_kernels.hpp) are launched, free of
// HIP: lanes and topics per lane from the topic count, the chunk geometry and scratch sizes of the parity-pair chain, the tiles
// of the tiled passes, the three thresholds, and the block plan of a P(z|w,d) budget.  Plain integers in, plain values out: no
// context, no device memory, no environment.  plsa_ref.hpp turns these into launches; tests/ref_plan_host.cpp runs every
// function on a CPU.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace plsa::ref {

// Addends per chunk of the pair chain: a kernel argument (a multiple of 64).  A walk step costs ~115 ns whatever the length, a
// chunk that goes the slow way ~22 ns per addend, and the number of such chunks hardly depends on the corpus (~25 binade
// crossings per topic, most of them shared by the 64 topics of a group: ~600 chunks per walk at k = 64).  With the groups of
// PAIR_R chunks the length is 256 everywhere; walking chunks only (one level) the best length grows with sqrt(nnz) and the host
// takes 1024 from 48 M non-zeros on (config-3 sample, 15 M: 64 / 128 / 256 -> the four kernels together 39.9 / 27.5 / 24.5 ms
// in their first form; config 3 whole, 100 M: the walk 49 ms at 256, 24 ms at 1024, 9 ms with the groups).
constexpr int PAIR_L_SMALL = 256, PAIR_L_LARGE = 1024;
constexpr long long PAIR_L_LARGE_FROM = 48000000;
constexpr int PAIR_SC = 8;            // chunks a wave handles back to back (8 consecutive float64 chunk sums per lane: one 64-B line)
constexpr int PAIR_R = 16;            // chunks per group of the second level (k_ref_pair_compose)

namespace plan {

// Topics per lane (NZ) and lanes per document / column (G) of the passes: topic z = lane + G t, so G * NZ covers kp.
// 0: more than 1024 topics, unsupported.
inline int topics_per_lane(int kp) { int nz = 1; while (64 * nz < kp && nz < 16) nz *= 2; return kp > 1024 ? 0 : nz; }
inline int group_lanes(int kp) { int g = 8; while (g < kp && g < 64) g *= 2; return kp > 1024 ? 0 : g; }

// The pair chain over `span_nnz` addends per topic: chunks of L addends, groups of PAIR_R chunks (the second level), super-chunks
// of PAIR_SC chunks (one wave's turn; the chunk sums are padded to whole super-chunks).  The scratch is sized for `cap_nnz`, the
// longest span the chain is called with (blocks of documents: sized once, no reallocation under the chain of the block before).
// L: 256; with one level 1024 from PAIR_L_LARGE_FROM non-zeros of the corpus on; chunk_knob where it is a multiple of 64 in
// 64..4096 (anything else is ignored).  One level has no group records: their byte counts are 0.
struct ChainGeom { int64_t n_chunks, n_groups, n_super, n_pad; };
struct PairChain { int L; ChainGeom span, cap; int64_t csum_bytes, pairs_bytes, exps_bytes, pairs2_bytes, exps2_bytes; };
inline ChainGeom chain_geom(int64_t nnz, int L) {
    const int64_t chunks = (nnz + L - 1) / L, supers = (chunks + PAIR_SC - 1) / PAIR_SC;
    return {chunks, (chunks + PAIR_R - 1) / PAIR_R, supers, supers * PAIR_SC};
}
inline PairChain pair_chain(int64_t span_nnz, int64_t cap_nnz, int64_t corpus_nnz, int kp, bool two_levels, int chunk_knob) {
    PairChain p;
    p.L = !two_levels && corpus_nnz >= PAIR_L_LARGE_FROM ? PAIR_L_LARGE : PAIR_L_SMALL;
    if (chunk_knob >= 64 && chunk_knob <= 4096 && chunk_knob % 64 == 0) p.L = chunk_knob;
    p.span = chain_geom(span_nnz, p.L);
    p.cap = chain_geom(cap_nnz, p.L);
    p.csum_bytes = 8 * p.cap.n_pad * kp;                          // float64 chunk sums
    p.pairs_bytes = 16 * p.cap.n_chunks * kp;                     // four 32-bit words per record
    p.exps_bytes = 4 * p.cap.n_chunks * kp;
    p.pairs2_bytes = two_levels ? 16 * p.cap.n_groups * kp : 0;
    p.exps2_bytes = two_levels ? 4 * p.cap.n_groups * kp : 0;
    return p;
}

// The tiled E-step and the tiled document pass: a wave's tile is 64 / nz entries (documents), two tiles of kp + 1 floats per
// entry in LDS per workgroup of two waves
inline int64_t e_step_tiles(int64_t nnz, int nz) { return (nnz + 64 / nz - 1) / (64 / nz); }
inline int64_t tile_lds_bytes(int kp, int nz) { return (int64_t)sizeof(float) * 2 * (64 / nz) * (kp + 1); }

// Are the long chains evaluated from parity pairs?  chain_mode: 0 auto, 1 pairs, 2 serial; auto: from 4096 non-zeros, until a
// finished walk was too slow (pairs_off)
inline bool pairs_now(int chain_mode, bool pairs_off, int64_t nnz) { return chain_mode == 1 || (chain_mode == 0 && !pairs_off && nnz >= 4096); }
// a finished walk with more than a quarter of its chunks on the slow way
inline bool walk_too_slow(unsigned long long slow, unsigned long long chunks) { return chunks > 0 && slow * 4 > chunks; }

// The tiled document pass pays from ~300 k documents on (config 3 whole: 22 -> 10 ms); below, the wave tile that holds the few
// longest documents is the pass, and the group kernel walks a long document faster.  knob: -1 unset, 0 / 1 pins either
inline bool row_tiled(int64_t n, int knob) { return knob < 0 ? n >= 300000 : knob != 0; }

// The block plan of a P(z|w,d) budget: whole documents, in order, as many per block as (block_nnz + 64) * kp * 4 <= budget
// allows (the 64 rows are the slack the tiled E-step stores its last tile into).  Blocks are documents [doc[b], doc[b + 1]) =
// entries [ent[b], ent[b + 1]).  indptr is read only where nnz > block_max_rows.
struct BlockPlan {
    enum Status { OK, NO_ROW, DOC_TOO_LONG } status = OK;
    std::vector<long long> doc, ent;
    int64_t largest = 0;                 // non-zeros of the largest block
    int64_t bad_doc = 0, bad_len = 0;    // DOC_TOO_LONG: the document and its non-zeros
};
inline int64_t block_max_rows(int kp, int64_t budget) { return budget / ((int64_t)sizeof(float) * kp) - 64; }
inline BlockPlan block_plan(const int *indptr, int64_t n, int64_t nnz, int kp, int64_t budget) {
    BlockPlan pl;
    const int64_t max_rows = block_max_rows(kp, budget);
    if (max_rows < 1) { pl.status = BlockPlan::NO_ROW; return pl; }
    pl.doc.assign(1, 0); pl.ent.assign(1, 0);
    int64_t b0 = 0;                      // first entry of the block being filled
    if (nnz > max_rows)
        for (int64_t d = 0; d < n; ++d) {
            const int64_t len = (int64_t)indptr[d + 1] - indptr[d];
            if (len > max_rows) { pl.status = BlockPlan::DOC_TOO_LONG; pl.bad_doc = d; pl.bad_len = len; return pl; }
            if ((int64_t)indptr[d + 1] - b0 > max_rows) {       // document d opens the next block
                pl.doc.push_back(d); pl.ent.push_back(indptr[d]);
                pl.largest = std::max(pl.largest, (int64_t)indptr[d] - b0);
                b0 = indptr[d];
            }
        }
    pl.doc.push_back(n); pl.ent.push_back(nnz);
    pl.largest = std::max(pl.largest, nnz - b0);
    return pl;
}

}  // namespace plan
}  // namespace plsa::ref
