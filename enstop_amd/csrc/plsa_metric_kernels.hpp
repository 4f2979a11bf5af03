// plsa_metric_kernels.hpp -- co-document counts of word lists on the resident CSC (include/plsa_hip_metrics.h).
//
// The coherence of a topic (enstop/utils.py:150-203) is a function of integer counts: for the topic's top words, how many
// documents hold a stored entry of both words of a pair, and how many entries of each word are positive.  The reference
// intersects the sorted posting lists of every pair (nw * (nw - 1) / 2 merges per list of nw words); here a list of words
// is one 32-bit mask per document:
//
//   k_metric_mark   walks the posting list of word b of set s once and ORs bit b into mask[s][document]
//   k_metric_count  streams mask[s][0 .. n) and counts, for every pair (i, j), the documents with both bits set
//
// Everything is integer and every combination is an OR or an integer addition: the result does not depend on the order in
// which workgroups run, so it is the same bit pattern in every run.  Bit 31 is in use when nw == 32: every shift is unsigned.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plsa_combine_plan.hpp"

namespace plsa {

using plan::METRIC_BLOCK;
using plan::METRIC_MAX_WORDS;

// grid (pieces of a posting list, nw, sets of the chunk).  words [sets][nw]; mask [sets][n] zeroed by the caller;
// positive [sets][nw] zeroed by the caller: stored entries of the word whose value is > 0.
__global__ __launch_bounds__(METRIC_BLOCK) void k_metric_mark(const int *__restrict__ colptr, const int *__restrict__ csc_row,
                                                              const float *__restrict__ csc_val, const int *__restrict__ words,
                                                              int nw, int64_t n, unsigned *__restrict__ mask,
                                                              unsigned long long *__restrict__ positive) {
    const int b = blockIdx.y;
    const int64_t s = blockIdx.z;
    const int w = words[s * nw + b];
    const int64_t begin = colptr[w], end = colptr[w + 1];
    const unsigned bit = 1u << b;
    unsigned *row_mask = mask + s * n;
    unsigned pos = 0;
    for (int64_t e = begin + (int64_t)blockIdx.x * METRIC_BLOCK + threadIdx.x; e < end; e += (int64_t)gridDim.x * METRIC_BLOCK) {
        atomicOr(row_mask + csc_row[e], bit);      // two words of one set can meet in a document
        pos += csc_val[e] > 0.f;
    }
    for (int o = 32; o > 0; o >>= 1) pos += __shfl_xor(pos, o, 64);
    if ((threadIdx.x & 63) == 0 && pos) atomicAdd(positive + s * nw + b, (unsigned long long)pos);
}

// grid (stretches of the documents, sets of the chunk).  co [sets][nw][nw] zeroed by the caller, both triangles filled.
// A wave takes 64 documents: lane j keeps the 64-document column of bit j (a ballot), and for every bit i some document
// has, popcount(column i & column j) goes to the workgroup's counter (i, j) in LDS.  Waves without a marked document
// skip all of it; that is most of them for tail words.
__global__ __launch_bounds__(METRIC_BLOCK) void k_metric_count(const unsigned *__restrict__ mask, int nw, int64_t n,
                                                               unsigned long long *__restrict__ co) {
    __shared__ unsigned cnt[METRIC_MAX_WORDS * METRIC_MAX_WORDS];
    const int64_t s = blockIdx.y;
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < METRIC_MAX_WORDS * METRIC_MAX_WORDS; i += METRIC_BLOCK) cnt[i] = 0u;
    __syncthreads();
    const unsigned *row_mask = mask + s * n;
    for (int64_t base = (int64_t)blockIdx.x * METRIC_BLOCK; base < n; base += (int64_t)gridDim.x * METRIC_BLOCK) {
        const int64_t d = base + threadIdx.x;
        const unsigned mk = d < n ? row_mask[d] : 0u;
        if (__ballot(mk != 0u) == 0ull) continue;           // wave-uniform
        unsigned long long mine = 0ull;
        for (int j = 0; j < nw; ++j) {
            const unsigned long long col = __ballot((mk >> j) & 1u);
            if (lane == j) mine = col;
        }
        for (int i = 0; i < nw; ++i) {
            const unsigned long long col = __ballot((mk >> i) & 1u);
            if (col == 0ull) continue;                      // wave-uniform
            if (lane < nw) {
                const unsigned both = (unsigned)__popcll(col & mine);
                if (both) atomicAdd(&cnt[i * METRIC_MAX_WORDS + lane], both);
            }
        }
    }
    __syncthreads();
    // a workgroup sees fewer than 2^31 documents: its 32-bit counters cannot wrap; the totals are 64-bit
    for (int idx = threadIdx.x; idx < nw * nw; idx += METRIC_BLOCK) {
        const int i = idx / nw, j = idx - i * nw;
        const unsigned v = cnt[i * METRIC_MAX_WORDS + j];
        if (v) atomicAdd(co + (s * nw + i) * nw + j, (unsigned long long)v);
    }
}

}  // namespace plsa
