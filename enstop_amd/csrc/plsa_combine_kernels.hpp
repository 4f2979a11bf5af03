// plsa_combine_kernels.hpp -- the dense kernels of the topic combination (host side: plsa_combine.hpp): all-pairs Hellinger and
// all-pairs KL over the stacked topics, and the cluster representatives.  Tile origins and slice bounds come from
// plsa_combine_plan.hpp.  The co-document counts live in plsa_metric_kernels.hpp, the embedding in plsa_embed_kernels.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "plsa_combine_plan.hpp"

namespace plsa {

typedef long long i64;             // as in plsa_kernels.hpp
using plan::HELL_KSTEP;
using plan::HELL_TILE;
static_assert(plan::COMBINE_BLOCK == 256, "the kernels below are written for 256 threads: 16 x 16 in the gram kernels, 256-entry reductions");

// ------------------------------------------------------------------------------------------------
// All-pairs Hellinger distance between topic vectors (the precomputed metric of the ensemble's topic
// combination, enstop/enstop_.py:258-266):  D_ij = sqrt(1 - sum_w sqrt(p_i[w] p_j[w]) / sqrt(|p_i|_1 |p_j|_1)).
//   k_hell_prepare : per topic, |p|_1 in float64 and sqrt() in place
//   k_hell_gram    : 64 x 64 tile of R R^T over one slice of the vocabulary (upper-triangular tiles
//                    only); float32 products, flushed into float64 every 256 words
//   k_hell_finish  : adds the slice partials in fixed order, forms the distance
// A plain dense contraction on the vector ALUs: t = n_runs * k is a few hundred, the whole job is tens
// of GFLOP -- milliseconds -- so no matrix-core path is warranted.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_hell_prepare(float *__restrict__ R, int t, i64 m, double *__restrict__ l1) {
    __shared__ double red[256];
    const int i = blockIdx.x;
    float *row = R + (i64)i * m;
    double s = 0.0;
    for (i64 w = threadIdx.x; w < m; w += 256) {
        const float p = row[w];
        s += (double)p;
        row[w] = sqrtf(fmaxf(p, 0.f));
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) l1[i] = red[0];
}

__global__ __launch_bounds__(256) void k_hell_gram(const float *__restrict__ R, int t, i64 m, i64 slice,
                                                   double *__restrict__ partial /*[slices][t][t]*/) {
    __shared__ float sa[HELL_KSTEP][HELL_TILE + 1], sb[HELL_KSTEP][HELL_TILE + 1];
    const plan::PairTile tile = plan::tri_tile(blockIdx.x, plan::pair_nt(t));       // i <= j: the upper triangle
    const int bi = tile.i * HELL_TILE, bj = tile.j * HELL_TILE;
    const i64 w0 = plan::slice_begin(blockIdx.y, slice), w1 = plan::slice_end(blockIdx.y, slice, m);
    const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;          // 16 x 16 threads, 4 x 4 outputs each
    double acc[4][4];
    float facc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) { acc[a][b] = 0.0; facc[a][b] = 0.f; }
    int since_flush = 0;
    for (i64 w = w0; w < w1; w += HELL_KSTEP) {
        // stage 64 rows x 32 words of both operands (each row segment is 128 contiguous bytes)
        for (int e = threadIdx.x; e < HELL_TILE * HELL_KSTEP; e += 256) {
            const int r = e / HELL_KSTEP, kk = e % HELL_KSTEP;
            const i64 ww = w + kk;
            sa[kk][r] = (bi + r < t && ww < w1) ? R[(i64)(bi + r) * m + ww] : 0.f;
            sb[kk][r] = (bj + r < t && ww < w1) ? R[(i64)(bj + r) * m + ww] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < HELL_KSTEP; ++kk) {
            float av[4], bv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { av[a] = sa[kk][ty * 4 + a]; bv[a] = sb[kk][tx * 4 + a]; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) facc[a][b] += av[a] * bv[b];
        }
        __syncthreads();
        since_flush += HELL_KSTEP;
        if (since_flush >= 256) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) { acc[a][b] += (double)facc[a][b]; facc[a][b] = 0.f; }
            since_flush = 0;
        }
    }
    double *out = partial + (i64)blockIdx.y * t * t;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = bi + ty * 4 + a, j = bj + tx * 4 + b;
            if (i < t && j < t) out[(i64)i * t + j] = acc[a][b] + (double)facc[a][b];
        }
}

__global__ __launch_bounds__(256) void k_hell_finish(const double *__restrict__ partial, int slices, int t,
                                                     const double *__restrict__ l1, double *__restrict__ D) {
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e >= (i64)t * t) return;
    const int i = (int)(e / t), j = (int)(e % t);
    const int a = min(i, j), b = max(i, j);                // only the upper triangle was computed
    double g = 0.0;
    for (int s = 0; s < slices; ++s) g += partial[(i64)s * t * t + (i64)a * t + b];
    const double li = l1[i], lj = l1[j];
    double d;
    if (i == j || (li == 0.0 && lj == 0.0)) d = 0.0;
    else if (li == 0.0 || lj == 0.0) d = 1.0;
    else d = sqrt(fmax(1.0 - g / sqrt(li * lj), 0.0));
    D[e] = d;
}

// ------------------------------------------------------------------------------------------------
// All-pairs KL divergence of the stacked ensemble topics, enstop/enstop_.py:234-253:
//   D[i, j] = sum over words with p_i > 0 and p_j > 0 of  p_i * (log2 p_i - log2 p_j)      (bits)
// Not symmetric: every (i, j) tile is computed.  Same staging as k_hell_gram; log2 (v_log_f32 IS a
// base-2 logarithm) is evaluated while a tile is staged into LDS, the pair term is formed directly
// (no cancellation between two large dot products), float partial sums are flushed into float64
// every 256 words.
// v_log_f32 does not take subnormal inputs (it returns -inf for 0 < p < 2^-126, and one such entry makes
// a whole D[i, j] non-finite); topic entries that small are reachable (e_step_thresh = 1e-32 over a
// norm_pwz of 1e5 ... 1e7), so they are scaled into the normal range first.  Normal inputs take the
// bare instruction as before: their bits do not change.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float kl_log2(float p) {
    const bool tiny = p < 1.17549435e-38f;                       // FLT_MIN = 2^-126
    const float l = __log2f(tiny ? p * 4294967296.f : p);        // 2^32: exact
    return tiny ? l - 32.f : l;
}

__global__ __launch_bounds__(256) void k_kl_gram(const float *__restrict__ T, int t, i64 m, i64 slice,
                                                 double *__restrict__ partial /*[slices][t][t]*/) {
    __shared__ float sp[HELL_KSTEP][HELL_TILE + 1], sl[HELL_KSTEP][HELL_TILE + 1];   // row side: p_i, log2 p_i
    __shared__ float sq[HELL_KSTEP][HELL_TILE + 1], sm[HELL_KSTEP][HELL_TILE + 1];   // column side: log2 p_j, [p_j > 0]
    const plan::PairTile tile = plan::square_tile(blockIdx.x, plan::pair_nt(t));
    const int bi = tile.i * HELL_TILE, bj = tile.j * HELL_TILE;
    const i64 w0 = plan::slice_begin(blockIdx.y, slice), w1 = plan::slice_end(blockIdx.y, slice, m);
    const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
    double acc[4][4];
    float facc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) { acc[a][b] = 0.0; facc[a][b] = 0.f; }
    int since_flush = 0;
    for (i64 w = w0; w < w1; w += HELL_KSTEP) {
        for (int e = threadIdx.x; e < HELL_TILE * HELL_KSTEP; e += 256) {
            const int r = e / HELL_KSTEP, kk = e % HELL_KSTEP;
            const i64 ww = w + kk;
            const float pi = (bi + r < t && ww < w1) ? T[(i64)(bi + r) * m + ww] : 0.f;
            const float pj = (bj + r < t && ww < w1) ? T[(i64)(bj + r) * m + ww] : 0.f;
            sp[kk][r] = pi > 0.f ? pi : 0.f;
            sl[kk][r] = pi > 0.f ? kl_log2(pi) : 0.f;
            sq[kk][r] = pj > 0.f ? kl_log2(pj) : 0.f;
            sm[kk][r] = pj > 0.f ? 1.f : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < HELL_KSTEP; ++kk) {
            float pa[4], la[4], lb[4], mb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                pa[a] = sp[kk][ty * 4 + a]; la[a] = sl[kk][ty * 4 + a];
                lb[a] = sq[kk][tx * 4 + a]; mb[a] = sm[kk][tx * 4 + a];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) facc[a][b] += (pa[a] * mb[b]) * (la[a] - lb[b]);
        }
        __syncthreads();
        since_flush += HELL_KSTEP;
        if (since_flush >= 256) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) { acc[a][b] += (double)facc[a][b]; facc[a][b] = 0.f; }
            since_flush = 0;
        }
    }
    double *out = partial + (i64)blockIdx.y * t * t;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = bi + ty * 4 + a, j = bj + tx * 4 + b;
            if (i < t && j < t) out[(i64)i * t + j] = acc[a][b] + (double)facc[a][b];
        }
}

__global__ __launch_bounds__(256) void k_sum_slices(const double *__restrict__ partial, int slices, i64 count,
                                                    double *__restrict__ D) {
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    double g = 0.0;
    for (int s = 0; s < slices; ++s) g += partial[(i64)s * count + e];
    D[e] = g;
}

// ------------------------------------------------------------------------------------------------
// Cluster representatives of the topic combination, enstop/enstop_.py:299-308, 340-345, 385-393:
//   rep[c] = ( sum_{i in c} w_i sqrt(p_i) / sum_{i in c} w_i )^2, then L1-normalised
// (w == nullptr: plain mean).  members[] lists the topic rows of each cluster back to back
// (first[c] .. first[c+1]); rows are added in member order (fixed order: reproducible).
//   k_rep_accumulate : one thread per (cluster, word); per-block float64 partial of the row sum
//   k_rep_normalise  : fixed-order sum of the block partials, division, float32 output
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rep_accumulate(const float *__restrict__ T, i64 m,
                                                        const int *__restrict__ first, const int *__restrict__ members,
                                                        const double *__restrict__ w, double *__restrict__ rep /*[c][m]*/,
                                                        double *__restrict__ block_sums /*[c][gridDim.x]*/) {
    const int c = blockIdx.y;
    const int i0 = first[c], i1 = first[c + 1];
    const i64 word = (i64)blockIdx.x * 256 + threadIdx.x;
    double v = 0.0;
    if (word < m) {
        double num = 0.0, den = 0.0;
        for (int i = i0; i < i1; ++i) {
            const double wi = w ? w[members[i]] : 1.0;
            num += wi * (double)sqrtf(T[(i64)members[i] * m + word]);
            den += wi;
        }
        const double mean = den > 0.0 ? num / den : 0.0;
        v = mean * mean;
        rep[(i64)c * m + word] = v;
    }
    __shared__ double red[256];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) block_sums[(i64)c * gridDim.x + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void k_rep_normalise(const double *__restrict__ rep, i64 m,
                                                       const double *__restrict__ block_sums, int n_blocks,
                                                       float *__restrict__ out /*[c][m]*/) {
    const int c = blockIdx.y;
    __shared__ double total;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < n_blocks; ++b) s += block_sums[(i64)c * n_blocks + b];
        total = s;
    }
    __syncthreads();
    const i64 word = (i64)blockIdx.x * 256 + threadIdx.x;
    if (word < m) out[(i64)c * m + word] = (float)(rep[(i64)c * m + word] / total);
}

}  // namespace plsa
