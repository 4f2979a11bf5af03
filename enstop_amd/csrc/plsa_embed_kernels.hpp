// plsa_embed_kernels.hpp -- the embedding stage of topic_combination="hellinger_umap" (include/plsa_hip_embed.h;
// enstop_.py:354-414 hands the stacked topics to umap.UMAP(metric="hellinger")).
//
// UMAP as published (McInnes, Healy, Melville 2018) at the size of this stage, a few hundred to a few thousand points
// whose exact distance matrix plsa_all_pairs_hellinger has already produced:
//
//   k_knn_membership  per row of D: the n_neighbors nearest entries by (value, index), the bandwidths rho and sigma, and
//                     the directed membership strengths -- one wave per row, one launch
//   k_layout_lds      all epochs of the force layout in ONE launch: one workgroup, both position buffers in LDS
//   k_layout_epoch    one epoch of the same layout over two global buffers, for layouts the LDS cannot hold
//
// The layout is synchronous: in an epoch every vertex reads the positions the epoch started with, sums its own gradient
// terms in a fixed order and writes its own new position to the other buffer.  A vertex is owned by one thread, so there
// are no float atomics and a run is a function of its inputs and its seed.  Both layout kernels call layout_vertex, whose
// arithmetic is written out operation by operation (no contraction): the two give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plsa_combine_plan.hpp"

namespace plsa {

constexpr int EMBED_MAX_NEIGHBORS = 1024;          // the selected neighbours of a row are staged in LDS
constexpr int EMBED_MAX_DIM = 8;
constexpr int LAYOUT_LDS_BLOCK = 1024;
using plan::LAYOUT_EPOCH_BLOCK;
using plan::LAYOUT_LDS_BYTES;

// ---------------------------------------------------------------------------------------------------------------------
// neighbours, bandwidths, membership strengths

__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);     // every lane ends with the same bits
    return v;
}

// grid (t), block (64): the wave of row `row`.  D [t][t] float64.  idx, dist, member [t][k]; rho, sigma, row_sum [t];
// done: one counter, zeroed by the caller.  The rows whose neighbours are all at distance 0 take their sigma floor from the
// mean over ALL neighbour distances, which no row knows alone: every wave leaves the sum of its row in row_sum, and the
// wave that arrives last (an integer ticket) adds the sums in index order and raises the sigma of those rows.
__global__ __launch_bounds__(64) void k_knn_membership(const double *__restrict__ D, int t, int k, int *__restrict__ idx,
                                                       float *__restrict__ dist, float *__restrict__ rho,
                                                       float *__restrict__ sigma, float *__restrict__ member,
                                                       float *__restrict__ row_sum, unsigned *__restrict__ done) {
    __shared__ float s_dist[EMBED_MAX_NEIGHBORS];
    __shared__ int s_idx[EMBED_MAX_NEIGHBORS];
    const int row = blockIdx.x, lane = threadIdx.x;
    const double *d_row = D + (int64_t)row * t;
    // step 1: k times, the smallest (value, index) above the one selected before -- a stable ascending sort's first k
    double last_v = -INFINITY;
    int last_c = -1;
    for (int j = 0; j < k; ++j) {
        double best_v = INFINITY;
        int best_c = 0x7fffffff;
        for (int c = lane; c < t; c += 64) {
            const double v = d_row[c];
            const bool after = v > last_v || (v == last_v && c > last_c);
            if (after && (v < best_v || (v == best_v && c < best_c))) { best_v = v; best_c = c; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(best_v, o, 64);
            const int oc = __shfl_xor(best_c, o, 64);
            if (ov < best_v || (ov == best_v && oc < best_c)) { best_v = ov; best_c = oc; }
        }
        last_v = best_v;
        last_c = best_c;
        if (lane == 0) { s_dist[j] = (float)best_v; s_idx[j] = best_c; }
    }
    __syncthreads();
    // step 2 in float32: rho, the bisection for sigma, the floor
    float r = INFINITY, total = 0.f;
    for (int j = lane; j < k; j += 64) {
        const float d = s_dist[j];
        total += d;
        if (d > 0.f && d < r) r = d;
    }
    for (int o = 32; o > 0; o >>= 1) r = fminf(r, __shfl_xor(r, o, 64));
    total = wave_sum(total);
    if (r == INFINITY) r = 0.f;
    const float target = log2f((float)k);
    float lo = 0.f, hi = INFINITY, mid = 1.f;
    for (int n = 0; n < 64; ++n) {
        float psum = 0.f;
        for (int j = 1 + lane; j < k; j += 64) {
            const float d = s_dist[j] - r;
            psum += d > 0.f ? expf(-(d / mid)) : 1.f;
        }
        psum = wave_sum(psum);
        if (fabsf(psum - target) < 1e-5f) break;       // wave-uniform: every lane holds the same sum
        if (psum > target) {
            hi = mid;
            mid = (lo + hi) * 0.5f;
        } else {
            lo = mid;
            mid = hi == INFINITY ? mid * 2.f : (lo + hi) * 0.5f;
        }
    }
    if (r > 0.f) mid = fmaxf(mid, 1e-3f * (total / (float)k));
    // step 3
    for (int j = lane; j < k; j += 64) {
        const float d = s_dist[j] - r;
        const int c = s_idx[j];
        const int64_t o = (int64_t)row * k + j;
        idx[o] = c;
        dist[o] = s_dist[j];
        member[o] = c == row ? 0.f : (d > 0.f ? expf(-(d / mid)) : 1.f);
    }
    if (lane == 0) { rho[row] = r; sigma[row] = mid; row_sum[row] = total; }
    // the rows without a positive neighbour distance (membership 1 whatever sigma is): floor from the global mean
    __threadfence();
    __syncthreads();
    __shared__ unsigned s_ticket;
    if (lane == 0) s_ticket = atomicAdd(done, 1u);
    __syncthreads();
    if (s_ticket != gridDim.x - 1) return;
    __threadfence();
    float all = 0.f;
    for (int base = 0; base < t; base += 64) {          // row sums in index order, 64 at a time
        const int i = base + lane;
        all += wave_sum(i < t ? row_sum[i] : 0.f);
    }
    const float floor_all = 1e-3f * (all / ((float)t * (float)k));
    for (int i = lane; i < t; i += 64)
        if (rho[i] == 0.f) {
            const float s = sigma[i];
            if (s < floor_all) sigma[i] = floor_all;
        }
}

// ---------------------------------------------------------------------------------------------------------------------
// layout

__host__ __device__ inline uint64_t embed_mix64(uint64_t x) {     // the finaliser of splitmix64 (Steele, Lea, Flood 2014)
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
constexpr uint64_t EMBED_GOLDEN = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ float clip4(float v) { return fminf(fmaxf(v, -4.f), 4.f); }

struct LayoutGraph {
    const int *indptr;      // [t + 1]
    const int *indices;     // [nnz]
    const float *eps;       // [nnz] epochs per sample = max(W) / w
    float2 *state;          // [nnz] (epoch of the next sample, epoch of the next negative sample), owned by the edge's row
    int t;
    int n_epochs;
    float a, b, rate;
    uint64_t seed;
};

// The update of vertex i in epoch `epoch`: cur is read, nxt[i] is written.  Terms are summed edge by edge in CSR order,
// the attractive term of a due edge (twice: the layout moves both ends of an edge, and W is symmetric) and then its due
// negative samples by sample index.  Every product and sum below is one rounded float32 operation.
template <int DIM>
__device__ __forceinline__ void layout_vertex(const LayoutGraph &G, int i, int epoch, const float *cur, float *nxt) {
#pragma clang fp contract(off)
    float yi[DIM], g[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) { yi[d] = cur[i * DIM + d]; g[d] = 0.f; }
    const float fn = (float)epoch;
    const float alpha = 1.f - fn / (float)G.n_epochs;
    const float a = G.a, b = G.b;
    const float two_ab = 2.f * a * b, two_b = 2.f * b;
    const uint64_t key = embed_mix64(G.seed + EMBED_GOLDEN * (uint64_t)(epoch + 1));
    const int end = G.indptr[i + 1];
    for (int e = G.indptr[i]; e < end; ++e) {
        float2 st = G.state[e];
        if (!(st.x <= fn)) continue;
        const int j = G.indices[e];
        const float ee = G.eps[e];
        float diff[DIM], d2 = 0.f;
#pragma unroll
        for (int d = 0; d < DIM; ++d) { diff[d] = yi[d] - cur[j * DIM + d]; d2 += diff[d] * diff[d]; }
        float c = 0.f;
        if (d2 > 0.f) {
            const float pb = powf(d2, b);
            c = -(two_ab * pb) / (d2 * (a * pb + 1.f));
        }
#pragma unroll
        for (int d = 0; d < DIM; ++d) g[d] += 2.f * clip4(c * diff[d]);
        st.x += ee;
        const float epn = ee / G.rate;
        const int n_neg = (int)((fn - st.y) / epn);
        const uint64_t ekey = embed_mix64(key ^ (uint64_t)e);
        for (int p = 0; p < n_neg; ++p) {
            const uint64_t h = embed_mix64(ekey + EMBED_GOLDEN * (uint64_t)(p + 1));
            const int v = (int)((uint32_t)(h >> 32) % (uint32_t)G.t);
            d2 = 0.f;
#pragma unroll
            for (int d = 0; d < DIM; ++d) { diff[d] = yi[d] - cur[v * DIM + d]; d2 += diff[d] * diff[d]; }
            c = 0.f;
            if (v != i && d2 > 0.f) {
                const float pb = powf(d2, b);
                c = two_b / ((0.001f + d2) * (a * pb + 1.f));
            }
#pragma unroll
            for (int d = 0; d < DIM; ++d) g[d] += clip4(c * diff[d]);
        }
        st.y += (float)n_neg * epn;
        G.state[e] = st;
    }
#pragma unroll
    for (int d = 0; d < DIM; ++d) nxt[i * DIM + d] = yi[d] + alpha * g[d];
}

// grid (1), block (LAYOUT_LDS_BLOCK), dynamic LDS 2 * t * DIM floats.  y [t][DIM]: the initial layout in, the final one out.
template <int DIM>
__global__ __launch_bounds__(LAYOUT_LDS_BLOCK) void k_layout_lds(LayoutGraph G, float *__restrict__ y) {
    extern __shared__ float layout_lds[];
    const int n = G.t * DIM;
    float *cur = layout_lds, *nxt = layout_lds + n;
    for (int x = threadIdx.x; x < n; x += LAYOUT_LDS_BLOCK) cur[x] = y[x];
    __syncthreads();
    for (int epoch = 0; epoch < G.n_epochs; ++epoch) {
        for (int i = threadIdx.x; i < G.t; i += LAYOUT_LDS_BLOCK) layout_vertex<DIM>(G, i, epoch, cur, nxt);
        __syncthreads();
        float *s = cur; cur = nxt; nxt = s;
    }
    for (int x = threadIdx.x; x < n; x += LAYOUT_LDS_BLOCK) y[x] = cur[x];
}

// grid (vertices / LAYOUT_EPOCH_BLOCK), one launch per epoch; cur and nxt [t][DIM] are different buffers
template <int DIM>
__global__ __launch_bounds__(LAYOUT_EPOCH_BLOCK) void k_layout_epoch(LayoutGraph G, int epoch, const float *__restrict__ cur,
                                                                     float *__restrict__ nxt) {
    const int i = blockIdx.x * LAYOUT_EPOCH_BLOCK + threadIdx.x;
    if (i < G.t) layout_vertex<DIM>(G, i, epoch, cur, nxt);
}

}  // namespace plsa
