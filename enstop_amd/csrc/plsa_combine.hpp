// plsa_combine.hpp -- host side of the topic combination, the second half of what the ensemble does: all-pairs Hellinger and KL
// and the cluster representatives (include/plsa_hip.h; plsa_combine_kernels.hpp), the co-document counts
// (include/plsa_hip_metrics.h; plsa_metric_kernels.hpp), k-NN membership and the force layout (include/plsa_hip_embed.h;
// plsa_embed_kernels.hpp).  Part of plsa_hip.hip's translation unit (included at its end: it uses the context, `ensure`,
// `Scope` and `launch_check` defined there).  Grids, carves and member lists come from plsa_combine_plan.hpp.
//
// The six entry points share one frame, CombineCall: it opens the call (NULL context, device), uploads and downloads, and
// guards every exit -- no entry point returns while the stream may still read host memory or a local buffer.
#pragma once

#include "../../include/plsa_hip_embed.h"
#include "../../include/plsa_hip_metrics.h"
#include "plsa_embed_kernels.hpp"
#include "plsa_metric_kernels.hpp"

namespace {

// Declared AFTER every host vector and local DevBuf the stream reads, so that it is destroyed before them: while `busy`, its
// destructor waits for the stream, whichever HIPCHK, CHK or refusal the call leaves through.
struct CombineCall {
    plsa_ctx *c;
    const char *who;
    bool busy = false;          // the stream may hold work of this call
    CombineCall(plsa_ctx *c_, const char *who_) : c(c_), who(who_) {}
    ~CombineCall() { if (busy) (void)hipStreamSynchronize(c->stream); }
    int open() {
        if (!c) return fail(c, "%s: ctx is NULL", who);
        HIPCHK(c, hipSetDevice(c->device));
        return 0;
    }
    int copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
        busy = true;
        HIPCHK(c, hipMemcpyAsync(dst, src, bytes, kind, c->stream));
        return 0;
    }
    int to_device(void *dst, const void *src, size_t bytes) { return copy(dst, src, bytes, hipMemcpyHostToDevice); }
    int download(void *dst, const void *src, size_t bytes) { return copy(dst, src, bytes, hipMemcpyDeviceToHost); }
    int upload(DevBuf &b, const void *src, size_t bytes) {          // ensure and upload
        CHK(ensure(c, b, bytes));
        return bytes ? to_device(b.p, src, bytes) : 0;
    }
    int zero(void *dst, size_t bytes) {
        busy = true;
        HIPCHK(c, hipMemsetAsync(dst, 0, bytes, c->stream));
        return 0;
    }
    int wait() {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        busy = false;
        return 0;
    }
};

// one launch on the call's stream: in a Scope under its kernel's name, followed by launch_check
#define COMBINE_LAUNCH(call, name, kernel, grid, block, lds, ...)                                  \
    do {                                                                                           \
        (call).busy = true;                                                                        \
        { Scope s_((call).c, name);                                                                \
          hipLaunchKernelGGL(kernel, grid, block, lds, (call).c->stream, __VA_ARGS__); }           \
        CHK(launch_check((call).c, name));                                                         \
    } while (0)

template <int DIM>
int layout_run(CombineCall &call, const plsa::LayoutGraph &G, float *y0, float *y1, bool lds, float **result) {
    if (lds) {
        COMBINE_LAUNCH(call, "k_layout_lds", plsa::k_layout_lds<DIM>, dim3(1), dim3(plsa::LAYOUT_LDS_BLOCK),
                       sizeof(float) * 2 * (size_t)G.t * DIM, G, y0);
        *result = y0;
        return 0;
    }
    const unsigned grid = plsa::plan::layout_epoch_grid(G.t);
    float *cur = y0, *nxt = y1;
    for (int epoch = 0; epoch < G.n_epochs; ++epoch) {
        COMBINE_LAUNCH(call, "k_layout_epoch", plsa::k_layout_epoch<DIM>, dim3(grid), dim3(plsa::LAYOUT_EPOCH_BLOCK), 0, G, epoch, cur, nxt);
        std::swap(cur, nxt);
    }
    *result = cur;
    return 0;
}

}  // namespace

extern "C" {

// enstop/utils.py:22-41 with axis=1 (float64, sequential marginal, guarded division)
void plsa_host_normalize_rows(double *a, int64_t rows, int64_t cols) {
    for (int64_t i = 0; i < rows; ++i) {
        double *r = a + i * cols;
        double marginal = 0.0;
        for (int64_t j = 0; j < cols; ++j) marginal += r[j];
        if (marginal > 0.0)
            for (int64_t j = 0; j < cols; ++j) r[j] /= marginal;
    }
}

// enstop/enstop_.py:258-266 (pairwise umap.distances.hellinger over the stacked topics) on the device
int plsa_all_pairs_hellinger(plsa_ctx *c, const float *topics, int64_t t, int64_t m, double *D) {
    DevBuf R, l1, part, dD;
    CombineCall call(c, "plsa_all_pairs_hellinger");
    CHK(call.open());
    if (!topics || !D || t <= 0 || m <= 0 || t > 65536) return fail(c, "plsa_all_pairs_hellinger: bad arguments");
    const i64 tiles = plsa::plan::tri_tiles(plsa::plan::pair_nt(t));
    const plsa::plan::Slicing s = plsa::plan::vocab_slicing(tiles, m, c->prop.multiProcessorCount);
    const dim3 block(plsa::plan::COMBINE_BLOCK);
    CHK(ensure(c, l1, sizeof(double) * (size_t)t));
    CHK(ensure(c, part, sizeof(double) * (size_t)s.slices * t * t));
    CHK(ensure(c, dD, sizeof(double) * (size_t)t * t));
    CHK(call.upload(R, topics, sizeof(float) * (size_t)t * m));
    COMBINE_LAUNCH(call, "k_hell_prepare", plsa::k_hell_prepare, dim3((unsigned)t), block, 0, R.as<float>(), (int)t, (i64)m, l1.as<double>());
    COMBINE_LAUNCH(call, "k_hell_gram", plsa::k_hell_gram, dim3((unsigned)tiles, (unsigned)s.slices), block, 0, R.as<float>(), (int)t,
                   (i64)m, (i64)s.words, part.as<double>());
    COMBINE_LAUNCH(call, "k_hell_finish", plsa::k_hell_finish, dim3(plsa::plan::elementwise_grid(t * t)), block, 0, part.as<double>(),
                   s.slices, (int)t, l1.as<double>(), dD.as<double>());
    CHK(call.download(D, dD.p, sizeof(double) * (size_t)t * t));
    return call.wait();
}

// enstop/enstop_.py:244-253 (all_pairs_kl_divergence over the stacked topics) on the device
int plsa_all_pairs_kl(plsa_ctx *c, const float *topics, int64_t t, int64_t m, double *D) {
    DevBuf T, part, dD;
    CombineCall call(c, "plsa_all_pairs_kl");
    CHK(call.open());
    if (!topics || !D || t <= 0 || m <= 0 || t > 65536) return fail(c, "plsa_all_pairs_kl: bad arguments");
    const i64 tiles = plsa::plan::square_tiles(plsa::plan::pair_nt(t));
    const plsa::plan::Slicing s = plsa::plan::vocab_slicing(tiles, m, c->prop.multiProcessorCount);
    const dim3 block(plsa::plan::COMBINE_BLOCK);
    CHK(ensure(c, part, sizeof(double) * (size_t)s.slices * t * t));
    CHK(ensure(c, dD, sizeof(double) * (size_t)t * t));
    CHK(call.upload(T, topics, sizeof(float) * (size_t)t * m));
    COMBINE_LAUNCH(call, "k_kl_gram", plsa::k_kl_gram, dim3((unsigned)tiles, (unsigned)s.slices), block, 0, T.as<float>(), (int)t, (i64)m,
                   (i64)s.words, part.as<double>());
    COMBINE_LAUNCH(call, "k_sum_slices", plsa::k_sum_slices, dim3(plsa::plan::elementwise_grid(t * t)), block, 0, part.as<double>(),
                   s.slices, (i64)t * t, dD.as<double>());
    CHK(call.download(D, dD.p, sizeof(double) * (size_t)t * t));
    return call.wait();
}

// enstop/enstop_.py:299-308, 340-345 (weights == NULL) and 385-393 (membership-strength weights)
int plsa_cluster_representatives(plsa_ctx *c, const float *topics, int64_t t, int64_t m, const int32_t *labels,
                                 const double *weights, int32_t n_clusters, float *out) {
    std::vector<int> first, members;
    DevBuf T, dfirst, dmem, dw, rep, bs, dout;
    CombineCall call(c, "plsa_cluster_representatives");
    CHK(call.open());
    if (!topics || !labels || !out || t <= 0 || m <= 0 || n_clusters < 0)
        return fail(c, "plsa_cluster_representatives: bad arguments");
    if (n_clusters == 0) return 0;
    if (n_clusters > plsa::plan::GRID_YZ_MAX)      // a cluster is a row of the grid
        return fail(c, "plsa_cluster_representatives: n_clusters=%d above %d", n_clusters, plsa::plan::GRID_YZ_MAX);
    const i64 bad = plsa::plan::member_lists(labels, t, n_clusters, first, members);
    if (bad >= 0) return fail(c, "plsa_cluster_representatives: label %d >= n_clusters %d", labels[bad], n_clusters);
    // enstop_.py:385-393 np.average raises on an all-zero weight vector; callers handle that case
    const unsigned nb = plsa::plan::elementwise_grid(m);
    const dim3 grid(nb, (unsigned)n_clusters), block(plsa::plan::COMBINE_BLOCK);
    CHK(ensure(c, rep, sizeof(double) * (size_t)n_clusters * m));
    CHK(ensure(c, bs, sizeof(double) * (size_t)n_clusters * nb));
    CHK(ensure(c, dout, sizeof(float) * (size_t)n_clusters * m));
    CHK(call.upload(T, topics, sizeof(float) * (size_t)t * m));
    CHK(call.upload(dfirst, first.data(), sizeof(int) * first.size()));
    CHK(call.upload(dmem, members.data(), sizeof(int) * members.size()));
    if (weights) CHK(call.upload(dw, weights, sizeof(double) * (size_t)t));
    COMBINE_LAUNCH(call, "k_rep_accumulate", plsa::k_rep_accumulate, grid, block, 0, T.as<float>(), (i64)m, dfirst.as<int>(),
                   dmem.as<int>(), weights ? dw.as<double>() : nullptr, rep.as<double>(), bs.as<double>());
    COMBINE_LAUNCH(call, "k_rep_normalise", plsa::k_rep_normalise, grid, block, 0, rep.as<double>(), (i64)m, bs.as<double>(), (int)nb,
                   dout.as<float>());
    CHK(call.download(out, dout.p, sizeof(float) * (size_t)n_clusters * m));
    return call.wait();
}

// enstop/utils.py:150-203 (the counts behind coherence: pairwise document-list intersections, `data > 0` column sums) on
// the device: plsa_metric_kernels.hpp
int plsa_codocument_counts(plsa_ctx *c, const int32_t *words, int64_t sets, int32_t nw, int32_t max_sets_per_pass,
                           int64_t *co, int64_t *positive) {
    CombineCall call(c, "plsa_codocument_counts");
    CHK(call.open());
    if (nw < 2 || nw > plsa::METRIC_MAX_WORDS)
        return fail(c, "plsa_codocument_counts: nw=%d outside [2,%d]", nw, plsa::METRIC_MAX_WORDS);
    if (sets < 1 || sets > ((i64)1 << 24)) return fail(c, "plsa_codocument_counts: sets=%lld outside [1,2^24]", (long long)sets);
    if (max_sets_per_pass < 0) return fail(c, "plsa_codocument_counts: max_sets_per_pass=%d is negative", max_sets_per_pass);
    if (!words || !co || !positive) return fail(c, "plsa_codocument_counts: words, co and positive must not be NULL");
    if (c->n <= 0) return fail(c, "plsa_codocument_counts: no corpus uploaded");
    // the ids index colptr on the device: checked here, before anything is launched
    for (i64 i = 0; i < sets * nw; ++i)
        if (words[i] < 0 || words[i] >= c->m)
            return fail(c, "plsa_codocument_counts: word id %d (set %lld, position %lld) outside [0,%lld)", words[i],
                        (long long)(i / nw), (long long)(i % nw), (long long)c->m);
    const i64 n = c->n, per_co = (i64)nw * nw;
    std::fill(co, co + sets * per_co, (int64_t)0);
    std::fill(positive, positive + sets * nw, (int64_t)0);
    if (c->nnz == 0) return 0;
    CHK(ensure_csc(c));
    size_t free_b = 0, total_b = 0;
    if (max_sets_per_pass == 0 && hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)1 << 30; }
    const i64 chunk = plsa::plan::metric_sets_per_pass(free_b, c->metric_mask.cap, n, sets, max_sets_per_pass);
    const plsa::plan::MetricCarve carve = plsa::plan::metric_carve(chunk, nw);
    CHK(ensure(c, c->metric_mask, sizeof(unsigned) * (size_t)chunk * (size_t)n));
    CHK(ensure(c, c->metric_small, carve.total));
    char *small = c->metric_small.as<char>();
    unsigned long long *d_co = reinterpret_cast<unsigned long long *>(small + carve.co);
    unsigned long long *d_pos = reinterpret_cast<unsigned long long *>(small + carve.positive);
    int *d_words = reinterpret_cast<int *>(small + carve.words);
    const unsigned mark_x = plsa::plan::metric_mark_x(n), count_x = plsa::plan::metric_count_x(n);
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counters are copied out as int64");
    for (i64 s0 = 0; s0 < sets; s0 += chunk) {
        const i64 cs = std::min<i64>(chunk, sets - s0);
        CHK(call.zero(c->metric_mask.p, sizeof(unsigned) * (size_t)cs * (size_t)n));
        CHK(call.zero(d_co, carve.words));                 // both counter arrays
        CHK(call.to_device(d_words, words + s0 * nw, sizeof(int) * (size_t)(cs * nw)));
        COMBINE_LAUNCH(call, "k_metric_mark", plsa::k_metric_mark, dim3(mark_x, (unsigned)nw, (unsigned)cs), dim3(plsa::METRIC_BLOCK), 0,
                       c->csc.colptr.as<int>(), c->csc.row.as<int>(), c->csc.val.as<float>(), d_words, (int)nw, (int64_t)n,
                       c->metric_mask.as<unsigned>(), d_pos);
        COMBINE_LAUNCH(call, "k_metric_count", plsa::k_metric_count, dim3(count_x, (unsigned)cs), dim3(plsa::METRIC_BLOCK), 0,
                       c->metric_mask.as<unsigned>(), (int)nw, (int64_t)n, d_co);
        CHK(call.download(co + s0 * per_co, d_co, sizeof(int64_t) * (size_t)(cs * per_co)));
        CHK(call.download(positive + s0 * nw, d_pos, sizeof(int64_t) * (size_t)(cs * nw)));
        CHK(call.wait());   // the next chunk reuses the staging buffers
    }
    return 0;
}

// enstop/enstop_.py:354-414 (umap.UMAP on the stacked topics): nearest neighbours, bandwidths and membership strengths of a
// precomputed distance matrix -- plsa_embed_kernels.hpp
int plsa_knn_membership(plsa_ctx *c, const double *D, int64_t t, int32_t n_neighbors, int32_t *idx, float *dist, float *rho,
                        float *sigma, float *member) {
    DevBuf dD, dint, dflt;
    CombineCall call(c, "plsa_knn_membership");
    CHK(call.open());
    if (!D || !idx || !dist || !rho || !sigma || !member) return fail(c, "plsa_knn_membership: an array is NULL");
    if (t < 2 || t > 65536) return fail(c, "plsa_knn_membership: t=%lld outside [2,65536]", (long long)t);
    if (n_neighbors < 1 || n_neighbors > t || n_neighbors > plsa::EMBED_MAX_NEIGHBORS)
        return fail(c, "plsa_knn_membership: n_neighbors=%d outside [1,min(t,%d)]", n_neighbors, plsa::EMBED_MAX_NEIGHBORS);
    for (i64 i = 0; i < t * t; ++i)      // a NaN would never be selected: a row could run out of entries
        if (!std::isfinite(D[i])) return fail(c, "plsa_knn_membership: D[%lld,%lld] is not finite", (long long)(i / t), (long long)(i % t));
    const size_t tk = (size_t)t * (size_t)n_neighbors;
    const plsa::plan::KnnCarve carve = plsa::plan::knn_carve(t, n_neighbors);
    CHK(ensure(c, dint, sizeof(int) * carve.int_total));
    CHK(ensure(c, dflt, sizeof(float) * carve.float_total));
    int *d_idx = dint.as<int>() + carve.idx;
    unsigned *d_done = reinterpret_cast<unsigned *>(dint.as<int>() + carve.done);
    float *f = dflt.as<float>();
    CHK(call.upload(dD, D, sizeof(double) * (size_t)t * t));
    CHK(call.zero(d_done, sizeof(unsigned)));
    COMBINE_LAUNCH(call, "k_knn_membership", plsa::k_knn_membership, dim3((unsigned)t), dim3(64), 0, dD.as<double>(), (int)t,
                   (int)n_neighbors, d_idx, f + carve.dist, f + carve.rho, f + carve.sigma, f + carve.member, f + carve.row_sum, d_done);
    CHK(call.download(idx, d_idx, sizeof(int) * tk));
    CHK(call.download(dist, f + carve.dist, sizeof(float) * tk));
    CHK(call.download(member, f + carve.member, sizeof(float) * tk));
    CHK(call.download(rho, f + carve.rho, sizeof(float) * (size_t)t));
    CHK(call.download(sigma, f + carve.sigma, sizeof(float) * (size_t)t));
    return call.wait();
}

// enstop/enstop_.py:354-414 (umap.UMAP on the stacked topics): the force layout of the fuzzy graph -- plsa_embed_kernels.hpp
int plsa_layout(plsa_ctx *c, const int32_t *indptr, const int32_t *indices, const float *weights, int64_t t, int32_t dim,
                float *y_inout, int32_t n_epochs, float a, float b, int32_t negative_sample_rate, uint64_t seed, int32_t path) {
    std::vector<float> eps;
    std::vector<float2> state;
    DevBuf dptr, dind, deps, dstate, dy;
    CombineCall call(c, "plsa_layout");
    CHK(call.open());
    if (!indptr || !y_inout) return fail(c, "plsa_layout: indptr and y_inout must not be NULL");
    if (t < 1 || t > 65536) return fail(c, "plsa_layout: t=%lld outside [1,65536]", (long long)t);
    if (dim < 1 || dim > plsa::EMBED_MAX_DIM) return fail(c, "plsa_layout: dim=%d outside [1,%d]", dim, plsa::EMBED_MAX_DIM);
    if (n_epochs < 1 || n_epochs > 100000) return fail(c, "plsa_layout: n_epochs=%d outside [1,100000]", n_epochs);
    if (negative_sample_rate < 1 || negative_sample_rate > 64)
        return fail(c, "plsa_layout: negative_sample_rate=%d outside [1,64]", negative_sample_rate);
    if (path < 0 || path > 2) return fail(c, "plsa_layout: path=%d is none of 0 (auto), 1 (LDS), 2 (per epoch)", path);
    if (!std::isfinite(a) || !std::isfinite(b) || a <= 0.f || b <= 0.f) return fail(c, "plsa_layout: a and b must be positive");
    // the graph indexes the position buffers on the device: checked here, before anything is launched
    if (indptr[0] != 0) return fail(c, "plsa_layout: indptr[0] is not 0");
    for (i64 i = 0; i < t; ++i)
        if (indptr[i + 1] < indptr[i]) return fail(c, "plsa_layout: indptr decreases at row %lld", (long long)i);
    const i64 nnz = indptr[t];
    if (nnz > 0 && (!indices || !weights)) return fail(c, "plsa_layout: indices and weights must not be NULL");
    float wmax = 0.f;
    for (i64 e = 0; e < nnz; ++e) {
        if (indices[e] < 0 || indices[e] >= t) return fail(c, "plsa_layout: indices[%lld]=%d outside [0,%lld)", (long long)e, indices[e], (long long)t);
        if (!std::isfinite(weights[e]) || !(weights[e] > 0.f)) return fail(c, "plsa_layout: weights[%lld] is not a positive number", (long long)e);
        wmax = std::max(wmax, weights[e]);
    }
    for (i64 i = 0; i < t * dim; ++i)
        if (!std::isfinite(y_inout[i])) return fail(c, "plsa_layout: y_inout[%lld] is not finite", (long long)i);
    const size_t y_bytes = sizeof(float) * (size_t)t * (size_t)dim;
    const plsa::plan::LayoutPath taken = plsa::plan::layout_path(path, plsa::plan::layout_fits_lds(t, dim));
    if (taken == plsa::plan::LAYOUT_REFUSED)
        return fail(c, "plsa_layout: path 1 keeps two position buffers in LDS: 2 * %lld * %d * 4 = %zu bytes exceed %zu", (long long)t,
                    dim, 2 * y_bytes, plsa::LAYOUT_LDS_BYTES);
    const float rate = (float)negative_sample_rate;
    eps.resize((size_t)nnz);
    state.resize((size_t)nnz);
    for (i64 e = 0; e < nnz; ++e) {
        const plsa::plan::EdgeSchedule s = plsa::plan::layout_edge_schedule(wmax, weights[e], rate);
        eps[e] = s.eps;
        state[e] = make_float2(s.eps, s.negative);
    }
    CHK(ensure(c, dy, 2 * y_bytes));
    CHK(call.upload(dptr, indptr, sizeof(int) * (size_t)(t + 1)));
    CHK(call.upload(dind, indices, sizeof(int) * (size_t)nnz));
    CHK(call.upload(deps, eps.data(), sizeof(float) * (size_t)nnz));
    CHK(call.upload(dstate, state.data(), sizeof(float2) * (size_t)nnz));
    CHK(call.to_device(dy.p, y_inout, y_bytes));
    plsa::LayoutGraph G;
    G.indptr = dptr.as<int>(); G.indices = dind.as<int>(); G.eps = deps.as<float>(); G.state = dstate.as<float2>();
    G.t = (int)t; G.n_epochs = n_epochs; G.a = a; G.b = b; G.rate = rate; G.seed = seed;
    float *y0 = dy.as<float>(), *y1 = y0 + (size_t)t * dim, *result = nullptr;
    static constexpr decltype(&layout_run<1>) run[plsa::EMBED_MAX_DIM] = {layout_run<1>, layout_run<2>, layout_run<3>, layout_run<4>,
                                                                          layout_run<5>, layout_run<6>, layout_run<7>, layout_run<8>};
    CHK(run[dim - 1](call, G, y0, y1, taken == plsa::plan::LAYOUT_LDS, &result));
    CHK(call.download(y_inout, result, y_bytes));
    return call.wait();
}

#undef COMBINE_LAUNCH

}  // extern "C"
