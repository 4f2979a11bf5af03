/*
 * plsa_hip_embed.h -- the embedding stage of topic_combination="hellinger_umap" of libplsa_hip.so on the device.
 *
 * The reference hands the stacked topics of an ensemble to umap.UMAP(n_neighbors, n_components, metric="hellinger") and
 * clusters the embedding (enstop_.py:354-414).  The stack is a few hundred to a few thousand points and
 * plsa_all_pairs_hellinger already gives their exact distance matrix, so UMAP as published reduces to the two entry points
 * below and a few O(t * n_neighbors) host steps between them (symmetrisation, the sampling schedule, the initial layout:
 * enstop_amd/embedding.py).  The layout is synchronous and deterministic: a result is a function of the inputs and the seed.
 *
 * Same conventions as plsa_hip.h: status codes, plsa_last_error(ctx), borrowed host arrays, not thread-safe.
 */
#ifndef PLSA_HIP_EMBED_H
#define PLSA_HIP_EMBED_H

#include "plsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* enstop_.py:354-414 (umap's nearest neighbours, smooth_knn_dist and membership strengths on a precomputed metric).
 * D [t*t] row-major distances, finite; 2 <= t <= 65536; 1 <= n_neighbors <= min(t, 1024) counts the row's own entry.
 *   idx, dist [t*n_neighbors]  the n_neighbors smallest entries of every row, ascending, ties towards the lower column
 *                              (np.argsort(kind="stable")); dist is the float32 of the entry
 *   rho [t]      smallest positive neighbour distance, 0 without one
 *   sigma [t]    sum_{j>=1} (d_j - rho > 0 ? exp(-(d_j - rho) / sigma) : 1) = log2(n_neighbors), by at most 64 bisection steps
 *                to 1e-5 in float32, then at least 1e-3 * mean(d_row) (rho > 0) or 1e-3 * mean of all neighbour distances
 *   member [t*n_neighbors]  0 for the row itself, 1 where d - rho <= 0, else exp(-(d - rho) / sigma)
 * One kernel launch.  A NULL array, a size outside the ranges or a non-finite distance is a status code: nothing is launched. */
int plsa_knn_membership(plsa_ctx *ctx, const double *D, int64_t t, int32_t n_neighbors, int32_t *idx, float *dist,
                        float *rho, float *sigma, float *member);

/* enstop_.py:354-414 (umap's optimize_layout_euclidean, restated as a synchronous update: in every epoch each vertex reads
 * the positions the epoch began with, sums its terms in CSR order and moves once).
 * indptr [t+1], indices, weights [indptr[t]]: the symmetric fuzzy graph as CSR, weights > 0; an edge is sampled every
 * max(weights) / weight epochs and draws negative_sample_rate negative samples per sample, their vertices from a
 * counter-based generator keyed by (seed, epoch, edge, sample).  y_inout [t*dim]: the initial layout in, the final layout
 * out.  1 <= dim <= 8, 1 <= n_epochs <= 100000, 1 <= negative_sample_rate <= 64.  The learning rate of epoch e is
 * 1 - e / n_epochs.
 * path  0: the persistent kernel when both position buffers fit the workgroup's 64 KiB of LDS (2 * t * dim * 4 bytes),
 *          else one launch per epoch;  1: the persistent kernel, a status code when it does not fit;  2: one launch per
 *          epoch.  Both paths run the same per-vertex code and give the same bits. */
int plsa_layout(plsa_ctx *ctx, const int32_t *indptr, const int32_t *indices, const float *weights, int64_t t, int32_t dim,
                float *y_inout, int32_t n_epochs, float a, float b, int32_t negative_sample_rate, uint64_t seed,
                int32_t path);

#ifdef __cplusplus
}
#endif
#endif
