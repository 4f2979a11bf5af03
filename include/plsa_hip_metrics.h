/*
 * plsa_hip_metrics.h -- topic-quality metrics of libplsa_hip.so on the device.
 *
 * The reference scores a topic by the coherence of its top words (enstop/utils.py:150-203): for every pair of top words it
 * intersects the two words' document lists, and it divides by the number of documents in which the earlier word has a
 * positive count.  Both are integer counts over the corpus; everything after them is a handful of logarithms.  The counts
 * are what this entry point computes, on the matrix that is ACTIVE on the context (the uploaded corpus or its current
 * bootstrap resample), exactly: integer arithmetic that does not depend on the order of execution.
 *
 * Same conventions as plsa_hip.h: status codes, plsa_last_error(ctx), borrowed host arrays, not thread-safe.
 */
#ifndef PLSA_HIP_METRICS_H
#define PLSA_HIP_METRICS_H

#include "plsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* words[s*nw + i], 0 <= s < sets, 0 <= i < nw: `sets` lists of `nw` distinct column ids each, 2 <= nw <= 32.
 *   co[(s*nw + i)*nw + j]  documents with a STORED entry in column words[s,i] and in column words[s,j] (stored zeros
 *                          count, as in the reference's index intersection); the diagonal is the column's stored entries
 *   positive[s*nw + i]     stored entries of column words[s,i] whose value is > 0 (enstop/utils.py:234, `data > 0`)
 * The sets are processed max_sets_per_pass at a time (0: as many as a quarter of the free device memory allows), one
 * 32-bit mask per document and set of scratch; plsa_release_scratch frees it.  An id outside [0, m), nw outside [2, 32],
 * sets < 1, a NULL array or a context without a corpus is a status code: nothing is launched.  A corpus without stored
 * entries, or an empty column, gives zeros. */
int plsa_codocument_counts(plsa_ctx *ctx, const int32_t *words /* [sets*nw] */, int64_t sets, int32_t nw,
                           int32_t max_sets_per_pass, int64_t *co /* [sets*nw*nw] */, int64_t *positive /* [sets*nw] */);

#ifdef __cplusplus
}
#endif
#endif
