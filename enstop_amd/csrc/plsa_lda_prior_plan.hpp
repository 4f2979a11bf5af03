// plsa_lda_prior_plan.hpp -- the launch arithmetic of the kernels of LDA's learned priors (plsa_lda_prior_kernels.hpp) and the
// schedule of the prior updates (plsa_lda_priors.hpp), free of HIP like plsa_lda_plan.hpp, on which it stands: plain values
// in, plain values out.  tests/lda_prior_host.cpp walks the same functions on a CPU (its `logmean` and `due` commands).
//
// k_lda_logmean: slabs of whole rows, each owning one float64 partial per topic -- the cut of k_log_prior (prior_rows_first,
// prior_rows_last) into lda_logmean_grid(rows) = min(LDA_LOGMEAN_SLABS, max(rows, 1)) slabs: a function of the row count alone,
// never of the grid cap, so the partials and the sums formed of them do not depend on the launch geometry.  A slab's workgroup
// walks the topics in batches of 256: in the batch that starts at topic zb, logmean_span(kp, zb) topics are live and
// logmean_strands(span) = 256 / span threads share a topic -- thread t owns topic zb + t % span and the strand t / span, the
// rows first + strand, first + strand + strands, ... of the slab (a thread whose strand is not below `strands` idles); the
// strands of a topic are added in strand order.  k_lda_logmean_sums has the workgroups and lanes of k_lda_topic_sums
// (lda_topic_grid, LDA_TOPIC_LANES); a lane adds its partials into LOGMEAN_CHAINS sums in turn and those in their order.
//
// k_lda_rows_v, k_lda_bound_v: the walks of k_lda_rows and of k_lda_bound.
//
// The schedule: priors are updated after the iterations prior_start, prior_start + prior_every, ... (counted from 1).
#pragma once

#include "plsa_lda_plan.hpp"

namespace plsa {
namespace plan {

constexpr int LDA_LOGMEAN_SLABS = 4096;
constexpr int LOGMEAN_CHAINS = 8;      // sums a lane of k_lda_logmean_sums keeps going: its j-th partial goes into sum j % 8

inline int lda_logmean_grid(int64_t rows) { return (int)std::min<int64_t>(LDA_LOGMEAN_SLABS, std::max<int64_t>(rows, 1)); }

#if defined(__HIPCC__)
#define PLSA_LDA_PRIOR_HD __host__ __device__
#else
#define PLSA_LDA_PRIOR_HD
#endif

PLSA_LDA_PRIOR_HD inline int logmean_span(int kp, int zb) { return kp - zb < LDA_BLOCK ? kp - zb : LDA_BLOCK; }
PLSA_LDA_PRIOR_HD inline int logmean_strands(int span) { return LDA_BLOCK / span; }
#undef PLSA_LDA_PRIOR_HD

// whether the priors are updated behind iteration `done` (1-based: the count of iterations finished)
inline bool prior_due(int done, int prior_start, int prior_every) {
    return done >= prior_start && (done - prior_start) % prior_every == 0;
}

}  // namespace plan
}  // namespace plsa
