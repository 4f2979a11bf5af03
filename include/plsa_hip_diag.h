/*
 * plsa_hip_diag.h -- diagnostics, measurement hooks, test plumbing and synthetic corpora of libplsa_hip.so.
 *
 * NOT part of the drop-in: a maintainer binding the reference's seam (enstop/enstop_.py:52-53) needs include/plsa_hip.h
 * only.  What is declared here has no counterpart in the reference; it exists for bench.py (timings, bandwidth ceilings,
 * the synthetic corpora of SURVEY.md section 8d), for the parity tests (read-backs, a given P(z|w,d), host emulation of
 * the all-reduce, NumPy-identity of the device initialisation) and for reports (schedule, placement, queues).
 * Same conventions as plsa_hip.h: status codes, plsa_last_error(), borrowed host arrays, opaque context.
 */
#ifndef PLSA_HIP_DIAG_H
#define PLSA_HIP_DIAG_H

#include "plsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the GPU_MAX_HW_QUEUES value this process runs with (4 = the HIP runtime's default; see plsa_hip.h, lifetime) */
int plsa_hw_queues(void);
/* 64-char device name ("AMD Instinct MI355X"), gcnArchName, CU count and HBM bytes. */
int plsa_device_info(plsa_ctx *ctx, char *name64, char *arch64, int *cus, int64_t *hbm_bytes);

/* read back the ACTIVE matrix (the uploaded corpus, a bootstrap resample, a synthetic corpus) in the layout of plsa_upload_csr */
int plsa_download_active_csr(plsa_ctx *ctx, int32_t *indptr, int32_t *indices, float *data);

/* Throughput-mode alternative to plsa_init(random) + plsa_set_factors: uniform draws from a
 * counter-based generator, rows L1-normalised, entirely on the device.  NOT the reference's NumPy
 * MT19937 stream -- use plsa_set_factors for seed-for-seed parity (enstop/plsa.py:455-456).      */
int plsa_init_factors_device(plsa_ctx *ctx, int32_t k, uint64_t seed);

/* Diagnostics: the k float64 topic marginals (enstop/utils.py:24-29, `marginal[i] += ndarray[i, j]` left to right) that the
 * last plsa_init_factors_mt19937 call divided by.  The device evaluates that sequential sum from per-chunk parity pairs
 * (csrc/plsa_init_kernels.hpp: k_mt_chunk_pairs); the tests pin it bit for bit to numpy's own sequential accumulation. */
int plsa_mt_marginals(plsa_ctx *ctx, double *out, int32_t k);

/* uploads a host P(z|w,d) [nnz,k] in place of plsa_e_step's output (lets plsa_m_step be tested in isolation against
 * enstop/plsa.py:124-204) */
int plsa_set_p(plsa_ctx *ctx, const float *P);

/* host copies of the un-normalised P(w|z) accumulator [m, kp] of the doc-sharded fit (plsa_accumulator_device): a host-side
 * emulation of the all-reduce for tests without a communicator */
int plsa_accumulator_get(plsa_ctx *ctx, float *host);
int plsa_accumulator_set(plsa_ctx *ctx, const float *host);

/* RCCL's own text for the last failure in this process (ncclGetLastError); ctx may be NULL.  No reference
 * counterpart (dask / joblib raise Python exceptions, enstop_.py:209-217); read by enstop_amd/comm.py::report_failure
 * so that a failed multi-GPU start says which stage and why. */
int plsa_comm_last_error(plsa_ctx *ctx, char *buf, int64_t cap);

/* barrier and float64 all-reduce (op 0 sum, 1 max) over the context's communicator, staged through HBM: the bracketing and the
 * max-over-ranks of bench.py's timed regions.  Identity without a communicator. */
int plsa_comm_barrier(plsa_ctx *ctx);
int plsa_comm_allreduce_f64(plsa_ctx *ctx, double *inout, int64_t count, int32_t op);

/* PLSA_REFERENCE_SUMS: norm_pwz[z] -- the reference's one float32 running sum over all non-zeros, enstop/plsa.py:193 -- is evaluated
 * from per-chunk (parity -> increment) pairs and a walk that checks every chunk; chunks that fail the check (binade crossings, a
 * chain that has drifted from the real sums) are added addend by addend.  Reports, over the walks finished so far on this
 * context: chunks that took the slow way, chunks in all, and whether the context has gone back to the serial chain for the
 * current corpus (more than a quarter slow; PLSA_REF_CHAIN=pairs / serial pins either).  Same bits whichever way.  Waits for
 * the context's streams.  Any pointer may be NULL. */
int plsa_reference_chain_info(plsa_ctx *ctx, int64_t *slow_chunks, int64_t *chunks, int32_t *serial_now);

/* The materialised P array is placed by probing: up to PLSA_PLACEMENT_CANDIDATES (default 4)
 * allocations are streamed through once and the fastest is kept (HBM placement alone moves the
 * E-step by ~15 %).  Reports the last probe: candidates tried and the fill
 * bandwidth of the kept / the worst candidate (0 when no probing took place).                    */
int plsa_placement_info(plsa_ctx *ctx, int32_t *candidates, double *best_gbps, double *worst_gbps);

/* Schedule of the column pass for the current structure (diagnostics; bench.py reports it): the visiting list is
 * walked in chunks, XCD x takes the chunks [xcd_lo[x], xcd_lo[x+1]); the boundaries are MEASURED -- timed launches
 * of the pass itself, stretches resized until the eight XCDs finish together (csrc/plsa_hip.hip::ensure_balance).
 * xcd_end_us: per-XCD finish times of the last timed launch (0 when none ran: small corpora, PLSA_BALANCE=0).
 * Results never depend on the boundaries.  No counterpart in the reference (its loops are per-thread ranges of
 * numba.prange, enstop/plsa.py:91).  Any pointer may be NULL.                                               */
int plsa_schedule_info(plsa_ctx *ctx, int32_t *xcd_lo /*[9]*/, double *xcd_end_us /*[8]*/, int32_t *timed_launches,
                       int32_t *item_len, int64_t *n_items);

/* Index streams of the fused passes for the current structure: 1 = the packed entry stream (one 32-bit word per non-zero,
 * id | count << 24 with an escape to the float array), 0 = the (index, value) arrays (ineligible
 * stream, or PLSA_PACKED=0), -1 = not built yet.  csr: the document pass, csc: the column pass.  Any pointer may be NULL. */
int plsa_packed_info(plsa_ctx *ctx, int32_t *csr, int32_t *csc);

/* Lane shapes and gather widths of the fused passes for the factors in force (set_shape, table_is_wide in csrc/plsa_hip.hip):
 * col = {lpn, ch, full} of the column pass (also the E-step, the log-likelihood and the reductions), row = {lpn, ch, full} of
 * the document pass, full = (kp == 4 * lpn * ch); wide = {document pass, column pass}: 1 when that pass gathers its factor
 * table (P(w|z), m rows / P(z|d), n rows) with 64-bit row addresses (a table of 4 GB or more, or PLSA_FORCE_WIDE).  A wide
 * pass runs the run-time-kp instantiation whatever `full` says.  Tests read it to know which instantiations they reached.
 * Any pointer may be NULL; fails before plsa_set_factors. */
int plsa_pass_info(plsa_ctx *ctx, int32_t *col /*[3]*/, int32_t *row /*[3]*/, int32_t *wide /*[2]*/);

/* How the last plsa_fit / plsa_refit on this context ran, for tests that must know which loop and which column tail they
 * reached.  info = {fused loop, pipelined (column chain and document pass on two event-linked streams), speculated (the third
 * buffer set: an iteration enqueued ahead of an unread likelihood test), hipGraph launches, column tail (0 none ran, 1 the
 * single sweep k_col_reduce_norm, 2 the four-kernel form of the doc-sharded fit), two-stage norm_pwz (k_norm_reduce ran),
 * XCD split of the last column pass}.  A fit resets all seven when it starts; the last three are written by the column
 * pass and its tail themselves, so after plsa_m_step they describe that call's.  Changes no behaviour. */
int plsa_fit_info(plsa_ctx *ctx, int32_t *info /*[7]*/);

/* ---- measurement --------------------------------------------------------------------------------
 * HIP events on the context's own stream around every kernel launch (bench.py roofline figures).  */
int plsa_timing_enable(plsa_ctx *ctx, int32_t on);
int plsa_timing_reset(plsa_ctx *ctx);
/* total milliseconds and launch count of kernels whose name starts with `prefix`. */
int plsa_timing_get(plsa_ctx *ctx, const char *prefix, double *total_ms, int64_t *launches);
/* newline-separated "name launches total_ms" report into buf. */
int plsa_timing_report(plsa_ctx *ctx, char *buf, int64_t cap);
/* achievable streaming bandwidth of this device, GB/s, over `bytes` of scratch HBM:
 * kind 0 = fill with non-temporal stores, 1 = fill with plain stores, 2 = copy (bytes read + bytes
 * written counted), 3 = read-only stream (small sizes probe the L2 / Infinity-Cache service rate),
 * 4 / 5 / 6 = non-temporal fill in the E-step's store order (each wave writes 16 / 4 / 64 consecutive
 * 1-KB rows before moving on).
 * The practical ceiling the E-step's P write is compared with.   */
int plsa_measure_stream_bandwidth(plsa_ctx *ctx, int64_t bytes, int32_t kind, int32_t reps, double *gbps);

/* ---- host helper ---------------------------------------------------------------------------------
 * plsa_host_normalize_rows <- enstop/utils.py:8-41 normalize(ndarray, axis=1): float64, in place,
 *   sequential marginal, used by the factor initialisation (enstop/plsa.py:510-511, 980).          */
void plsa_host_normalize_rows(double *a, int64_t rows, int64_t cols);

/* plsa_host_mt19937_jump: advance a numpy.random.RandomState key (624 words) by 624 * 2^log2_blocks
 *   outputs with the jump polynomial the device initialisation uses (csrc/mt_jump.hpp); the position
 *   inside the block is unaffected by a whole-block jump.  Host-only (tests pin the polynomial
 *   arithmetic against NumPy without a GPU).  Returns 0, or 1 if log2_blocks is outside [0, 40].   */
int plsa_host_mt19937_jump(uint32_t *key /*[624]*/, int32_t log2_blocks);

/* synthetic bag-of-words CSR generated on the device (bench.py / large-size tests; not part of the
 * reference): lognormal document lengths, Zipf(s) word ids, the stored count of a (doc, word) pair is its
 * multiplicity among the document's token draws (a multinomial bag of words).  The result
 * becomes base + active matrix.  nnz_target is approximate; the exact nnz is returned.            */
int plsa_generate_synthetic(plsa_ctx *ctx, int64_t n, int64_t m, int64_t nnz_target, double zipf_s,
                            uint64_t seed, int64_t *nnz_out);
/* the same with TOPICAL structure (round 5; the corpus above draws every token independently -- no co-occurrence, unlike
 * text such as the reference's 20-Newsgroups, notebooks/EnsTop with 20-Newsgroups.ipynb:49): document d draws a topic
 * mixture theta_d ~ Dirichlet(alpha) over k0 latent topics, every topic has its own Zipf(s) ranking of the vocabulary,
 * a token comes from the shared ranking with probability `background` and otherwise from topic t ~ theta_d: the
 * generative model pLSA assumes.  1 <= k0 <= 256, alpha > 0, 0 <= background <= 1; deterministic in all arguments. */
int plsa_generate_synthetic_topics(plsa_ctx *ctx, int64_t n, int64_t m, int64_t nnz_target, double zipf_s,
                                   uint64_t seed, int32_t k0, double alpha, double background, int64_t *nnz_out);
/* ground truth of the topical corpus currently held as the base matrix: out[d] = the latent topic with the largest share
 * of document d's mixture theta_d (tests: does a fit recover the planted structure; experiments: document orderings). */
int plsa_synthetic_dominant_topics(plsa_ctx *ctx, int32_t *out /* [n], host */);

/* ---- tempered EM (plsa_hip_tempered.h) ---------------------------------------------------------------
 * The side tables of one tempered iteration at `beta` (0 < beta <= 1), formed from the current factors exactly as that
 * iteration forms them and read back in plsa_get_factors' layouts: U_out [n, k] = P(z|d)^beta, V_out [k, m] = P(w|z)^beta
 * (either may be NULL).  The factors stay as they are.  Tests need the exact bits of the tables.               */
int plsa_temper_factors(plsa_ctx *ctx, double beta, float *U_out, float *V_out);

/* ---- smoothed (MAP) EM --------------------------------------------------------------------------------
 * Declared here because include/ is closed to new files and the feature headers to new entries; these three are an
 * estimator, not a diagnostic, and move to a header of their own when that listing is next opened.  The reference has no
 * counterpart.
 *
 * Every fit of plsa_hip.h is a maximum-likelihood fit: a word a topic never saw gets P(w|z) = 0 exactly, and exact zeros are
 * absorbing under EM.  MAP estimation under Dirichlet priors adds a pseudo-count to every expected count before it is
 * normalised.  a >= 0 (document side) and b >= 0 (word side) are those counts, the Dirichlet concentrations minus one.  One
 * smoothed iteration is the ordinary E-step followed by
 *
 *   n_dz = sum_w x_dw P(z|w,d)            N_d = sum_z n_dz      (unweighted)        P(z|d) = (n_dz + a) / (N_d + k a)
 *   n_wz = sum_d sw_d x_dw P(z|w,d)       N_z = sum_w n_wz      (weighted)          P(w|z) = (n_wz + b) / (N_z + m b)
 *
 * which is EM on the log posterior
 *
 *   F = sum sw_d x_dw log sum_z P(w|z) P(z|d)  +  a sum_d sw_d sum_z log P(z|d)  +  b sum_z sum_w log P(w|z) .
 *
 * F does not decrease from one iteration to the next; it stands in the trace and in the stop test where plsa_fit has the
 * log-likelihood.  The fused passes are the ones plsa_fit runs: the document pass also hands back N_d, and k_smooth_rows
 * rewrites the P(z|d) = u it has just written as fmaf(u, N_d, (float)a) / (N_d + (float)(k a)); the column pass leaves n_wz
 * un-normalised, the existing norm kernels form N_z, and k_smooth_topics writes (n_wz + (float)b) / (float)(N_z + m b).
 * With a = 0 the document side is plsa_fit's, launch for launch and bit for bit; with b = 0 the word side is.  A document
 * without tokens gets 1 / k when a > 0.  The padding topics k .. kp - 1 stay exactly 0.
 *
 * One stream, no look-ahead buffer set, no hipGraph.  norm_pdz [n] and the partial sums of the log prior belong to the
 * context: kept between calls, freed by plsa_release_scratch and plsa_destroy.
 *
 * Each of these is a status code and a message, and launches nothing: a or b negative, NaN or infinite; flags without
 * PLSA_FUSED; flags with PLSA_SHARDED, PLSA_GRAPH, PLSA_REFERENCE_SUMS or PLSA_REFERENCE_LL; a context in reference
 * arithmetic (plsa_set_arithmetic), or one that is a shard of a communicator (plsa_comm_init).
 *
 * plsa_fit_smoothed: plsa_fit's arguments, loop and stop rule, with the pseudo-counts after sw; the trace holds F.
 * a == 0 and b == 0 calls plsa_fit with the same arguments and does nothing else. */
int plsa_fit_smoothed(plsa_ctx *ctx, const float *sw /* [n] or NULL */, double a, double b, int32_t n_iter, int32_t n_iter_per_test,
                      double tolerance, float thresh, int32_t flags, int32_t *iters_done, float *ll_trace, int32_t *n_ll);
/* plsa_refit's arguments, loop and stop rule with the document-side pseudo-count after sw: only P(z|d) moves, the topics are
 * never written, and the trace holds F without its word-side term (a constant there).  a == 0 calls plsa_refit. */
int plsa_refit_smoothed(plsa_ctx *ctx, const float *sw /* [n] or NULL */, double a, int32_t n_iter, int32_t n_iter_per_test,
                        double tolerance, float thresh, int32_t flags, int32_t *iters_done, float *ll_trace, int32_t *n_ll);
/* *out = F of the factors in force (one double).  The likelihood is plsa_log_likelihood's; each prior term is summed in float64
 * over a fixed number of slabs of rows, so its bits do not depend on the launch geometry.  A term whose pseudo-count is 0 is
 * neither launched nor added: at a = b = 0 the result has the bits of plsa_log_likelihood.  A factor entry equal to 0 adds
 * nothing to a prior term (it can only stand in starting factors the caller supplied). */
int plsa_log_posterior(plsa_ctx *ctx, const float *sw /* [n] or NULL */, double a, double b, double *out);

/*
 * ---- variational Bayes LDA: four entry points in a section of their own, like smoothed EM above ----
 *
 * Latent Dirichlet allocation by batch variational Bayes (Blei, Ng, Jordan 2003; the batch form of Hoffman, Blei, Bach 2010,
 * which scikit-learn's LatentDirichletAllocation follows).  The reference has no counterpart.
 *
 * The state is gamma [n, k] > 0 (the Dirichlet parameters of the document mixtures) and lambda [k, m] > 0 (those of the
 * topics).  It lives where P(z|d) and P(w|z) live: plsa_set_factors puts a state on the context, plsa_get_factors reads it
 * back, plsa_factors_snapshot and plsa_factors_restore work on it -- none of them normalises.  With
 *
 *   A_dz = exp(psi(gamma_dz) - psi(sum_z gamma_dz))          B_zw = exp(psi(lambda_zw) - psi(sum_w lambda_zw))
 *
 * the optimal responsibilities are phi_dwz = A_dz B_zw / sum_z' A_dz' B_z'w, and one iteration is
 *
 *   gamma_dz = alpha + sum_w x_dw phi_dwz                      lambda_zw = eta + sum_d x_dw phi_dwz
 *
 * with both sums taken under the SAME tables: given phi the bound separates in gamma and lambda, so this is exact coordinate
 * ascent and the bound never decreases.  Any priors alpha, eta > 0 are legal, the sparse regime below 1 included, which
 * plsa_fit_smoothed (pseudo-counts >= 0, concentrations >= 1) cannot express.
 *
 * The tables: every entry is evaluated in float64 (a digamma by recurrence to x >= 6 and a twelve-term asymptotic series,
 * absolute error below 2^-40 wherever psi(x) >= -88) and rounded to float32 once.  The row sums of gamma are float64 sums of
 * the stored float32 entries, the topic sums of lambda float64 slab sums added in slab order.
 *
 * float32 ends at exp(-87), and psi(0.01) is -100.6: an entry at a prior below about 0.012 is below the float32 normal range.
 * The responsibilities do not change when a document's row of A or a word's row of B (its k entries) is multiplied by a
 * constant, so the passes run on SCALED tables: every such row is divided by its largest entry, in the exponent
 * (exp(psi(x) - psi(S) - shift), shift the logarithm of the row's largest entry, float64).  The largest entry of every such row is 1;
 * an entry that still leaves float32 is below 1e-38 of the largest entry of its row and may be flushed to 0.  This holds for
 * each table alone, NOT for the products the passes and k_loglik form: with both priors around 0.01, a token whose document
 * peaks on one topic and whose word peaks on another can have every product A_dz B_zw below float32.  Such a token drops out of
 * the counts and the bound is -inf: priors that small are legal, but a state that far apart is outside what float32 tables hold.  The bound's likelihood term gets sum x_dw (shift_d + shift_w) back, a float64 sum.  thresh is compared with the
 * products of the scaled tables.  plsa_lda_tables reads the tables of the definition, unscaled.
 *
 * One stream, no look-ahead buffer set, no hipGraph: the launch chain of an iteration is k_lda_rowsum, k_lda_topic_partial,
 * k_lda_topic_sums, k_lda_wordmax, k_lda_tables (twice), k_row_pass<fused>, k_col_pass<fused>, k_col_reduce, k_lda_rows and k_lda_topics on
 * the context's stream.  The passes are the ones plsa_fit runs.
 *
 * The bound (what the trace holds and the stop test sees, where plsa_fit has the log-likelihood):
 *
 *   L = sum x_dw log sum_z A_dz B_zw
 *     + sum_d [lgamma(k alpha) - k lgamma(alpha) - lgamma(S_d) + sum_z (lgamma(gamma_dz) + (alpha - gamma_dz)(psi(gamma_dz) - psi(S_d)))]
 *     + sum_z [lgamma(m eta) - m lgamma(eta) - lgamma(S_z) + sum_w (lgamma(lambda_zw) + (eta - lambda_zw)(psi(lambda_zw) - psi(S_z)))]
 *
 * for any gamma, lambda > 0 with phi at its optimum (scikit-learn's _approx_bound).  The likelihood term is k_loglik on the
 * scaled tables plus the shifts (k_lda_shift_sum); the Dirichlet sums and the shift sum are float64 slab partials added in a
 * fixed order (k_lda_bound, k_ll_final), whose bits do not depend on the launch geometry.  A state entry equal to 0 adds nothing to a table or to the bound.
 *
 * There are no sample weights: weights made resident by plsa_set_sample_weight are not applied.
 *
 * Each of these is a status code and a message, and launches nothing: a prior that is not a finite number > 0 (NaN
 * included); doc_iter < 1; flags without PLSA_FUSED; flags with PLSA_SHARDED, PLSA_GRAPH, PLSA_REFERENCE_SUMS or
 * PLSA_REFERENCE_LL; a context in reference arithmetic (plsa_set_arithmetic); a context that is a shard of a communicator.
 *
 * The side tables, the sums and the bound's scratch belong to the context: 4 kp (n + m) bytes and change, kept between calls,
 * freed by plsa_release_scratch and plsa_destroy.
 */
/* n_iter iterations from the state on the context, with plsa_fit's loop and stop rule on the bound: the bound of the initial
 * state, then one after every n_iter_per_test-th iteration, the stop on its relative change against `tolerance` (0 never stops
 * on it).  doc_iter >= 1: the first doc_iter - 1 rounds of an iteration update gamma alone against the unchanged B, the last
 * round updates both from the same tables.  thresh: the passes' threshold on a product A_dz B_zw, as in plsa_fit.  flags:
 * PLSA_FUSED is required; PLSA_TRACE_LL and PLSA_STOP_NO_ZERO_ARM mean what they mean in plsa_fit.  iters_done, bound_trace,
 * n_bound: plsa_fit's iters_done, ll_trace, n_ll. */
int plsa_lda_fit(plsa_ctx *ctx, double alpha, double eta, int32_t n_iter, int32_t n_iter_per_test, double tolerance,
                 int32_t doc_iter, float thresh, int32_t flags, int32_t *iters_done, float *bound_trace, int32_t *n_bound);

/* The fold-in: gamma alone moves, lambda is never written.  Every iteration is doc_iter gamma rounds against the B of the
 * lambda on the context; the bound of the trace is the likelihood term and the document part (the topic part is a constant
 * there).  Loop and stop rule of plsa_refit. */
int plsa_lda_refit(plsa_ctx *ctx, double alpha, int32_t n_iter, int32_t n_iter_per_test, double tolerance, int32_t doc_iter,
                   float thresh, int32_t flags, int32_t *iters_done, float *bound_trace, int32_t *n_bound);

/* The bound of the state in force, float64; with_topics == 0 leaves the topic part out (eta is then not read). */
int plsa_lda_bound(plsa_ctx *ctx, double alpha, double eta, int32_t with_topics, double *out);

/* Diagnostic read-back, like plsa_temper_factors: the tables A [n, k] and B [k, m] an iteration would form from the state in
 * force, which stays as it is.  Either pointer may be NULL. */
int plsa_lda_tables(plsa_ctx *ctx, float *A_out, float *B_out);

#ifdef __cplusplus
}
#endif
#endif /* PLSA_HIP_DIAG_H */
