// plsa_smoothed.hpp -- host side of smoothed (MAP) EM: plsa_fit_smoothed, plsa_refit_smoothed and plsa_log_posterior
// (include/plsa_hip_diag.h); part of plsa_hip.hip's translation unit (included at its end: it uses the
// context, the pass wrappers, plsa_fit and plsa_refit).
//
// A smoothed iteration is the launch chain of an unsharded fused iteration with the pseudo-counts added behind the passes,
// which stay untouched: run_row_pass hands norm_pdz back, k_smooth_rows rewrites the P(z|d) the pass has just written;
// run_col_pass(parts 3) leaves the un-normalised P(w|z) sums in Vacc, run_vacc_norm forms norm_pwz from them, k_smooth_topics
// writes the new P(w|z).  A side whose pseudo-count is 0 runs the ordinary chain of that side, so it keeps its bits.  One
// stream, no look-ahead buffers, no hipGraph; every value of the trace is k_loglik on the factors plus the log prior
// (k_log_prior), the objective the iteration does not decrease.  The call around the loops is the frame of plsa_drivers.hpp.
#pragma once

namespace {

// U[out_u] <- (U[out_u] * N_d + a) / (N_d + k a) behind a document pass that left N_d in c->smoothed.norm_pdz
int run_smooth_rows(plsa_ctx *c, double a) {
    const int kq = c->kp / 4;
    const i64 n4 = c->n * kq;
    Scope s(c, "k_smooth_rows");
    hipLaunchKernelGGL(plsa::k_smooth_rows, dim3(plsa::plan::smooth_grid(n4, c->grid_cap)), dim3(plsa::plan::SMOOTH_BLOCK), 0, c->ls,
                       c->U[out_u(c)].as<float4>(), c->smoothed.norm_pdz.as<float>(), (long long)n4, kq, c->k, (float)a,
                       (float)(c->k * a));
    return launch_check(c, "k_smooth_rows");
}

// Vt[out_v] <- (Vacc + b) / (norm_pwz + m b) behind run_col_pass(parts 3): norm_pwz from Vacc by the existing norm kernels
int run_smooth_topics(plsa_ctx *c, double b) {
    CHK(run_vacc_norm(c));
    const int kq = c->kp / 4;
    const i64 n4 = c->m * kq;
    Scope s(c, "k_smooth_topics");
    hipLaunchKernelGGL(plsa::k_smooth_topics, dim3(plsa::plan::smooth_grid(n4, c->grid_cap)), dim3(plsa::plan::SMOOTH_BLOCK),
                       sizeof(float) * (size_t)c->kp, c->ls, c->Vacc.as<float4>(), c->Vt[out_v(c)].as<float4>(), (long long)n4, kq,
                       c->k, c->norm_pwz.as<float>(), (float)b, (double)c->m * b);
    return launch_check(c, "k_smooth_topics");
}

// c->smoothed.out[slot] <- sum of coef * w[row] * log(table) over the topics below k: one partial per slab, added in order
int run_log_prior(plsa_ctx *c, const DevBuf &table, i64 rows, const float *d_w, double coef, int slot) {
    plsa_ctx::Smoothed &sm = c->smoothed;
    CHK(ensure(c, sm.partials, sizeof(double) * 2 * plsa::plan::PRIOR_SLABS));
    CHK(ensure(c, sm.out, sizeof(double) * 2));
    const int slabs = plsa::plan::prior_grid(rows);
    double *partials = sm.partials.as<double>() + (size_t)slot * plsa::plan::PRIOR_SLABS;
    {
        Scope s(c, "k_log_prior");
        hipLaunchKernelGGL(plsa::k_log_prior, dim3(slabs), dim3(plsa::plan::SMOOTH_BLOCK), 0, c->stream, table.as<float4>(),
                           (long long)rows, c->kp / 4, c->k, d_w, coef, partials);
    }
    {
        Scope s(c, "k_ll_final");
        hipLaunchKernelGGL(plsa::k_ll_final, dim3(1), dim3(256), 0, c->stream, partials, slabs, sm.out.as<double>() + slot);
    }
    return launch_check(c, "k_log_prior");
}

// F = log-likelihood + a sum_d sw_d sum_z log P(z|d) + b sum_z sum_w log P(w|z) of the current factors; a term whose
// pseudo-count is 0 is neither launched nor added, so F(0, 0) has the bits of run_loglik
int run_log_posterior(plsa_ctx *c, const float *d_sw, double a, double b, double *out) {
    plsa_ctx::Smoothed &sm = c->smoothed;
    // the prior sums land in a page-locked slot of the context, as the likelihood does in h_ll: whichever way this function is
    // left, a copy still on its way writes to memory that outlives the call
    if (!sm.h_out && host_alloc(sm.h_out, 2) != hipSuccess) return fail(c, "plsa_log_posterior: page-locked buffer allocation failed");
    double *prior = sm.h_out.get();
    if (a > 0.0) CHK(run_log_prior(c, c->U[c->cu], c->n, d_sw, a, 0));
    if (b > 0.0) CHK(run_log_prior(c, c->Vt[c->cv], c->m, nullptr, b, 1));
    if (a > 0.0) HIPCHK(c, hipMemcpyAsync(&prior[0], sm.out.as<double>(), sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (b > 0.0) HIPCHK(c, hipMemcpyAsync(&prior[1], sm.out.as<double>() + 1, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    double ll = 0.0;
    CHK(run_loglik(c, d_sw, &ll));       // waits for c->stream: the priors have arrived as well
    if (a > 0.0) ll += prior[0];
    if (b > 0.0) ll += prior[1];
    *out = ll;
    return 0;
}

// the reference's loop (fit::run_materialised) over smoothed iterations.  update_v = false: the refit -- the document side
// only, the topics are never written (the word-side prior is a constant there: not in F)
struct SmoothedBackend {
    plsa_ctx *c;
    const float *d_sw, *d_sw_m;
    float thresh;
    double a, b;
    bool update_v;
    int loglik(double *f) { return run_log_posterior(c, d_sw, a, update_v ? b : 0.0, f); }
    int iteration() {
        float *d_norm_pdz = nullptr;
        if (a > 0.0) {
            CHK(ensure(c, c->smoothed.norm_pdz, sizeof(float) * (size_t)c->n));
            d_norm_pdz = c->smoothed.norm_pdz.as<float>();
        }
        CHK(run_row_pass(c, false, false, d_sw, thresh, d_norm_pdz, nullptr));
        if (a > 0.0) CHK(run_smooth_rows(c, a));
        if (update_v && b > 0.0) {
            CHK(run_col_pass(c, false, d_sw_m, thresh, 3));
            CHK(run_smooth_topics(c, b));
        } else if (update_v) {
            CHK(run_col_pass(c, false, d_sw_m, thresh, 1));
            CHK(run_col_tail(c));
        }
        c->cu ^= 1;
        if (update_v) c->cv ^= 1;
        return 0;
    }
};

int smoothed_count_ok(plsa_ctx *c, const char *who, const char *name, double v) {
    if (!(v >= 0.0) || !std::isfinite(v)) return fail(c, "%s: pseudo-count %s=%g is not a finite number >= 0", who, name, v);
    return 0;
}

int smoothed_context_ok(plsa_ctx *c, const char *who) {
    if (c->ref_sums || c->ref_ll) return plain_fused_refusal(c, who, "smoothed", PlainFused::REFERENCE_CONTEXT);
    if (c->comm) return fail(c, "%s: the context is a shard of a communicator (plsa_comm_init); smoothed EM has no multi-GPU form", who);
    return 0;
}

int smoothed_eligible(plsa_ctx *c, const char *who, double a, double b, int flags) {
    CHK(smoothed_count_ok(c, who, "a", a));
    CHK(smoothed_count_ok(c, who, "b", b));
    CHK(plain_fused_refusal(c, who, "smoothed", plain_fused(c, flags), flags));
    return smoothed_context_ok(c, who);
}

}  // namespace

extern "C" {

int plsa_fit_smoothed(plsa_ctx *c, const float *sw, double a, double b, int32_t n_iter, int32_t n_iter_per_test, double tolerance,
                      float thresh, int32_t flags, int32_t *iters_done, float *ll_trace, int32_t *n_ll) {
    CHK(smoothed_eligible(c, "plsa_fit_smoothed", a, b, flags));
    if (a == 0.0 && b == 0.0) return plsa_fit(c, sw, n_iter, n_iter_per_test, tolerance, thresh, flags, iters_done, ll_trace, n_ll);
    const FitCall call{sw, n_iter, n_iter_per_test, tolerance, flags, iters_done, ll_trace, n_ll};
    CHK(fit_open(c, "plsa_fit_smoothed", call));
    return fit_run(c, call, fit_rule(flags), true, [&](FitRun &r) {
        SmoothedBackend backend{c, r.d_sw, r.d_sw_m, thresh, a, b, true};
        return plsa::fit::run_materialised(backend, r.tests, n_iter, r.trace, &r.iters);
    });
}

int plsa_refit_smoothed(plsa_ctx *c, const float *sw, double a, int32_t n_iter, int32_t n_iter_per_test, double tolerance,
                        float thresh, int32_t flags, int32_t *iters_done, float *ll_trace, int32_t *n_ll) {
    CHK(smoothed_eligible(c, "plsa_refit_smoothed", a, 0.0, flags));
    if (a == 0.0) return plsa_refit(c, sw, n_iter, n_iter_per_test, tolerance, thresh, flags, iters_done, ll_trace, n_ll);
    const FitCall call{sw, n_iter, n_iter_per_test, tolerance, flags, iters_done, ll_trace, n_ll};
    CHK(fit_open(c, "plsa_refit_smoothed", call));
    return fit_run(c, call, plsa::fit::REFIT, true, [&](FitRun &r) {
        SmoothedBackend backend{c, r.d_sw, nullptr, thresh, a, 0.0, false};
        return plsa::fit::run_materialised(backend, r.tests, n_iter, r.trace, &r.iters);
    });
}

int plsa_log_posterior(plsa_ctx *c, const float *sw, double a, double b, double *out) {
    CHK(smoothed_count_ok(c, "plsa_log_posterior", "a", a));
    CHK(smoothed_count_ok(c, "plsa_log_posterior", "b", b));
    CHK(smoothed_context_ok(c, "plsa_log_posterior"));
    if (!out) return fail(c, "plsa_log_posterior: out is NULL");
    const float *d_sw = nullptr;
    CHK(open_weighted(c, sw, &d_sw));
    return run_log_posterior(c, d_sw, a, b, out);
}

}  // extern "C"
