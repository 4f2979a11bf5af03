// plsa_lda_priors.hpp -- host side of LDA with a vector document-topic prior and learned priors: plsa_lda_prior_fit,
// plsa_lda_prior_refit, plsa_lda_prior_bound and plsa_lda_prior_stats (enstop_amd/include/plsa_hip_lda_priors.h, DESIGN.md
// section 20); part of plsa_hip.hip's translation unit (included at its end, behind plsa_lda.hpp: it uses its tables, its
// topic side, its round, its bound, and the call frame of plsa_drivers.hpp).
//
// The prior vector lives on the device twice, float64 [kp] for the bound and float32 [kp] for k_lda_rows_v (0 at the pads),
// sent from a page-locked slot that also receives the sums T_z of a prior update.  An update runs behind a round: the tables
// of the new state are formed (the next iteration would form them anyway: the validity flags make that free), k_lda_logmean
// and k_lda_logmean_sums leave T on the device, the host waits for 2 kp doubles and runs the Newton iterations of
// plsa_lda_prior_math.hpp.  One stream, no look-ahead buffers, no hipGraph.
#pragma once

namespace {

// the page-locked slot: T of gamma [kp], T of lambda [kp], alpha float64 [kp], alpha float32 [kp] (the last two in the layout of
// the device buffer)
int lda_prior_slot(plsa_ctx *c) {
    plsa_ctx::LdaPrior &p = c->lda_prior;
    if (p.h && p.h_kp >= c->kp) return 0;
    if (host_alloc(p.h, (size_t)4 * c->kp) != hipSuccess) return fail(c, "plsa_lda_prior: page-locked buffer allocation failed");
    p.h_kp = c->kp;
    return 0;
}

double *lda_prior_alpha64(plsa_ctx *c) { return c->lda_prior.alpha.as<double>(); }
float4 *lda_prior_alpha32(plsa_ctx *c) { return reinterpret_cast<float4 *>(c->lda_prior.alpha.as<double>() + c->kp); }

// alpha [k] onto the device.  The slot is free: every earlier copy out of it was followed by a wait for the stream
int lda_prior_send(plsa_ctx *c, const double *alpha) {
    plsa_ctx::LdaPrior &p = c->lda_prior;
    CHK(lda_prior_slot(c));
    CHK(ensure(c, p.alpha, (sizeof(double) + sizeof(float)) * (size_t)c->kp));
    double *a64 = p.h.get() + 2 * (size_t)c->kp;
    float *a32 = reinterpret_cast<float *>(a64 + c->kp);
    for (int z = 0; z < c->kp; ++z) {
        a64[z] = z < c->k ? alpha[z] : 0.0;
        a32[z] = (float)a64[z];
    }
    HIPCHK(c, hipMemcpyAsync(p.alpha.p, a64, (sizeof(double) + sizeof(float)) * (size_t)c->kp, hipMemcpyHostToDevice, c->stream));
    return 0;
}

// U[out_u] <- U[out_u] * N_d + alpha_z behind a document pass that left N_d in c->lda.norm_pdz
int run_lda_rows_v(plsa_ctx *c) {
    const int kq = c->kp / 4;
    const i64 n4 = c->n * kq;
    Scope s(c, "k_lda_rows_v");
    hipLaunchKernelGGL(plsa::k_lda_rows_v, dim3(plsa::plan::lda_grid(n4, c->grid_cap)), dim3(plsa::plan::LDA_BLOCK), 0, c->ls,
                       c->U[out_u(c)].as<float4>(), c->lda.norm_pdz.as<float>(), (long long)n4, kq, c->k, lda_prior_alpha32(c));
    return launch_check(c, "k_lda_rows_v");
}

// c->lda.out[0] <- the Dirichlet part of the bound of gamma under the vector prior (without its constant)
int run_lda_dirichlet_v(plsa_ctx *c) {
    plsa_ctx::Lda &l = c->lda;
    const int slabs = plsa::plan::lda_bound_grid(c->n);
    double *partials = l.partials.as<double>();
    {
        Scope s(c, "k_lda_bound_v");
        hipLaunchKernelGGL(plsa::k_lda_bound_v, dim3(slabs), dim3(plsa::plan::LDA_BLOCK), 0, c->stream, c->U[c->cu].as<float4>(),
                           (long long)c->n, c->kp / 4, c->k, lda_prior_alpha64(c), lda_sums(c, LDA_S_DOC), lda_sums(c, LDA_PSI_DOC),
                           partials);
    }
    {
        Scope s(c, "k_ll_final");
        hipLaunchKernelGGL(plsa::k_ll_final, dim3(1), dim3(256), 0, c->stream, partials, slabs, l.out.as<double>());
    }
    return launch_check(c, "k_lda_bound_v");
}

// run_lda_bound with the vector prior on the device (lda_prior_send) and in alpha [k]: the document constant is
// lgamma(sum alpha) - sum lgamma(alpha_z)
int run_lda_bound_v(plsa_ctx *c, const double *alpha, double eta, bool with_topics, double *out) {
    CHK(lda_bound_send(c, "plsa_lda_prior_bound", [c] { return run_lda_dirichlet_v(c); }, eta, with_topics));
    double sum = 0.0, each = 0.0;
    for (int z = 0; z < c->k; ++z) { sum += alpha[z]; each += lgamma(alpha[z]); }
    return lda_bound_finish(c, lgamma(sum) - each, eta, with_topics, out);
}

// slot T (0: gamma, BY_ROW; 1: lambda) of c->lda_prior.t [2][kp] <- the sums of psi(entry) - psi(S) per topic, from the sums of
// the tables in force (run_lda_table_u / run_lda_table_v have run)
template <bool BY_ROW>
int run_lda_logmean(plsa_ctx *c) {
    plsa_ctx::LdaPrior &p = c->lda_prior;
    const i64 rows = BY_ROW ? c->n : c->m;
    const int slabs = plsa::plan::lda_logmean_grid(rows);
    CHK(ensure(c, p.partials, sizeof(double) * (size_t)plsa::plan::lda_logmean_grid(std::max(c->n, c->m)) * c->kp));
    CHK(ensure(c, p.t, sizeof(double) * 2 * (size_t)c->kp));
    {
        Scope s(c, "k_lda_logmean");
        hipLaunchKernelGGL(plsa::k_lda_logmean<BY_ROW>, dim3(slabs), dim3(plsa::plan::LDA_BLOCK), 0, c->ls,
                           (BY_ROW ? c->U[c->cu] : c->Vt[c->cv]).as<float>(), (long long)rows, c->kp, c->k,
                           lda_sums(c, BY_ROW ? LDA_S_DOC : LDA_S_TOPIC), lda_sums(c, BY_ROW ? LDA_PSI_DOC : LDA_PSI_TOPIC),
                           p.partials.as<double>());
    }
    {
        Scope s(c, "k_lda_logmean_sums");
        hipLaunchKernelGGL(plsa::k_lda_logmean_sums, dim3(plsa::plan::lda_topic_grid(c->kp)), dim3(plsa::plan::LDA_BLOCK), 0, c->ls,
                           p.partials.as<double>(), slabs, c->kp, c->k, p.t.as<double>() + (BY_ROW ? 0 : c->kp));
    }
    return launch_check(c, "k_lda_logmean");
}

// the sums of the state in force into the page-locked slot (docs: [0, kp), topics: [kp, 2 kp)), waited for
int run_lda_prior_stats(plsa_ctx *c, bool docs, bool topics) {
    plsa_ctx::LdaPrior &p = c->lda_prior;
    if (!docs && !topics) return 0;
    CHK(lda_prior_slot(c));
    if (docs) { CHK(run_lda_table_u(c)); CHK(run_lda_logmean<true>(c)); }
    if (topics) { CHK(run_lda_table_v(c)); CHK(run_lda_logmean<false>(c)); }
    // the halves that were formed, and nothing else: [first, first + count) of the 2 kp doubles
    const size_t first = docs ? 0 : (size_t)c->kp, count = (size_t)c->kp * ((docs ? 1 : 0) + (topics ? 1 : 0));
    HIPCHK(c, hipMemcpyAsync(p.h.get() + first, p.t.as<double>() + first, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// LdaBackend with the vector prior -- its own: the alpha vector, the rows step, the prior update
struct LdaPriorBackend {
    plsa_ctx *c;
    float thresh;
    std::vector<double> alpha;
    double eta;
    int doc_iter;
    bool update_v;
    int loglik(double *f) { return run_lda_bound_v(c, alpha.data(), eta, update_v, f); }
    int iteration() {
        return lda_rounds(c, thresh, [this] { return run_lda_rows_v(c); }, update_v ? LdaColumns::TOPICS : LdaColumns::NONE, eta)
            .iteration(doc_iter);
    }
    // alpha (learn bit 0) and eta (bit 1) <- the maximisers of the bound at the state in force
    int update_priors(int learn) {
        CHK(run_lda_prior_stats(c, (learn & 1) != 0, (learn & 2) != 0));
        const double *t = c->lda_prior.h.get();
        if (learn & 1) {
            plsa::lda::maximise_alpha(alpha.data(), t, c->k, (double)c->n);
            CHK(lda_prior_send(c, alpha.data()));
        }
        if (learn & 2) {
            double total = 0.0;
            for (int z = 0; z < c->k; ++z) total += t[c->kp + z];
            plsa::lda::maximise_eta(&eta, total, (double)c->k, (double)c->m);
        }
        return 0;
    }
};

// fit::run_materialised with the prior updates behind the iterations the schedule names (plan::prior_due), before the test
// that may be due there.  While a prior is learned, a test is recorded but cannot stop the loop before the first update.
int run_lda_prior_loop(LdaPriorBackend &b, plsa::fit::Tests &t, int n_iter, bool trace, int learn, int prior_start, int prior_every,
                       int *iters) {
    double f = 0.0;
    CHK(b.loglik(&f));
    t.initial(f);
    for (int i = 0; i < n_iter; ++i) {
        CHK(b.iteration());
        ++*iters;
        if (learn && plsa::plan::prior_due(i + 1, prior_start, prior_every)) CHK(b.update_priors(learn));
        if (t.due_after(i)) {
            if (i == n_iter - 1 && !trace) break;
            CHK(b.loglik(&f));
            if (t.test(f)) {
                if (!(learn && i + 1 < prior_start)) break;
                t.prev = (float)f;                               // the verdict is set aside: the next test compares with this bound
            }
        }
    }
    return 0;
}

int lda_prior_vector_ok(plsa_ctx *c, const char *who, const double *alpha) {
    if (!alpha) return fail(c, "%s: alpha is NULL", who);
    for (int z = 0; z < c->k; ++z) CHK(lda_prior_ok(c, who, "alpha", alpha[z]));
    return 0;
}

int lda_prior_eligible(plsa_ctx *c, const char *who, const double *alpha, double eta, int doc_iter, int flags) {
    CHK(lda_prior_vector_ok(c, who, alpha));
    return lda_eligible(c, who, 1.0, eta, doc_iter, flags);
}

}  // namespace

extern "C" {

int plsa_lda_prior_fit(plsa_ctx *c, double *alpha, double *eta, int32_t learn, int32_t prior_start, int32_t prior_every,
                       int32_t n_iter, int32_t n_iter_per_test, double tolerance, int32_t doc_iter, float thresh, int32_t flags,
                       int32_t *iters_done, float *bound_trace, int32_t *n_bound) {
    const char *who = "plsa_lda_prior_fit";
    if (!eta) return fail(c, "%s: eta is NULL", who);
    CHK(lda_prior_eligible(c, who, alpha, *eta, doc_iter, flags));
    if (learn < 0 || learn > 3) return fail(c, "%s: learn=%d is not in 0 .. 3 (bit 0 alpha, bit 1 eta)", who, learn);
    if (prior_start < 1) return fail(c, "%s: prior_start=%d is not >= 1", who, prior_start);
    if (prior_every < 1) return fail(c, "%s: prior_every=%d is not >= 1", who, prior_every);
    const FitCall call{nullptr, n_iter, n_iter_per_test, tolerance, flags, iters_done, bound_trace, n_bound};
    CHK(fit_open(c, who, call));
    lda_open(c);
    CHK(lda_prior_send(c, alpha));
    LdaPriorBackend backend{c, thresh, std::vector<double>(alpha, alpha + c->k), *eta, doc_iter, true};
    CHK(fit_run(c, call, fit_rule(flags), true, [&](FitRun &r) {
        return run_lda_prior_loop(backend, r.tests, n_iter, r.trace, learn, prior_start, prior_every, &r.iters);
    }));
    std::copy(backend.alpha.begin(), backend.alpha.end(), alpha);
    *eta = backend.eta;
    return 0;
}

int plsa_lda_prior_refit(plsa_ctx *c, const double *alpha, int32_t n_iter, int32_t n_iter_per_test, double tolerance,
                         int32_t doc_iter, float thresh, int32_t flags, int32_t *iters_done, float *bound_trace, int32_t *n_bound) {
    const char *who = "plsa_lda_prior_refit";
    CHK(lda_prior_eligible(c, who, alpha, 1.0, doc_iter, flags));
    const FitCall call{nullptr, n_iter, n_iter_per_test, tolerance, flags, iters_done, bound_trace, n_bound};
    CHK(fit_open(c, who, call));
    lda_open(c);
    CHK(lda_prior_send(c, alpha));
    LdaPriorBackend backend{c, thresh, std::vector<double>(alpha, alpha + c->k), 1.0, doc_iter, false};
    return fit_run(c, call, plsa::fit::REFIT, true, [&](FitRun &r) {
        return run_lda_prior_loop(backend, r.tests, n_iter, r.trace, 0, 1, 1, &r.iters);
    });
}

int plsa_lda_prior_bound(plsa_ctx *c, const double *alpha, double eta, int32_t with_topics, double *out) {
    const char *who = "plsa_lda_prior_bound";
    CHK(lda_prior_vector_ok(c, who, alpha));
    if (with_topics) CHK(lda_prior_ok(c, who, "eta", eta));
    CHK(lda_context_ok(c, who));
    if (!out) return fail(c, "%s: out is NULL", who);
    HIPCHK(c, hipSetDevice(c->device));
    CHK(need_factors(c));
    lda_open(c);
    CHK(lda_prior_send(c, alpha));
    return run_lda_bound_v(c, alpha, eta, with_topics != 0, out);
}

int plsa_lda_prior_stats(plsa_ctx *c, double *t_doc, double *t_topic) {
    CHK(lda_context_ok(c, "plsa_lda_prior_stats"));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(need_factors(c));
    lda_open(c);
    CHK(run_lda_prior_stats(c, t_doc != nullptr, t_topic != nullptr));
    const double *t = c->lda_prior.h.get();
    if (t_doc) std::copy(t, t + c->k, t_doc);
    if (t_topic) std::copy(t + c->kp, t + c->kp + c->k, t_topic);
    lda_open(c);                                         // (the scaled tables of a diagnostic call are nobody's)
    return 0;
}

}  // extern "C"
