// plsa_lda.hpp -- host side of variational Bayes LDA: plsa_lda_fit, plsa_lda_refit, plsa_lda_bound and plsa_lda_tables
// (include/plsa_hip_diag.h); part of plsa_hip.hip's translation unit (included at its end: it uses the
// context, the pass wrappers and the call frame of plsa_drivers.hpp).
//
// The state lives in the factor buffers: gamma [n, kp] in U[cu], lambda [m, kp] in Vt[cv].  An iteration forms the two
// exp-digamma tables A, B into side tables of the context (every document's row of A and every word's row of B scaled to a
// largest entry of 1, which leaves the responsibilities as they are and keeps the tables inside float32), runs the launch chain of an unsharded fused iteration with the side
// tables standing in for the factors (StandIn) -- run_row_pass handing norm_pdz back, run_col_pass(parts 3) leaving the raw
// counts in Vacc -- and adds the priors behind the passes (k_lda_rows, k_lda_topics).  Both updates come from the same
// responsibilities, so the bound (run_lda_bound) never decreases.  One stream, no look-ahead buffers, no hipGraph.
//
// Three pieces are here once for every form of LDA -- the vector and learned priors of plsa_lda_priors.hpp and the online step
// and fold of plsa_lda_online.hpp enter them with their own parameters: the topic-side table chain (run_lda_topic_tables), the
// round (LdaRounds) and the bound in an enqueue half and a finish half (lda_bound_send, lda_bound_finish).
#pragma once

namespace {

// the float64 side arrays of the tables in force: per document S_d, psi(S_d) and the shift of its row of A; per topic S_z and
// psi(S_z); per word the shift of its row of B
enum LdaSum { LDA_S_DOC, LDA_PSI_DOC, LDA_SHIFT_DOC, LDA_S_TOPIC, LDA_PSI_TOPIC, LDA_SHIFT_WORD };

double *lda_sums(plsa_ctx *c, LdaSum which) {
    const size_t n = (size_t)c->n, kp = (size_t)c->kp;
    const size_t at[6] = {0, n, 2 * n, 3 * n, 3 * n + kp, 3 * n + 2 * kp};
    return c->lda.sums.as<double>() + at[which];
}

int lda_ensure_sums(plsa_ctx *c) {
    return ensure(c, c->lda.sums, sizeof(double) * (3 * (size_t)c->n + 2 * (size_t)c->kp + (size_t)c->m));
}

// A <- exp(psi(gamma) - psi(S_d) - shift_d) from U[cu], shift_d the logarithm of the largest entry of document d's row (scaled;
// otherwise no shift: the tables of the definition, for plsa_lda_tables), with S_d, psi(S_d) and shift_d left in the context
int run_lda_table_u(plsa_ctx *c, bool scaled = true) {
    plsa_ctx::Lda &l = c->lda;
    if (l.a_valid && scaled) return 0;
    l.a_valid = false;
    CHK(ensure(c, l.A, sizeof(float) * (size_t)c->n * c->kp));
    CHK(lda_ensure_sums(c));
    const int kq = c->kp / 4, lanes = plsa::plan::lda_row_lanes(kq);
    const i64 n4 = c->n * kq;
    {
        Scope s(c, "k_lda_rowsum");
        hipLaunchKernelGGL(plsa::k_lda_rowsum, dim3(plsa::plan::lda_rowsum_grid(c->n, kq, c->grid_cap)), dim3(plsa::plan::LDA_BLOCK), 0,
                           c->ls, c->U[c->cu].as<float4>(), (long long)c->n, kq, c->k, lanes, lda_sums(c, LDA_S_DOC),
                           lda_sums(c, LDA_PSI_DOC), lda_sums(c, LDA_SHIFT_DOC));
    }
    {
        Scope s(c, "k_lda_tables");
        hipLaunchKernelGGL(plsa::k_lda_tables<true>, dim3(plsa::plan::lda_grid(n4, c->grid_cap)), dim3(plsa::plan::LDA_BLOCK), 0, c->ls,
                           c->U[c->cu].as<float4>(), l.A.as<float4>(), (long long)n4, kq, c->k, lda_sums(c, LDA_S_DOC),
                           lda_sums(c, LDA_PSI_DOC), scaled ? lda_sums(c, LDA_SHIFT_DOC) : nullptr);
    }
    CHK(launch_check(c, "k_lda_tables"));
    l.a_valid = scaled;
    return 0;
}

// one topic side: lambda [m, kp], the table B formed from it, the float64 slab partials of lambda's column sums, S_z and
// psi(S_z) [kp], the shift per word [m].  A context's own (lda_topic_side) or an online state's (plsa_lda_online.hpp)
struct LdaTopicSide {
    float4 *lam, *B;
    double *slabs, *S, *psi, *shift;
    i64 m;
    int k, kp;
};

// B <- exp(psi(lambda) - psi(S_z) - shift_w) on c's stream: S_z from the float64 slab sums added in slab order (sweep:
// k_lda_topic_partial forms them; otherwise the caller's kernel has left them), shift_w the logarithm of the largest entry of
// word w's row (scaled; otherwise no shift).  The one place the topic-side chain is launched from
int run_lda_topic_tables(plsa_ctx *c, const LdaTopicSide &t, bool sweep, bool scaled) {
    const int kq = t.kp / 4, lanes = plsa::plan::lda_row_lanes(kq);
    const i64 n4 = t.m * kq;
    const int nb = plsa::plan::lda_bound_grid(t.m);
    if (sweep) {
        Scope s(c, "k_lda_topic_partial");
        hipLaunchKernelGGL(plsa::k_lda_topic_partial, dim3(nb), dim3(plsa::plan::LDA_BLOCK), 0, c->ls,
                           reinterpret_cast<const float *>(t.lam), (long long)t.m, t.kp, t.slabs);
    }
    {
        Scope s(c, "k_lda_topic_sums");
        hipLaunchKernelGGL(plsa::k_lda_topic_sums, dim3(plsa::plan::lda_topic_grid(t.kp)), dim3(plsa::plan::LDA_BLOCK), 0, c->ls,
                           t.slabs, nb, t.kp, t.k, t.S, t.psi);
    }
    if (scaled) {
        Scope s(c, "k_lda_wordmax");
        hipLaunchKernelGGL(plsa::k_lda_wordmax, dim3(plsa::plan::lda_rowsum_grid(t.m, kq, c->grid_cap)), dim3(plsa::plan::LDA_BLOCK), 0,
                           c->ls, t.lam, (long long)t.m, kq, t.k, lanes, t.S, t.psi, t.shift);
    }
    {
        Scope s(c, "k_lda_tables");
        hipLaunchKernelGGL(plsa::k_lda_tables<false>, dim3(plsa::plan::lda_grid(n4, c->grid_cap)), dim3(plsa::plan::LDA_BLOCK), 0, c->ls,
                           t.lam, t.B, (long long)n4, kq, t.k, t.S, t.psi, scaled ? t.shift : nullptr);
    }
    return launch_check(c, "k_lda_tables");
}

// the table B of Vt[cv] in the context's side table, with its sums left in the context
int run_lda_table_v(plsa_ctx *c, bool scaled = true) {
    plsa_ctx::Lda &l = c->lda;
    if (l.b_valid && scaled) return 0;
    l.b_valid = false;
    CHK(ensure(c, l.B, sizeof(float) * (size_t)c->m * c->kp));
    CHK(lda_ensure_sums(c));
    CHK(ensure(c, c->colsum_partials, sizeof(double) * (size_t)plsa::plan::lda_bound_grid(c->m) * c->kp));
    CHK(run_lda_topic_tables(c, {c->Vt[c->cv].as<float4>(), l.B.as<float4>(), c->colsum_partials.as<double>(), lda_sums(c, LDA_S_TOPIC),
                                 lda_sums(c, LDA_PSI_TOPIC), lda_sums(c, LDA_SHIFT_WORD), c->m, c->k, c->kp}, true, scaled));
    l.b_valid = scaled;
    return 0;
}

// U[out_u] <- U[out_u] * N_d + alpha behind a document pass that left N_d in c->lda.norm_pdz
int run_lda_rows(plsa_ctx *c, double alpha) {
    const int kq = c->kp / 4;
    const i64 n4 = c->n * kq;
    Scope s(c, "k_lda_rows");
    hipLaunchKernelGGL(plsa::k_lda_rows, dim3(plsa::plan::lda_grid(n4, c->grid_cap)), dim3(plsa::plan::LDA_BLOCK), 0, c->ls,
                       c->U[out_u(c)].as<float4>(), c->lda.norm_pdz.as<float>(), (long long)n4, kq, c->k, (float)alpha);
    return launch_check(c, "k_lda_rows");
}

// Vt[out_v] <- Vacc + eta behind run_col_pass(parts 3)
int run_lda_topics(plsa_ctx *c, double eta) {
    const int kq = c->kp / 4;
    const i64 n4 = c->m * kq;
    Scope s(c, "k_lda_topics");
    hipLaunchKernelGGL(plsa::k_lda_topics, dim3(plsa::plan::lda_grid(n4, c->grid_cap)), dim3(plsa::plan::LDA_BLOCK), 0, c->ls,
                       c->Vacc.as<float4>(), c->Vt[out_v(c)].as<float4>(), (long long)n4, kq, c->k, (float)eta);
    return launch_check(c, "k_lda_topics");
}

// c->lda.out[slot] <- the Dirichlet part of the bound of one table (without its constants): one partial per slab, added in order
template <bool BY_ROW>
int run_lda_dirichlet(plsa_ctx *c, const DevBuf &table, i64 rows, double prior, int slot) {
    plsa_ctx::Lda &l = c->lda;
    const int slabs = plsa::plan::lda_bound_grid(rows);
    double *partials = l.partials.as<double>() + (size_t)slot * plsa::plan::PRIOR_SLABS;
    {
        Scope s(c, "k_lda_bound");
        hipLaunchKernelGGL(plsa::k_lda_bound<BY_ROW>, dim3(slabs), dim3(plsa::plan::LDA_BLOCK), 0, c->stream, table.as<float4>(),
                           (long long)rows, c->kp / 4, c->k, prior, lda_sums(c, BY_ROW ? LDA_S_DOC : LDA_S_TOPIC),
                           lda_sums(c, BY_ROW ? LDA_PSI_DOC : LDA_PSI_TOPIC), partials);
    }
    {
        Scope s(c, "k_ll_final");
        hipLaunchKernelGGL(plsa::k_ll_final, dim3(1), dim3(256), 0, c->stream, partials, slabs, l.out.as<double>() + slot);
    }
    return launch_check(c, "k_lda_bound");
}

// c->lda.out[2] <- sum x_dw (shift_d + shift_w): what the scaling of the tables took out of the likelihood term
int run_lda_shift_sum(plsa_ctx *c) {
    plsa_ctx::Lda &l = c->lda;
    const int slabs = plsa::plan::lda_shift_grid(c->n);
    double *partials = l.partials.as<double>() + (size_t)2 * plsa::plan::PRIOR_SLABS;
    {
        Scope s(c, "k_lda_shift_sum");
        hipLaunchKernelGGL(plsa::k_lda_shift_sum, dim3(slabs), dim3(plsa::plan::LDA_BLOCK), 0, c->stream, c->indptr, c->col, c->val,
                           (long long)c->n, lda_sums(c, LDA_SHIFT_DOC), lda_sums(c, LDA_SHIFT_WORD), partials);
    }
    {
        Scope s(c, "k_ll_final");
        hipLaunchKernelGGL(plsa::k_ll_final, dim3(1), dim3(256), 0, c->stream, partials, slabs, l.out.as<double>() + 2);
    }
    return launch_check(c, "k_lda_shift_sum");
}

// L = sum x_dw log sum_z A_dz B_zw + the Dirichlet part of gamma (+ the Dirichlet part of lambda: with_topics) of the state in
// force, in two halves.  The likelihood term is k_loglik on the scaled tables plus the shifts the scaling took out.
//
// The enqueue half: the sums, launched in one order for every caller, with no host wait.  `gamma_part` launches the Dirichlet
// part of gamma into c->lda.out[0] (run_lda_dirichlet<true> under a scalar alpha, run_lda_dirichlet_v under a vector); `who`
// names the entry point in the one refusal
template <class GammaPart>
int lda_bound_send(plsa_ctx *c, const char *who, GammaPart gamma_part, double eta, bool with_topics) {
    plsa_ctx::Lda &l = c->lda;
    // the sums land in a page-locked slot of the context: a copy still on its way writes to memory that outlives the call
    if (!l.h_out && host_alloc(l.h_out, 3) != hipSuccess) return fail(c, "%s: page-locked buffer allocation failed", who);
    CHK(ensure(c, l.partials, sizeof(double) * (2 * plsa::plan::PRIOR_SLABS + plsa::plan::LDA_SHIFT_SLABS)));
    CHK(ensure(c, l.out, sizeof(double) * 3));
    CHK(run_lda_table_u(c));
    CHK(run_lda_table_v(c));
    CHK(gamma_part());
    if (with_topics) CHK(run_lda_dirichlet<false>(c, c->Vt[c->cv], c->m, eta, 1));
    CHK(run_lda_shift_sum(c));
    HIPCHK(c, hipMemcpyAsync(l.h_out.get(), l.out.as<double>(), sizeof(double) * 3, hipMemcpyDeviceToHost, c->stream));
    StandIn u(c->U[c->cu], l.A), v(c->Vt[c->cv], l.B);
    return run_loglik(c, nullptr, nullptr);                  // sent behind the other sums: its event covers them as well
}

// The finish half: the host waits for the likelihood's event (not for what was enqueued behind it) and adds, in this order, the
// shifts, the gamma part with n times `doc_constant` -- lgamma(k alpha) - k lgamma(alpha), or lgamma(sum alpha) - sum
// lgamma(alpha_z), computed by the caller -- and with_topics the lambda part with k (lgamma(m eta) - m lgamma(eta))
int lda_bound_finish(plsa_ctx *c, double doc_constant, double eta, bool with_topics, double *out) {
    double ll = 0.0;
    CHK(wait_ll(c, &ll));
    const double *part = c->lda.h_out.get();
    ll += part[2];
    ll += part[0] + (double)c->n * doc_constant;
    if (with_topics) ll += part[1] + (double)c->k * (lgamma((double)c->m * eta) - (double)c->m * lgamma(eta));
    *out = ll;
    return 0;
}

auto lda_gamma_part(plsa_ctx *c, double alpha) {
    return [c, alpha] { return run_lda_dirichlet<true>(c, c->U[c->cu], c->n, alpha, 0); };
}
double lda_doc_constant(plsa_ctx *c, double alpha) { return lgamma(c->k * alpha) - c->k * lgamma(alpha); }

int run_lda_bound(plsa_ctx *c, double alpha, double eta, bool with_topics, double *out) {
    CHK(lda_bound_send(c, "plsa_lda_bound", lda_gamma_part(c, alpha), eta, with_topics));
    return lda_bound_finish(c, lda_doc_constant(c, alpha), eta, with_topics, out);
}

// what becomes of the column pass of a round: not run; run, the raw counts left in Vacc (the online step: the block's Vt is
// neither written nor flipped); run, lambda <- eta + the counts into Vt[out_v], which becomes the table in force
enum class LdaColumns { NONE, COUNTS, TOPICS };

// The LDA round, for the batch fits, the fits with a vector prior, the online step and the online fold: tables -> document
// pass (-> column pass) under StandIn -> rows -> flip.  `rows` launches gamma <- alpha + the document pass's counts
// (run_lda_rows under a scalar alpha, run_lda_rows_v under a vector); `columns` is what the last round of an iteration does
template <class Rows>
struct LdaRounds {
    plsa_ctx *c;
    float thresh;
    Rows rows;
    LdaColumns columns;
    double eta;
    int round(bool with_columns) {
        plsa_ctx::Lda &l = c->lda;
        const bool topics = with_columns && columns == LdaColumns::TOPICS;
        CHK(run_lda_table_u(c));
        CHK(run_lda_table_v(c));
        CHK(ensure(c, l.norm_pdz, sizeof(float) * (size_t)c->n));
        {
            StandIn u(c->U[c->cu], l.A), v(c->Vt[c->cv], l.B);
            CHK(run_row_pass(c, false, false, nullptr, thresh, l.norm_pdz.as<float>(), nullptr));
            if (with_columns) CHK(run_col_pass(c, false, nullptr, thresh, 3));
        }
        CHK(rows());
        if (topics) CHK(run_lda_topics(c, eta));
        c->cu ^= 1;
        l.a_valid = false;
        if (topics) { c->cv ^= 1; l.b_valid = false; }
        return 0;
    }
    // doc_iter - 1 gamma-only rounds, then one with the caller's mode
    int iteration(int doc_iter) {
        for (int r = 1; r < doc_iter; ++r) CHK(round(false));
        return round(columns != LdaColumns::NONE);
    }
};

template <class Rows>
LdaRounds<Rows> lda_rounds(plsa_ctx *c, float thresh, Rows rows, LdaColumns columns, double eta) {
    return {c, thresh, rows, columns, eta};
}

auto lda_scalar_rows(plsa_ctx *c, double alpha) {
    return [c, alpha] { return run_lda_rows(c, alpha); };
}

// the reference's loop (fit::run_materialised) over LDA iterations.  update_v = false: the refit -- gamma only, lambda is never
// written and its part of the bound, a constant there, is left out
struct LdaBackend {
    plsa_ctx *c;
    float thresh;
    double alpha, eta;
    int doc_iter;
    bool update_v;
    int loglik(double *f) { return run_lda_bound(c, alpha, eta, update_v, f); }
    int iteration() {
        return lda_rounds(c, thresh, lda_scalar_rows(c, alpha), update_v ? LdaColumns::TOPICS : LdaColumns::NONE, eta).iteration(doc_iter);
    }
};

int lda_prior_ok(plsa_ctx *c, const char *who, const char *name, double v) {
    if (!(v > 0.0) || !std::isfinite(v)) return fail(c, "%s: prior %s=%g is not a finite number > 0", who, name, v);
    return 0;
}

int lda_context_ok(plsa_ctx *c, const char *who) {
    if (c->ref_sums || c->ref_ll) return plain_fused_refusal(c, who, "LDA", PlainFused::REFERENCE_CONTEXT);
    if (c->comm) return fail(c, "%s: the context is a shard of a communicator (plsa_comm_init); LDA has no multi-GPU form", who);
    return 0;
}

int lda_eligible(plsa_ctx *c, const char *who, double alpha, double eta, int doc_iter, int flags) {
    CHK(lda_prior_ok(c, who, "alpha", alpha));
    CHK(lda_prior_ok(c, who, "eta", eta));
    if (doc_iter < 1) return fail(c, "%s: doc_iter=%d is not >= 1", who, doc_iter);
    CHK(plain_fused_refusal(c, who, "LDA", plain_fused(c, flags), flags));
    return lda_context_ok(c, who);
}

// the tables of a call are formed from the state the call finds: whatever an earlier call left is stale
void lda_open(plsa_ctx *c) { c->lda.a_valid = c->lda.b_valid = false; }

}  // namespace

extern "C" {

int plsa_lda_fit(plsa_ctx *c, double alpha, double eta, int32_t n_iter, int32_t n_iter_per_test, double tolerance, int32_t doc_iter,
                 float thresh, int32_t flags, int32_t *iters_done, float *bound_trace, int32_t *n_bound) {
    CHK(lda_eligible(c, "plsa_lda_fit", alpha, eta, doc_iter, flags));
    const FitCall call{nullptr, n_iter, n_iter_per_test, tolerance, flags, iters_done, bound_trace, n_bound};
    CHK(fit_open(c, "plsa_lda_fit", call));
    lda_open(c);
    return fit_run(c, call, fit_rule(flags), true, [&](FitRun &r) {
        LdaBackend backend{c, thresh, alpha, eta, doc_iter, true};
        return plsa::fit::run_materialised(backend, r.tests, n_iter, r.trace, &r.iters);
    });
}

int plsa_lda_refit(plsa_ctx *c, double alpha, int32_t n_iter, int32_t n_iter_per_test, double tolerance, int32_t doc_iter,
                   float thresh, int32_t flags, int32_t *iters_done, float *bound_trace, int32_t *n_bound) {
    CHK(lda_eligible(c, "plsa_lda_refit", alpha, 1.0, doc_iter, flags));
    const FitCall call{nullptr, n_iter, n_iter_per_test, tolerance, flags, iters_done, bound_trace, n_bound};
    CHK(fit_open(c, "plsa_lda_refit", call));
    lda_open(c);
    return fit_run(c, call, plsa::fit::REFIT, true, [&](FitRun &r) {
        LdaBackend backend{c, thresh, alpha, 1.0, doc_iter, false};
        return plsa::fit::run_materialised(backend, r.tests, n_iter, r.trace, &r.iters);
    });
}

int plsa_lda_bound(plsa_ctx *c, double alpha, double eta, int32_t with_topics, double *out) {
    CHK(lda_prior_ok(c, "plsa_lda_bound", "alpha", alpha));
    if (with_topics) CHK(lda_prior_ok(c, "plsa_lda_bound", "eta", eta));
    CHK(lda_context_ok(c, "plsa_lda_bound"));
    if (!out) return fail(c, "plsa_lda_bound: out is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(need_factors(c));
    lda_open(c);
    return run_lda_bound(c, alpha, eta, with_topics != 0, out);
}

int plsa_lda_tables(plsa_ctx *c, float *A_out, float *B_out) {
    CHK(lda_context_ok(c, "plsa_lda_tables"));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(need_factors(c));
    lda_open(c);
    CHK(run_lda_table_u(c, false));
    CHK(run_lda_table_v(c, false));
    {
        StandIn u(c->U[c->cu], c->lda.A), v(c->Vt[c->cv], c->lda.B);   // the read-back, pointed at the side tables
        CHK(plsa_get_factors(c, A_out, B_out));
    }
    return 0;
}

}  // extern "C"
