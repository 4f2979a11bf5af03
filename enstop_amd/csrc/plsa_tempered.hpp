// plsa_tempered.hpp -- host side of tempered EM (include/plsa_hip_tempered.h) and of plsa_temper_factors (plsa_hip_diag.h);
// part of plsa_hip.hip's translation unit (included at its end: it uses the context, the pass wrappers and plsa_fit).
//
// A tempered iteration raises the current factors to the power beta into two side tables (k_temper), then runs the launch
// chain of an unsharded fused iteration -- run_row_pass, run_col_pass, run_col_tail, untouched -- with the side tables standing
// in for the current factors: the passes read c->U[c->cu] and c->Vt[c->cv], so the side tables are swapped into those two
// places for the length of the chain (StandIn) and the passes write the alternates as they always do.  One stream, no
// look-ahead buffers, no hipGraph; every likelihood is k_loglik on the true factors.  The call around the loop is the frame
// of plsa_drivers.hpp.
#pragma once

namespace {

// both side tables from the current factors, on c->ls
int run_temper(plsa_ctx *c, double beta) {
    plsa_ctx::Tempered &t = c->tempered;
    CHK(ensure(c, t.U, sizeof(float) * (size_t)c->n * c->kp));
    CHK(ensure(c, t.Vt, sizeof(float) * (size_t)c->m * c->kp));
    const DevBuf *in[2] = {&c->U[c->cu], &c->Vt[c->cv]};
    DevBuf *out[2] = {&t.U, &t.Vt};
    const i64 rows[2] = {c->n, c->m};
    for (int i = 0; i < 2; ++i) {
        const i64 n4 = rows[i] * c->kp / 4;
        Scope s(c, "k_temper");
        hipLaunchKernelGGL(plsa::k_temper, dim3(plsa::plan::temper_grid(n4, c->grid_cap)), dim3(plsa::plan::TEMPER_BLOCK), 0, c->ls,
                           in[i]->as<float4>(), out[i]->as<float4>(), (long long)n4, beta);
    }
    return launch_check(c, "k_temper");
}

// the reference's loop (fit::run_materialised) over tempered iterations
struct TemperedBackend {
    plsa_ctx *c;
    const float *d_sw, *d_sw_m;
    float thresh;
    double beta;
    int loglik(double *ll) { return run_loglik(c, d_sw, ll); }
    int iteration() {
        CHK(run_temper(c, beta));
        {
            StandIn u(c->U[c->cu], c->tempered.U), v(c->Vt[c->cv], c->tempered.Vt);
            CHK(run_row_pass(c, false, false, d_sw, thresh, nullptr, nullptr));
            CHK(run_col_pass(c, false, d_sw_m, thresh, 1));
            CHK(run_col_tail(c));
        }
        c->cu ^= 1; c->cv ^= 1;
        return 0;
    }
};

int tempered_eligible(plsa_ctx *c, const char *who, double beta, int flags) {
    if (!(beta > 0.0 && beta <= 1.0)) return fail(c, "%s: beta=%g outside (0, 1]", who, beta);
    return plain_fused_refusal(c, who, "tempered", plain_fused(c, flags), flags);
}

}  // namespace

extern "C" {

int plsa_fit_tempered(plsa_ctx *c, const float *sw, double beta, int32_t n_iter, int32_t n_iter_per_test, double tolerance,
                      float thresh, int32_t flags, int32_t *iters_done, float *ll_trace, int32_t *n_ll) {
    CHK(tempered_eligible(c, "plsa_fit_tempered", beta, flags));
    if (beta == 1.0) return plsa_fit(c, sw, n_iter, n_iter_per_test, tolerance, thresh, flags, iters_done, ll_trace, n_ll);
    const FitCall call{sw, n_iter, n_iter_per_test, tolerance, flags, iters_done, ll_trace, n_ll};
    CHK(fit_open(c, "plsa_fit_tempered", call));
    return fit_run(c, call, fit_rule(flags), true, [&](FitRun &r) {
        TemperedBackend backend{c, r.d_sw, r.d_sw_m, thresh, beta};
        return plsa::fit::run_materialised(backend, r.tests, n_iter, r.trace, &r.iters);
    });
}

int plsa_factors_snapshot(plsa_ctx *c) {
    HIPCHK(c, hipSetDevice(c->device));
    CHK(need_factors(c));
    plsa_ctx::Tempered &t = c->tempered;
    const size_t ub = sizeof(float) * (size_t)c->n * c->kp, vb = sizeof(float) * (size_t)c->m * c->kp;
    t.have_snap = false;
    CHK(ensure(c, t.snapU, ub));
    CHK(ensure(c, t.snapVt, vb));
    HIPCHK(c, hipMemcpyAsync(t.snapU.p, c->U[c->cu].p, ub, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(t.snapVt.p, c->Vt[c->cv].p, vb, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    t.snap_n = c->n; t.snap_m = c->m; t.snap_k = c->k;
    t.have_snap = true;
    return 0;
}

int plsa_factors_restore(plsa_ctx *c) {
    HIPCHK(c, hipSetDevice(c->device));
    plsa_ctx::Tempered &t = c->tempered;
    if (!t.have_snap) return fail(c, "plsa_factors_restore: no snapshot on this context (plsa_factors_snapshot; plsa_release_scratch frees it)");
    CHK(need_factors(c));
    if (t.snap_n != c->n || t.snap_m != c->m || t.snap_k != c->k)
        return fail(c, "plsa_factors_restore: the snapshot holds factors for %lld x %lld with k=%d, the context now %lld x %lld with k=%d",
                    (long long)t.snap_n, (long long)t.snap_m, t.snap_k, (long long)c->n, (long long)c->m, c->k);
    const size_t ub = sizeof(float) * (size_t)c->n * c->kp, vb = sizeof(float) * (size_t)c->m * c->kp;
    HIPCHK(c, hipMemcpyAsync(c->U[c->cu].p, t.snapU.p, ub, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->Vt[c->cv].p, t.snapVt.p, vb, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->p_state.invalidate();             // new factors, as after plsa_set_factors
    return 0;
}

int plsa_temper_factors(plsa_ctx *c, double beta, float *U_out, float *V_out) {
    HIPCHK(c, hipSetDevice(c->device));
    if (!(beta > 0.0 && beta <= 1.0)) return fail(c, "plsa_temper_factors: beta=%g outside (0, 1]", beta);
    CHK(need_factors(c));
    CHK(run_temper(c, beta));
    {
        StandIn u(c->U[c->cu], c->tempered.U), v(c->Vt[c->cv], c->tempered.Vt);   // the read-back, pointed at the side tables
        CHK(plsa_get_factors(c, U_out, V_out));
    }
    return 0;
}

}  // extern "C"
