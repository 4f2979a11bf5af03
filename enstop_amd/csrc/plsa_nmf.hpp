// plsa_nmf.hpp -- host side of the KL-divergence NMF (include/plsa_hip_nmf.h); part of plsa_hip.hip's translation unit
// (included at its end: it uses the context, the builders and the launch helpers defined there).
//
// W lives in U[cu], H in Vt[cv]; both halves update in place (a document's row is read and written by its own group, the
// H tail is elementwise), so cu / cv never move and the alternates stay free.  The structures, entry streams, scratch and
// grids are the EM passes', taken from their preparations (prepare_row_pass, prepare_col_pass); `Vacc` holds the per-column
// sums (k_col_reduce adds the item partials, heavy columns included).
#pragma once

namespace {

int nmf_ready(plsa_ctx *c, const char *who) {
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n <= 0) return fail(c, "%s: no corpus uploaded", who);
    if (c->k <= 0 || !c->U[0].p || !c->Vt[0].p) return fail(c, "%s: factors not set (call plsa_nmf_set_factors)", who);
    if (c->k > 1024) return fail(c, "%s: k=%d outside [1,1024]", who, c->k);
    return need_factors(c);
}

// which: 0 = W_sum (over the n rows of U, zeros -> 1), 1 = H_sum (over the m rows of Vt, zeros -> EPS32)
int nmf_factor_sum(plsa_ctx *c, int which) {
    const i64 rows = which ? c->m : c->n;
    const float *A = which ? c->Vt[c->cv].as<float>() : c->U[c->cu].as<float>();
    const int nb = (int)std::min<i64>(plsa::NORM_BLOCKS, std::max<i64>(1, rows));
    CHK(ensure(c, c->nmf.slabs, sizeof(double) * (size_t)plsa::NORM_BLOCKS * c->kp));
    CHK(ensure(c, c->nmf.raw, sizeof(double) * 2 * (size_t)c->kp));
    CHK(ensure(c, c->nmf.guarded, sizeof(float) * 2 * (size_t)c->kp));
    {
        Scope s(c, "k_nmf_colsum_partial");
        hipLaunchKernelGGL(plsa::k_nmf_colsum_partial, dim3(nb), dim3(256), 0, c->ls, A, rows, c->kp, c->nmf.slabs.as<double>());
    }
    {
        Scope s(c, "k_nmf_colsum_final");
        hipLaunchKernelGGL(plsa::k_nmf_colsum_final, dim3(1), dim3(256), 0, c->ls, c->nmf.slabs.as<double>(), nb, c->kp,
                           c->nmf.raw.as<double>() + (size_t)which * c->kp, c->nmf.guarded.as<float>() + (size_t)which * c->kp,
                           which ? plsa::NMF_EPS32 : 1.0f);
    }
    return launch_check(c, "k_nmf_colsum");
}

bool nmf_row_items(plsa_ctx *c) { return c->ritems.use && c->ritems.n > 0; }

// `iters` W half-iterations with H (and the H_sum already on the device) fixed; more than one only in row-ordered mode
int nmf_run_update_w(plsa_ctx *c, int iters) {
    RowLaunch r;
    CHK(prepare_row_pass(c, false, false, r));
    if (r.items && iters != 1) return fail(c, "internal: the combined NMF pass needs whole documents");
    c->p_state.invalidate();
    CHK(dispatch_shape_row(c, [&](auto S) {
        using Sh = decltype(S);
        const float *Vt = c->Vt[c->cv].as<float>(), *hs = c->nmf.guarded.as<float>() + c->kp;
        float *W = c->U[c->cu].as<float>();
        const int n = (int)c->n, kp = c->kp;
        auto launch = [&](auto SS) {
            Scope s(c, "k_nmf_row_pass");
            hipLaunchKernelGGL((plsa::k_nmf_row_pass<decltype(SS)>), dim3(r.plan.grid), dim3(256), 0, c->ls, r.indptr, r.colidx,
                               r.vals, r.sblk, n, r.order, W, Vt, hs, kp, iters, r.ritem_row, r.ritem_start, r.rseg, r.n_ritems, r.rpartial);
        };
        if (r.packed) launch(plsa::Packed<Sh>{}); else launch(Sh{});
        if (r.items) {
            Scope s(c, "k_nmf_row_reduce");
            hipLaunchKernelGGL((plsa::k_nmf_row_reduce<Sh>), dim3(r.plan.reduce_grid), dim3(256), 0, c->ls,
                               r.ritem_first, n, r.rpartial, W, hs, kp);
        }
    }));
    return launch_check(c, "k_nmf_row_pass");
}

// one H half-iteration from the current W: W_sum, the column pass, the per-column sums, the update
int nmf_run_update_h(plsa_ctx *c) {
    ColLaunch l;
    CHK(prepare_col_pass(c, false, l));
    CHK(nmf_factor_sum(c, 0));
    c->p_state.invalidate();
    CHK(dispatch_shape_gather(c, table_is_wide(c, c->n), [&](auto S) {     // the pass gathers W rows: n of them
        using Sh = decltype(S);
        const int grid = plsa::plan::col_grid(nullptr, l.plan.n_chunks, false);      // one chunk per workgroup, no XCD stretches
        const float *W = c->U[c->cu].as<float>(), *Vt = c->Vt[c->cv].as<float>();
        auto launch = [&](auto SS) {
            Scope s(c, "k_nmf_col_pass");
            hipLaunchKernelGGL((plsa::k_nmf_col_pass<decltype(SS)>), dim3(grid), dim3(256), 0, c->ls, l.item_rec, l.n_items,
                               l.csc_row, l.csc_val, l.slot, W, Vt, l.partial, c->kp);
        };
        if (l.packed) launch(plsa::Packed<Sh>{}); else launch(Sh{});
    }));
    CHK(launch_check(c, "k_nmf_col_pass"));
    CHK(run_col_pass(c, false, nullptr, 0.f, 2));          // k_col_reduce: partial -> Vacc, fixed item order
    {
        Scope s(c, "k_nmf_h_finish");
        const i64 total4 = c->m * c->kp / 4;
        hipLaunchKernelGGL(plsa::k_nmf_h_finish, dim3(grid_for(c, total4, 256)), dim3(256), c->kp * sizeof(float), c->ls,
                           c->Vacc.as<float>(), c->Vt[c->cv].as<float>(), c->m, c->kp, c->nmf.guarded.as<float>());
    }
    return launch_check(c, "k_nmf_h_finish");
}

// the objective walks whole documents in the document pass' lane shape: that pass' two arrays and its whole-document grid
int nmf_run_divergence(plsa_ctx *c, double *out) {
    CHK(nmf_factor_sum(c, 0));
    CHK(nmf_factor_sum(c, 1));
    RowLaunch r;
    CHK(prepare_row_pass(c, true, false, r));
    const int grid = r.plan.reduce_grid;
    const int *order = r.order;
    if (r.items) CHK(ensure_roworder(c, &order));          // (a pass over row items has no use for the order)
    CHK(ensure(c, c->nmf.obj, sizeof(double) * 2 * (size_t)grid));
    CHK(ensure(c, c->nmf.out, sizeof(double) * 2));
    CHK(dispatch_shape_row(c, [&](auto S) {
        Scope s(c, "k_nmf_divergence");
        hipLaunchKernelGGL((plsa::k_nmf_divergence<decltype(S)>), dim3(grid), dim3(256), 0, c->ls, r.indptr, r.colidx, r.vals,
                           (int)c->n, order, c->U[c->cu].as<float>(), c->Vt[c->cv].as<float>(), c->kp, c->nmf.obj.as<double>());
    }));
    {
        Scope s(c, "k_nmf_divergence_final");
        hipLaunchKernelGGL(plsa::k_nmf_divergence_final, dim3(1), dim3(256), 0, c->ls, c->nmf.obj.as<double>(), grid,
                           c->nmf.raw.as<double>(), c->nmf.raw.as<double>() + c->kp, c->k, c->nmf.out.as<double>());
    }
    CHK(launch_check(c, "k_nmf_divergence"));
    double h[2] = {0.0, 0.0};
    HIPCHK(c, hipMemcpyAsync(h, c->nmf.out.p, sizeof h, hipMemcpyDeviceToHost, c->ls));
    HIPCHK(c, hipStreamSynchronize(c->ls));
    *out = h[0];
    return 0;
}

}  // namespace

extern "C" {

int plsa_nmf_set_factors(plsa_ctx *c, const float *W, const float *H, int64_t n, int64_t m, int32_t k) {
    if (!W || !H) return fail(c, "plsa_nmf_set_factors: W and H must both be given");
    return plsa_set_factors(c, W, H, n, m, k);     // stores the values as they are (padding columns zero)
}

int plsa_nmf_get_factors(plsa_ctx *c, float *W, float *H) {
    CHK(nmf_ready(c, "plsa_nmf_get_factors"));
    return plsa_get_factors(c, W, H);
}

int plsa_nmf_update_w(plsa_ctx *c) {
    CHK(nmf_ready(c, "plsa_nmf_update_w"));
    CHK(nmf_factor_sum(c, 1));
    CHK(nmf_run_update_w(c, 1));
    HIPCHK(c, hipStreamSynchronize(c->ls));
    return 0;
}

int plsa_nmf_update_h(plsa_ctx *c) {
    CHK(nmf_ready(c, "plsa_nmf_update_h"));
    CHK(nmf_run_update_h(c));
    HIPCHK(c, hipStreamSynchronize(c->ls));
    return 0;
}

int plsa_nmf_divergence(plsa_ctx *c, double *sqrt2d) {
    CHK(nmf_ready(c, "plsa_nmf_divergence"));
    if (!sqrt2d) return fail(c, "plsa_nmf_divergence: NULL argument");
    return nmf_run_divergence(c, sqrt2d);
}

int plsa_nmf_fit(plsa_ctx *c, int update_h, int max_iter, double tol, int32_t *n_iter, double *errors, int32_t errors_len) {
    CHK(nmf_ready(c, "plsa_nmf_fit"));
    if (max_iter < 1) return fail(c, "plsa_nmf_fit: max_iter=%d, expected at least 1", max_iter);
    int n_err = 0;
    auto record = [&](double e) { if (errors && n_err < errors_len) errors[n_err] = e; n_err++; };
    double error_at_init = 0.0;
    CHK(nmf_run_divergence(c, &error_at_init));
    record(error_at_init);
    double previous = error_at_init;
    CHK(ensure_ritems(c));
    // H fixed and whole documents: every iteration up to the next test (or the end) in one launch of the document pass
    const bool combined = !update_h && !nmf_row_items(c);
    if (!update_h) CHK(nmf_factor_sum(c, 1));
    int it = 0;
    while (it < max_iter) {
        if (combined) {
            const int next = tol > 0 ? std::min(max_iter, (it / 10 + 1) * 10) : max_iter;
            CHK(nmf_run_update_w(c, next - it));
            it = next;
        } else {
            if (update_h) CHK(nmf_factor_sum(c, 1));
            CHK(nmf_run_update_w(c, 1));
            if (update_h) CHK(nmf_run_update_h(c));
            it++;
        }
        if (tol > 0 && it % 10 == 0) {                     // "test convergence criterion every 10 iterations"
            double error = 0.0;
            CHK(nmf_run_divergence(c, &error));
            record(error);
            if ((previous - error) / error_at_init < tol) break;
            previous = error;
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->ls));
    if (n_iter) *n_iter = it;
    return 0;
}

}  // extern "C"
