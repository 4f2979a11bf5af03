// plsa_lda_online.hpp -- host side of online variational Bayes LDA (enstop_amd/include/plsa_hip_lda_online.h, DESIGN.md section
// 21); part of plsa_hip.hip's translation unit (included at its end, behind plsa_lda_priors.hpp: it uses the context, the pass
// wrappers, the rounds and the bound's sums of plsa_lda.hpp and the event discipline of plsa_online.hpp).
//
// A plsa_lda_online state owns lambda [m, kp], the table B formed from it, B's float64 side arrays (S_z [kp], psi(S_z) [kp],
// the shift per word [m] -- the tail of a context's lda.sums, in its order), the slab partials of the column sums, a step
// counter and ONE event.  A step or fold runs on the block context's one stream.  For its length the state's B stands in for
// the block's side table c->lda.B (StandIn) with b_valid set, and the side arrays are copied into the tail of the block's
// lda.sums, so every kernel of the block that reads the topic side -- the passes through run_lda_table_v's validity flag,
// k_lda_shift_sum for the bound -- reads the state's; the block's own topic table Vt is never read or written.  The blend,
// the topic sums, the word shifts and the table follow on the same stream, on the state's buffers.  Steps on different
// contexts are ordered on the device by the event.  No second stream, no look-ahead, no hipGraph.
#pragma once

struct plsa_lda_online {
    plsa_ctx *home = nullptr;        // its device, its stream and staging buffer for the host <-> device copies of lambda
    int device = 0;
    i64 m = 0;
    int k = 0, kp = 0;
    DevBuf lam, B, sums, slabs;
    Event ev;
    bool recorded = false;           // ev has been recorded at least once
    int64_t t = 0;                   // steps taken since plsa_lda_online_set_lambda
};

namespace {

size_t lda_online_table_bytes(const plsa_lda_online *st) { return sizeof(float) * (size_t)st->m * st->kp; }
size_t lda_online_side_count(const plsa_lda_online *st) { return 2 * (size_t)st->kp + (size_t)st->m; }

// the state's side arrays: S_z, psi(S_z), the shift per word
double *lda_online_s(plsa_lda_online *st) { return st->sums.as<double>(); }
double *lda_online_psi(plsa_lda_online *st) { return st->sums.as<double>() + st->kp; }
double *lda_online_shift(plsa_lda_online *st) { return st->sums.as<double>() + 2 * (size_t)st->kp; }

// every refusal of a step or fold that looks at the state, the block context and the arguments; launches nothing
int lda_online_eligible(plsa_lda_online *st, plsa_ctx *c, const char *who, double alpha, double eta, int flags) {
    if (!st) return fail(c, "%s: no state", who);
    CHK(lda_prior_ok(c, who, "alpha", alpha));
    CHK(lda_prior_ok(c, who, "eta", eta));
    CHK(plain_fused_refusal(c, who, "online LDA", plain_fused(c, flags), flags));
    if (c->sharded || c->comm)
        return fail(c, "%s: the context is a shard of a communicator (plsa_comm_init); online LDA has no multi-GPU form", who);
    if (c->device != st->device)
        return fail(c, "%s: the state lives on device %d, the block context on device %d", who, st->device, c->device);
    CHK(need_factors(c));
    if (c->m != st->m || c->k != st->k || c->kp != st->kp)
        return fail(c, "%s: the state holds lambda for %lld words with k=%d, the block context has %lld words with k=%d", who,
                    (long long)st->m, st->k, (long long)c->m, c->k);
    return 0;
}

// what another context's step or fold enqueued precedes what this one enqueues
int lda_online_wait(plsa_lda_online *st, plsa_ctx *c) {
    if (st->recorded) HIPCHK(c, hipStreamWaitEvent(c->stream, st->ev, 0));
    return 0;
}
int lda_online_record(plsa_lda_online *st, plsa_ctx *c) {
    HIPCHK(c, hipEventRecord(st->ev, c->stream));
    st->recorded = true;
    return 0;
}
// the host waits for the last step or fold (before it reads or writes lambda through the home stream)
int lda_online_host_wait(plsa_lda_online *st) {
    plsa_ctx *h = st->home;
    HIPCHK(h, hipSetDevice(st->device));
    if (st->recorded) HIPCHK(h, hipEventSynchronize(st->ev));
    return 0;
}

// B and its side arrays from the state's lambda on c's stream: run_lda_table_v's launches on the state's buffers.  sweep: the
// slab partials come from k_lda_topic_partial (a lambda the host set); otherwise k_lda_online_blend has left them
int lda_online_tables(plsa_lda_online *st, plsa_ctx *c, bool sweep) {
    const int kq = st->kp / 4, lanes = plsa::plan::lda_row_lanes(kq);
    const i64 n4 = st->m * kq;
    const int nb = plsa::plan::lda_bound_grid(st->m);
    if (sweep) {
        Scope s(c, "k_lda_topic_partial");
        hipLaunchKernelGGL(plsa::k_lda_topic_partial, dim3(nb), dim3(plsa::plan::LDA_BLOCK), 0, c->ls, st->lam.as<float>(),
                           (long long)st->m, st->kp, st->slabs.as<double>());
    }
    {
        Scope s(c, "k_lda_topic_sums");
        hipLaunchKernelGGL(plsa::k_lda_topic_sums, dim3(plsa::plan::lda_topic_grid(st->kp)), dim3(plsa::plan::LDA_BLOCK), 0, c->ls,
                           st->slabs.as<double>(), nb, st->kp, st->k, lda_online_s(st), lda_online_psi(st));
    }
    {
        Scope s(c, "k_lda_wordmax");
        hipLaunchKernelGGL(plsa::k_lda_wordmax, dim3(plsa::plan::lda_rowsum_grid(st->m, kq, c->grid_cap)), dim3(plsa::plan::LDA_BLOCK), 0,
                           c->ls, st->lam.as<float4>(), (long long)st->m, kq, st->k, lanes, lda_online_s(st), lda_online_psi(st),
                           lda_online_shift(st));
    }
    {
        Scope s(c, "k_lda_tables");
        hipLaunchKernelGGL(plsa::k_lda_tables<false>, dim3(plsa::plan::lda_grid(n4, c->grid_cap)), dim3(plsa::plan::LDA_BLOCK), 0, c->ls,
                           st->lam.as<float4>(), st->B.as<float4>(), (long long)n4, kq, st->k, lda_online_s(st), lda_online_psi(st),
                           lda_online_shift(st));
    }
    return launch_check(c, "k_lda_tables");
}

// lambda' = b Vacc + (a lambda + c) with its slab sums, then the tables of lambda': four launches on the block's stream
int lda_online_global_update(plsa_lda_online *st, plsa_ctx *c, float a, float b, float cc) {
    {
        Scope s(c, "k_lda_online_blend");
        hipLaunchKernelGGL(plsa::k_lda_online_blend, dim3(plsa::plan::blend_grid(st->m)), dim3(plsa::plan::BLEND_BLOCK), 0, c->ls,
                           st->lam.as<float4>(), c->Vacc.as<float4>(), (long long)st->m, st->kp, st->k, a, b, cc,
                           st->slabs.as<double>());
    }
    CHK(launch_check(c, "k_lda_online_blend"));
    return lda_online_tables(st, c, false);
}

// The state's topic side in the place the block's kernels read it, for the length of one launch chain: B behind c->lda.B with
// b_valid set (run_lda_table_v then launches nothing), the side arrays copied into the tail of c->lda.sums.  Everything the
// block owns is allocated by prepare(), before anything stands in.
struct LdaOnlineTopicSide {
    plsa_lda_online *st;
    plsa_ctx *c;
    StandIn b;
    LdaOnlineTopicSide(plsa_lda_online *st_, plsa_ctx *c_) : st(st_), c(c_), b(c_->lda.B, st_->B) { c->lda.b_valid = true; }
    ~LdaOnlineTopicSide() { c->lda.a_valid = c->lda.b_valid = false; }
    static int prepare(plsa_lda_online *st, plsa_ctx *c) {
        c->lda.a_valid = c->lda.b_valid = false;
        CHK(lda_ensure_sums(c));
        CHK(ensure(c, c->lda.norm_pdz, sizeof(float) * (size_t)c->n));
        HIPCHK(c, hipMemcpyAsync(lda_sums(c, LDA_S_TOPIC), st->sums.p, sizeof(double) * lda_online_side_count(st),
                                 hipMemcpyDeviceToDevice, c->stream));
        return 0;
    }
};

// one round of LdaBackend::round on the block under the topic side standing in: gamma <- alpha + the document pass's counts;
// with_counts: run_col_pass(parts 3) leaves the block's raw counts in Vacc.  The block's Vt is neither written nor flipped
int lda_online_round(plsa_ctx *c, double alpha, float thresh, bool with_counts) {
    plsa_ctx::Lda &l = c->lda;
    CHK(run_lda_table_u(c));
    CHK(run_lda_table_v(c));                                 // (valid: the state's B; launches nothing)
    {
        StandIn u(c->U[c->cu], l.A), v(c->Vt[c->cv], l.B);
        CHK(run_row_pass(c, false, false, nullptr, thresh, l.norm_pdz.as<float>(), nullptr));
        if (with_counts) CHK(run_col_pass(c, false, nullptr, thresh, 3));
    }
    CHK(run_lda_rows(c, alpha));
    c->cu ^= 1;
    l.a_valid = false;
    return 0;
}

// The bound of the block without the topic part at the state in force on c (the state's topic side standing in): the sums of
// run_lda_bound(c, alpha, ., false, .), launched in its order, without its host wait ...
int lda_online_bound_send(plsa_ctx *c, double alpha) {
    plsa_ctx::Lda &l = c->lda;
    if (!l.h_out && host_alloc(l.h_out, 3) != hipSuccess) return fail(c, "plsa_lda_online_step: page-locked buffer allocation failed");
    CHK(ensure(c, l.partials, sizeof(double) * (2 * plsa::plan::PRIOR_SLABS + plsa::plan::LDA_SHIFT_SLABS)));
    CHK(ensure(c, l.out, sizeof(double) * 3));
    CHK(run_lda_table_u(c));
    CHK(run_lda_table_v(c));
    CHK(run_lda_dirichlet<true>(c, c->U[c->cu], c->n, alpha, 0));
    CHK(run_lda_shift_sum(c));
    HIPCHK(c, hipMemcpyAsync(l.h_out.get(), l.out.as<double>(), sizeof(double) * 3, hipMemcpyDeviceToHost, c->stream));
    StandIn u(c->U[c->cu], l.A), v(c->Vt[c->cv], l.B);
    return run_loglik(c, nullptr, nullptr);                  // sent behind the other sums: its event covers them as well
}

// ... and the wait, with run_lda_bound's additions in its order
int lda_online_bound_wait(plsa_ctx *c, double alpha, double *out) {
    double ll = 0.0;
    CHK(wait_ll(c, &ll));
    const double *part = c->lda.h_out.get();
    ll += part[2];
    ll += part[0] + (double)c->n * (lgamma(c->k * alpha) - c->k * lgamma(alpha));
    *out = ll;
    return 0;
}

// host [k, m] -> lambda [m, kp] (0 at the pads), through the home context's staging buffer and stream; the caller waits
int lda_online_upload(plsa_lda_online *st, const float *host) {
    plsa_ctx *h = st->home;
    const size_t count = (size_t)st->k * st->m;
    CHK(ensure(h, h->tmp0, sizeof(float) * count));
    HIPCHK(h, hipMemcpyAsync(h->tmp0.p, host, sizeof(float) * count, hipMemcpyHostToDevice, h->stream));
    const iplan::Grid2 g = iplan::transpose_grid(st->m, st->kp);
    hipLaunchKernelGGL(plsa::k_v_to_vt, dim3(g.x, g.y), dim3(256), 0, h->stream, h->tmp0.as<float>(), st->lam.as<float>(), st->k,
                       (int)st->m, st->kp);
    return launch_check(h, "k_v_to_vt");
}

int lda_online_download(plsa_lda_online *st, float *host) {
    plsa_ctx *h = st->home;
    const size_t count = (size_t)st->k * st->m;
    CHK(ensure(h, h->tmp0, sizeof(float) * count));
    const iplan::Grid2 g = iplan::transpose_grid(st->m, st->kp);
    hipLaunchKernelGGL(plsa::k_vt_to_v, dim3(g.x, g.y), dim3(256), 0, h->stream, st->lam.as<float>(), h->tmp0.as<float>(), st->k,
                       (int)st->m, st->kp);
    CHK(launch_check(h, "k_vt_to_v"));
    CHK(copy_to_host(h, host, h->tmp0.p, sizeof(float) * count));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

}  // namespace

extern "C" {

int plsa_lda_online_create(plsa_ctx *home, int64_t m, int32_t k, plsa_lda_online **out) {
    if (!out) return fail(home, "plsa_lda_online_create: state is NULL");
    *out = nullptr;
    if (!home) return fail(nullptr, "plsa_lda_online_create: no home context");
    HIPCHK(home, hipSetDevice(home->device));
    if (k <= 0 || k > 1024) return fail(home, "plsa_lda_online_create: k=%d outside [1,1024]", k);
    if (m <= 0 || m >= ((int64_t)1 << 31) - 1) return fail(home, "plsa_lda_online_create: m=%lld outside [1, 2^31 - 2]", (long long)m);
    std::unique_ptr<plsa_lda_online> owner(new plsa_lda_online());
    plsa_lda_online *st = owner.get();
    st->home = home; st->device = home->device; st->m = m; st->k = k;
    st->kp = plsa::plan::lane_shape(k, home->chunks_per_lane, home->row_shape_8x2).kp;
    static_assert(plsa::plan::BLEND_MAX_KP >= 1024, "k <= 1024");
    const size_t bytes = lda_online_table_bytes(st);
    CHK(ensure(home, st->lam, bytes));
    CHK(ensure(home, st->B, bytes));
    CHK(ensure(home, st->sums, sizeof(double) * lda_online_side_count(st)));
    CHK(ensure(home, st->slabs, sizeof(double) * (size_t)plsa::plan::blend_grid(m) * st->kp));
    HIPCHK(home, hipMemsetAsync(st->lam.p, 0, bytes, home->stream));
    HIPCHK(home, hipMemsetAsync(st->B.p, 0, bytes, home->stream));
    HIPCHK(home, hipMemsetAsync(st->sums.p, 0, sizeof(double) * lda_online_side_count(st), home->stream));
    HIPCHK(home, hipStreamSynchronize(home->stream));
    HIPCHK(home, hipEventCreateWithFlags(&st->ev.h, hipEventDisableTiming));
    *out = owner.release();
    return 0;
}

void plsa_lda_online_destroy(plsa_lda_online *st) {
    if (!st) return;
    (void)hipSetDevice(st->device);
    if (st->recorded) (void)hipEventSynchronize(st->ev);
    delete st;
}

int plsa_lda_online_set_lambda(plsa_lda_online *st, const float *lam) {
    if (!st) return fail(nullptr, "plsa_lda_online_set_lambda: no state");
    plsa_ctx *h = st->home;
    if (!lam) return fail(h, "plsa_lda_online_set_lambda: lam is NULL");
    CHK(lda_online_host_wait(st));
    CHK(lda_online_upload(st, lam));
    CHK(lda_online_tables(st, h, true));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    st->t = 0;
    return 0;
}

int plsa_lda_online_get_lambda(plsa_lda_online *st, float *lam, int64_t *steps) {
    if (!st) return fail(nullptr, "plsa_lda_online_get_lambda: no state");
    CHK(lda_online_host_wait(st));
    if (steps) *steps = st->t;
    return lam ? lda_online_download(st, lam) : 0;
}

int plsa_lda_online_step(plsa_lda_online *st, plsa_ctx *c, double alpha, double eta, int32_t doc_iter, float thresh, double rho,
                         double scale, int32_t flags, double *bound_partial) {
    const char *who = "plsa_lda_online_step";
    if (!c) return fail(nullptr, "%s: no block context", who);
    CHK(lda_online_eligible(st, c, who, alpha, eta, flags));
    if (doc_iter < 1) return fail(c, "%s: doc_iter=%d is not >= 1", who, doc_iter);
    if (!(rho > 0.0 && rho <= 1.0)) return fail(c, "%s: rho=%g outside (0, 1]", who, rho);
    if (!(scale > 0.0) || !std::isfinite(scale)) return fail(c, "%s: scale=%g is not a positive number", who, scale);
    const float a = (float)(1.0 - rho), b = (float)(rho * scale), cc = (float)(rho * eta);
    HIPCHK(c, hipSetDevice(c->device));
    CHK(lda_online_wait(st, c));
    CHK(LdaOnlineTopicSide::prepare(st, c));
    {
        LdaOnlineTopicSide side(st, c);
        for (int r = 1; r < doc_iter; ++r) CHK(lda_online_round(c, alpha, thresh, false));
        CHK(lda_online_round(c, alpha, thresh, true));
        if (bound_partial) CHK(lda_online_bound_send(c, alpha));      // the scalar travels while the update runs
    }
    c->p_state.invalidate();
    CHK(lda_online_global_update(st, c, a, b, cc));
    CHK(lda_online_record(st, c));
    st->t += 1;
    if (bound_partial) CHK(lda_online_bound_wait(c, alpha, bound_partial));      // the only host wait of a step
    return 0;
}

int plsa_lda_online_fold(plsa_lda_online *st, plsa_ctx *c, double alpha, int32_t n_rounds, float thresh, int32_t flags) {
    const char *who = "plsa_lda_online_fold";
    if (!c) return fail(nullptr, "%s: no block context", who);
    CHK(lda_online_eligible(st, c, who, alpha, 1.0, flags));
    if (n_rounds < 0) return fail(c, "%s: n_rounds=%d is negative", who, n_rounds);
    HIPCHK(c, hipSetDevice(c->device));
    CHK(lda_online_wait(st, c));
    CHK(LdaOnlineTopicSide::prepare(st, c));
    {
        LdaOnlineTopicSide side(st, c);
        for (int r = 0; r < n_rounds; ++r) CHK(lda_online_round(c, alpha, thresh, false));
    }
    if (n_rounds > 0) c->p_state.invalidate();
    return lda_online_record(st, c);       // a later step writes the tables this fold reads
}

}  // extern "C"
