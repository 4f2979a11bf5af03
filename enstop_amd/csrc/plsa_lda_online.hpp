// plsa_lda_online.hpp -- host side of online variational Bayes LDA (enstop_amd/include/plsa_hip_lda_online.h, DESIGN.md section
// 21); part of plsa_hip.hip's translation unit (included at its end, behind plsa_lda_priors.hpp: it uses the context, the pass
// wrappers, the round, the bound and the topic-side table routine of plsa_lda.hpp and the state frame of plsa_online.hpp).
//
// A plsa_lda_online state owns lambda [m, kp], the table B formed from it, B's float64 side arrays (S_z [kp], psi(S_z) [kp],
// the shift per word [m] -- the tail of a context's lda.sums, in its order), the slab partials of the column sums, and the
// frame of an online state (OnlineFrame: a step counter and ONE event).  A step or fold runs on the block context's one stream.  For its length the state's B stands in for
// the block's side table c->lda.B (StandIn) with b_valid set, and the side arrays are copied into the tail of the block's
// lda.sums, so every kernel of the block that reads the topic side -- the passes through run_lda_table_v's validity flag,
// k_lda_shift_sum for the bound -- reads the state's; the block's own topic table Vt is never read or written.  The blend,
// the topic sums, the word shifts and the table follow on the same stream, on the state's buffers.  Steps on different
// contexts are ordered on the device by the event.  No second stream, no look-ahead, no hipGraph.
#pragma once

struct plsa_lda_online : OnlineFrame {
    DevBuf lam, B, sums, slabs;
};

namespace {

size_t lda_online_side_count(const plsa_lda_online *st) { return 2 * (size_t)st->kp + (size_t)st->m; }

// the state's topic side for run_lda_topic_tables: lambda, B, the slab partials and the side arrays S_z, psi(S_z), the shift
// per word
LdaTopicSide lda_online_side(plsa_lda_online *st) {
    double *sums = st->sums.as<double>();
    return {st->lam.as<float4>(), st->B.as<float4>(), st->slabs.as<double>(), sums, sums + st->kp, sums + 2 * (size_t)st->kp,
            st->m, st->k, st->kp};
}

// every refusal of a step or fold that looks at the state, the block context and the arguments; launches nothing
int lda_online_eligible(plsa_lda_online *st, plsa_ctx *c, const char *who, double alpha, double eta, int flags) {
    if (!st) return fail(c, "%s: no state", who);
    CHK(lda_prior_ok(c, who, "alpha", alpha));
    CHK(lda_prior_ok(c, who, "eta", eta));
    return online_frame_eligible(st, c, who, "online LDA",
                                 "the context is a shard of a communicator (plsa_comm_init); online LDA has no multi-GPU form", "lambda",
                                 flags);
}

// lambda' = b Vacc + (a lambda + c) with its slab sums (in the place of k_lda_topic_partial's sweep), then the tables of lambda':
// four launches on the block's stream
int lda_online_global_update(plsa_lda_online *st, plsa_ctx *c, float a, float b, float cc) {
    {
        Scope s(c, "k_lda_online_blend");
        hipLaunchKernelGGL(plsa::k_lda_online_blend, dim3(plsa::plan::blend_grid(st->m)), dim3(plsa::plan::BLEND_BLOCK), 0, c->ls,
                           st->lam.as<float4>(), c->Vacc.as<float4>(), (long long)st->m, st->kp, st->k, a, b, cc,
                           st->slabs.as<double>());
    }
    CHK(launch_check(c, "k_lda_online_blend"));
    return run_lda_topic_tables(c, lda_online_side(st), false, true);
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

}  // namespace

extern "C" {

int plsa_lda_online_create(plsa_ctx *home, int64_t m, int32_t k, plsa_lda_online **out) {
    return online_create(home, "plsa_lda_online_create", "state", m, k, out, [](plsa_lda_online *st) {
        CHK(online_table(st, st->lam));
        CHK(online_table(st, st->B));
        CHK(ensure(st->home, st->sums, sizeof(double) * lda_online_side_count(st)));
        CHK(ensure(st->home, st->slabs, sizeof(double) * (size_t)plsa::plan::blend_grid(st->m) * st->kp));
        HIPCHK(st->home, hipMemsetAsync(st->sums.p, 0, sizeof(double) * lda_online_side_count(st), st->home->stream));
        return 0;
    });
}

void plsa_lda_online_destroy(plsa_lda_online *st) { online_destroy(st); }

int plsa_lda_online_set_lambda(plsa_lda_online *st, const float *lam) {
    if (!st) return fail(nullptr, "plsa_lda_online_set_lambda: no state");
    plsa_ctx *h = st->home;
    if (!lam) return fail(h, "plsa_lda_online_set_lambda: lam is NULL");
    CHK(online_host_wait(st));
    CHK(online_upload(st, lam, st->lam, 1.0f, false));       // the caller waits: below, behind the tables
    CHK(run_lda_topic_tables(h, lda_online_side(st), true, true));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    st->t = 0;
    return 0;
}

int plsa_lda_online_get_lambda(plsa_lda_online *st, float *lam, int64_t *steps) {
    if (!st) return fail(nullptr, "plsa_lda_online_get_lambda: no state");
    CHK(online_host_wait(st));
    if (steps) *steps = st->t;
    return lam ? online_download(st, st->lam, lam) : 0;
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
    CHK(online_wait(st, c));
    CHK(LdaOnlineTopicSide::prepare(st, c));
    {
        LdaOnlineTopicSide side(st, c);
        // the block's raw counts stay in Vacc: its Vt is neither written nor flipped
        CHK(lda_rounds(c, thresh, lda_scalar_rows(c, alpha), LdaColumns::COUNTS, eta).iteration(doc_iter));
        // the bound of the block without the topic part, at the state in force: the scalar travels while the update runs
        if (bound_partial) CHK(lda_bound_send(c, who, lda_gamma_part(c, alpha), eta, false));
    }
    c->p_state.invalidate();
    CHK(lda_online_global_update(st, c, a, b, cc));
    CHK(online_record(st, c));
    st->t += 1;
    // the only host wait of a step
    return bound_partial ? lda_bound_finish(c, lda_doc_constant(c, alpha), eta, false, bound_partial) : 0;
}

int plsa_lda_online_fold(plsa_lda_online *st, plsa_ctx *c, double alpha, int32_t n_rounds, float thresh, int32_t flags) {
    const char *who = "plsa_lda_online_fold";
    if (!c) return fail(nullptr, "%s: no block context", who);
    CHK(lda_online_eligible(st, c, who, alpha, 1.0, flags));
    if (n_rounds < 0) return fail(c, "%s: n_rounds=%d is negative", who, n_rounds);
    HIPCHK(c, hipSetDevice(c->device));
    CHK(online_wait(st, c));
    CHK(LdaOnlineTopicSide::prepare(st, c));
    {
        LdaOnlineTopicSide side(st, c);
        auto rounds = lda_rounds(c, thresh, lda_scalar_rows(c, alpha), LdaColumns::NONE, 1.0);
        for (int r = 0; r < n_rounds; ++r) CHK(rounds.round(false));
    }
    if (n_rounds > 0) c->p_state.invalidate();
    return online_record(st, c);       // a later step writes the tables this fold reads
}

}  // extern "C"
