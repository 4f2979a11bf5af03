// plsa_online.hpp -- host side of online (stepwise) EM (include/plsa_hip_online.h); part of plsa_hip.hip's translation unit
// (included at its end: it uses the context, the pass wrappers and the normalisation kernels).
//
// A plsa_online state owns the topics V [m, kp], the running statistic S [m, kp], the slab sums and the norm of the global
// update, and the frame it shares with online LDA (OnlineFrame: a step counter and ONE event).  A step runs on the block context's one stream: the state's V is swapped into the place
// the block's passes read (c->Vt[c->cv], by a StandIn of plsa_drivers.hpp) for the length of the pass chain, then the blend, the
// norm and the division follow on the same stream.  Steps on different contexts are ordered on the device by the event:
// waited for by the stream at the start of a step or fold, recorded at its end.  No second stream, no look-ahead, no hipGraph.
#pragma once

// The frame of an online state, shared with online LDA (plsa_lda_online.hpp): where it lives, the shape of its [m, kp] tables,
// the step counter and ONE event.  A state derives from it and adds only its tables
struct OnlineFrame {
    plsa_ctx *home = nullptr;        // its device, its stream and staging buffer for the host <-> device copies of the tables
    int device = 0;
    i64 m = 0;
    int k = 0, kp = 0;
    Event ev;
    bool recorded = false;           // ev has been recorded at least once
    int64_t t = 0;                   // steps taken since the tables were last set
    size_t table_bytes() const { return sizeof(float) * (size_t)m * kp; }
};

struct plsa_online : OnlineFrame {
    DevBuf S, V, slabs, norm;
};

namespace {

// what another context's step or fold enqueued precedes what this one enqueues
int online_wait(OnlineFrame *st, plsa_ctx *c) {
    if (st->recorded) HIPCHK(c, hipStreamWaitEvent(c->stream, st->ev, 0));
    return 0;
}
int online_record(OnlineFrame *st, plsa_ctx *c) {
    HIPCHK(c, hipEventRecord(st->ev, c->stream));
    st->recorded = true;
    return 0;
}
// the host waits for the last step or fold (before it reads or writes the state's tables through the home stream)
int online_host_wait(OnlineFrame *st) {
    plsa_ctx *h = st->home;
    HIPCHK(h, hipSetDevice(st->device));
    if (st->recorded) HIPCHK(h, hipEventSynchronize(st->ev));
    return 0;
}

// *_create: the argument checks (`out_name`: what the refusal calls a NULL `out`), the frame's fields and kp, then `tables`
// (the state's own allocations and clears on the home stream), waited for, and the event
template <class State, class Tables>
int online_create(plsa_ctx *home, const char *who, const char *out_name, int64_t m, int32_t k, State **out, Tables tables) {
    if (!out) return fail(home, "%s: %s is NULL", who, out_name);
    *out = nullptr;
    if (!home) return fail(nullptr, "%s: no home context", who);
    HIPCHK(home, hipSetDevice(home->device));
    if (k <= 0 || k > 1024) return fail(home, "%s: k=%d outside [1,1024]", who, k);
    if (m <= 0 || m >= ((int64_t)1 << 31) - 1) return fail(home, "%s: m=%lld outside [1, 2^31 - 2]", who, (long long)m);
    std::unique_ptr<State> owner(new State());
    State *st = owner.get();
    st->home = home; st->device = home->device; st->m = m; st->k = k;
    st->kp = plsa::plan::lane_shape(k, home->chunks_per_lane, home->row_shape_8x2).kp;
    static_assert(plsa::plan::BLEND_MAX_KP >= 1024, "k <= 1024");
    CHK(tables(st));
    HIPCHK(home, hipStreamSynchronize(home->stream));
    HIPCHK(home, hipEventCreateWithFlags(&st->ev.h, hipEventDisableTiming));
    *out = owner.release();
    return 0;
}

template <class State>
void online_destroy(State *st) {
    if (!st) return;
    (void)hipSetDevice(st->device);
    if (st->recorded) (void)hipEventSynchronize(st->ev);
    delete st;
}

// a [m, kp] table of the state, allocated and cleared on the home stream
int online_table(OnlineFrame *st, DevBuf &table) {
    CHK(ensure(st->home, table, st->table_bytes()));
    HIPCHK(st->home, hipMemsetAsync(table.p, 0, st->table_bytes(), st->home->stream));
    return 0;
}

// the refusals of a step or fold that look at the state and the block context only; launches nothing.  `form` ("online",
// "online LDA") goes into the plain-fused refusal, `no_shards` is the sentence behind a communicator's shard, `holds` ("topics",
// "lambda") what the state is said to hold
int online_frame_eligible(OnlineFrame *st, plsa_ctx *c, const char *who, const char *form, const char *no_shards, const char *holds,
                          int flags) {
    if (!st) return fail(c, "%s: no state", who);
    CHK(plain_fused_refusal(c, who, form, plain_fused(c, flags), flags));
    if (c->sharded || c->comm) return fail(c, "%s: %s", who, no_shards);
    if (c->device != st->device) return fail(c, "%s: the state lives on device %d, the block context on device %d", who, st->device, c->device);
    CHK(need_factors(c));
    if (c->m != st->m || c->k != st->k || c->kp != st->kp)
        return fail(c, "%s: the state holds %s for %lld words with k=%d, the block context has %lld words with k=%d", who, holds,
                    (long long)st->m, st->k, (long long)c->m, c->k);
    return 0;
}

int online_eligible(plsa_online *st, plsa_ctx *c, const char *who, int flags) {
    CHK(online_frame_eligible(st, c, who, "online", "the context is one shard of a communicator; online EM has no doc-sharded form",
                              "topics", flags));
    if (c->Vt[c->cv].cap < st->table_bytes()) return fail(c, "internal: %s: the block's topic table is smaller than the state's", who);
    return 0;
}

// frozen-topic iterations: the document pass of the fused refit, P(z|d) of the block only
int online_fold_in(plsa_ctx *c, int n_iter, const float *d_sw, float thresh) {
    for (int i = 0; i < n_iter; ++i) {
        CHK(run_row_pass(c, false, false, d_sw, thresh, nullptr, nullptr));
        c->cu ^= 1;
    }
    return 0;
}

// S' = b Vacc + a S with its slab sums, norm, V' = S' / norm: three launches on the block's stream
int online_global_update(plsa_online *st, plsa_ctx *c, float a, float b) {
    const int nb = plsa::plan::blend_grid(st->m);
    {
        Scope s(c, "k_online_blend");
        hipLaunchKernelGGL(plsa::k_online_blend, dim3(nb), dim3(plsa::plan::BLEND_BLOCK), 0, c->stream, st->S.as<float4>(),
                           c->Vacc.as<float4>(), (long long)st->m, st->kp, a, b, st->slabs.as<double>());
    }
    {
        Scope s(c, "k_colsum_final");
        hipLaunchKernelGGL(plsa::k_colsum_final, dim3(1), dim3(256), 0, c->stream, st->slabs.as<double>(), nb, st->kp,
                           st->norm.as<float>());
    }
    {
        Scope s(c, "k_v_normalise");
        const i64 total4 = st->m * st->kp / 4;
        hipLaunchKernelGGL(plsa::k_v_normalise, dim3(grid_for(c, total4, 256)), dim3(256), st->kp * sizeof(float), c->stream,
                           st->S.as<float>(), st->V.as<float>(), (int)st->m, st->kp, st->norm.as<float>());
    }
    return launch_check(c, "k_online_blend");
}

// host [k, m] -> one of the state's tables [m, kp] (0 at the pads; divide_by: every entry divided by it first, in float32),
// through the home context's staging buffer and stream; wait: synchronous, otherwise the caller waits
int online_upload(OnlineFrame *st, const float *host, DevBuf &table, float divide_by, bool wait) {
    plsa_ctx *h = st->home;
    const size_t count = (size_t)st->k * st->m;
    std::vector<float> scaled;
    if (divide_by != 1.0f) {
        scaled.resize(count);
        for (size_t i = 0; i < count; ++i) scaled[i] = host[i] / divide_by;
        host = scaled.data();
    }
    CHK(ensure(h, h->tmp0, sizeof(float) * count));
    HIPCHK(h, hipMemcpyAsync(h->tmp0.p, host, sizeof(float) * count, hipMemcpyHostToDevice, h->stream));
    const iplan::Grid2 g = iplan::transpose_grid(st->m, st->kp);
    hipLaunchKernelGGL(plsa::k_v_to_vt, dim3(g.x, g.y), dim3(256), 0, h->stream, h->tmp0.as<float>(), table.as<float>(), st->k,
                       (int)st->m, st->kp);
    CHK(launch_check(h, "k_v_to_vt"));
    if (wait) HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int online_download(OnlineFrame *st, const DevBuf &table, float *host) {
    plsa_ctx *h = st->home;
    const size_t count = (size_t)st->k * st->m;
    CHK(ensure(h, h->tmp0, sizeof(float) * count));
    const iplan::Grid2 g = iplan::transpose_grid(st->m, st->kp);
    hipLaunchKernelGGL(plsa::k_vt_to_v, dim3(g.x, g.y), dim3(256), 0, h->stream, table.as<float>(), h->tmp0.as<float>(), st->k,
                       (int)st->m, st->kp);
    CHK(launch_check(h, "k_vt_to_v"));
    CHK(copy_to_host(h, host, h->tmp0.p, sizeof(float) * count));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

}  // namespace

extern "C" {

int plsa_online_create(plsa_ctx *home, int64_t m, int32_t k, plsa_online **out) {
    return online_create(home, "plsa_online_create", "out", m, k, out, [](plsa_online *st) {
        CHK(online_table(st, st->S));
        CHK(online_table(st, st->V));
        CHK(ensure(st->home, st->slabs, sizeof(double) * (size_t)plsa::plan::blend_grid(st->m) * st->kp));
        return ensure(st->home, st->norm, sizeof(float) * (size_t)st->kp);
    });
}

void plsa_online_destroy(plsa_online *st) { online_destroy(st); }

int plsa_online_set_topics(plsa_online *st, const float *V) {
    if (!st) return fail(nullptr, "plsa_online_set_topics: no state");
    if (!V) return fail(st->home, "plsa_online_set_topics: V is NULL");
    CHK(online_host_wait(st));
    CHK(online_upload(st, V, st->V, 1.0f, true));
    CHK(online_upload(st, V, st->S, (float)st->k, true));
    st->t = 0;
    return 0;
}

int plsa_online_get_topics(plsa_online *st, float *V) {
    if (!st) return fail(nullptr, "plsa_online_get_topics: no state");
    if (!V) return fail(st->home, "plsa_online_get_topics: V is NULL");
    CHK(online_host_wait(st));
    return online_download(st, st->V, V);
}

int plsa_online_statistic_get(plsa_online *st, float *S, int64_t *steps) {
    if (!st) return fail(nullptr, "plsa_online_statistic_get: no state");
    CHK(online_host_wait(st));
    if (steps) *steps = st->t;
    return S ? online_download(st, st->S, S) : 0;
}

int plsa_online_statistic_set(plsa_online *st, const float *S) {
    if (!st) return fail(nullptr, "plsa_online_statistic_set: no state");
    if (!S) return fail(st->home, "plsa_online_statistic_set: S is NULL");
    CHK(online_host_wait(st));
    return online_upload(st, S, st->S, 1.0f, true);
}

int plsa_online_step(plsa_online *st, plsa_ctx *c, const float *sw, int32_t inner_iter, float thresh, double rho, double scale,
                     int32_t flags, double *ll_partial) {
    if (!c) return fail(nullptr, "plsa_online_step: no block context");
    CHK(online_eligible(st, c, "plsa_online_step", flags));
    if (!(rho > 0.0 && rho <= 1.0)) return fail(c, "plsa_online_step: rho=%g outside (0, 1]", rho);
    if (!(scale > 0.0) || !std::isfinite(scale)) return fail(c, "plsa_online_step: scale=%g is not a positive number", scale);
    if (inner_iter < 0) return fail(c, "plsa_online_step: inner_iter=%d is negative", inner_iter);
    const float a = (float)(1.0 - rho), b = (float)(rho * scale);
    HIPCHK(c, hipSetDevice(c->device));
    const float *d_sw = nullptr;
    CHK(upload_sw(c, sw, &d_sw));
    CHK(online_wait(st, c));
    int blocks = 0;
    {
        StandIn topics(c->Vt[c->cv], st->V);
        CHK(online_fold_in(c, inner_iter, d_sw, thresh));
        CHK(run_row_pass(c, false, ll_partial != nullptr, d_sw, thresh, nullptr, &blocks));
        CHK(run_col_pass(c, false, d_sw, thresh));
    }
    c->cu ^= 1;
    c->p_state.invalidate();
    if (ll_partial) CHK(finish_ll(c, blocks, nullptr));      // the scalar travels while the update runs
    CHK(online_global_update(st, c, a, b));
    CHK(online_record(st, c));
    st->t += 1;
    if (ll_partial) CHK(wait_ll(c, ll_partial));              // the only host wait of a step
    return 0;
}

int plsa_online_fold(plsa_online *st, plsa_ctx *c, const float *sw, int32_t n_iter, float thresh, int32_t flags) {
    if (!c) return fail(nullptr, "plsa_online_fold: no block context");
    CHK(online_eligible(st, c, "plsa_online_fold", flags));
    if (n_iter < 0) return fail(c, "plsa_online_fold: n_iter=%d is negative", n_iter);
    HIPCHK(c, hipSetDevice(c->device));
    const float *d_sw = nullptr;
    CHK(upload_sw(c, sw, &d_sw));
    CHK(online_wait(st, c));
    {
        StandIn topics(c->Vt[c->cv], st->V);
        CHK(online_fold_in(c, n_iter, d_sw, thresh));
    }
    if (n_iter > 0) c->p_state.invalidate();
    return online_record(st, c);       // a later step writes the topics this fold reads
}

}  // extern "C"
