// plsa_drivers.hpp -- the call frame of the fit entry points, plsa_fit and plsa_refit, and the backends the loops of
// plsa_fit_schedule.hpp drive; part of plsa_hip.hip's translation unit (included at its end: it uses the context and the pass
// wrappers defined there).  The frame (FitCall, fit_open, fit_run) is what plsa_fit, plsa_refit, plsa_fit_tempered,
// plsa_fit_smoothed and plsa_refit_smoothed share: the refusals, the fit_info reset, the weights, the likelihood tests, the
// final synchronise and the counts.  An entry point adds its eligibility, its scopes, its backend and the name of its loop.
// Also here, for the variants included after this file: what "the plain fused schedule" means (plain_fused) and the guard
// that stands one table in for another (StandIn).
#pragma once

#include "plsa_fit_schedule.hpp"

namespace {

// PLSA_REFERENCE_SUMS / PLSA_REFERENCE_LL of a driver call: in force for that call on top of plsa_set_arithmetic's setting
struct ArithmeticScope {
    plsa_ctx *c;
    bool sums, ll;
    ArithmeticScope(plsa_ctx *c_, int flags) : c(c_), sums(c_->ref_sums), ll(c_->ref_ll) {
        if (flags & PLSA_REFERENCE_SUMS) c->ref_sums = true;
        if (flags & PLSA_REFERENCE_LL) c->ref_ll = true;
    }
    ~ArithmeticScope() { c->ref_sums = sums; c->ref_ll = ll; }
};

struct ShardedScope {           // PLSA_SHARDED: this context's rows are one shard of the corpus
    plsa_ctx *c;
    ShardedScope(plsa_ctx *c_, bool on) : c(c_) { c->sharded = on; }
    ~ShardedScope() { c->sharded = false; }
};

// One materialised EM iteration of a driver (plsa_fit, plsa_refit): E-step into P(z|w,d), M-step from it -- in the reference
// arithmetic under a budget (plsa_set_p_budget) block by block when the plan has more than one block.
int run_driver_iteration(plsa_ctx *c, float thresh, const float *d_sw, bool update_v) {
    bool blocked = false;
    if (c->ref_sums && c->p_budget > 0) {
        if (c->P.borrowed || c->p_lent)
            return fail(c, "plsa_set_p_budget: a budget and a P(z|w,d) buffer that is %s do not mix -- end the loan or set the budget to 0",
                        c->P.borrowed ? "borrowed (plsa_p_borrow)" : "lent out (plsa_p_reserve)");
        CHK(ensure_ref_blocks(c));
        blocked = c->ref_blocks.blocks() > 1;
        if (c->P.cap > (size_t)c->p_budget) {      // left by a call without the budget: it goes before anything is allocated
            HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream2));
            c->P.release();
            c->p_state.invalidate();
        }
    }
    if (blocked) CHK(run_ref_em_blocked(c, thresh, d_sw, update_v));
    else {
        CHK(run_e_step(c, thresh));
        CHK(run_m_step_from_p(c, d_sw, update_v, nullptr));
    }
    if (c->ref_sums) {
        plsa_ctx::PBlockInfo &pi = c->p_block_info;
        pi.budget = c->p_budget;
        pi.blocks = blocked ? c->ref_blocks.blocks() : 1;
        pi.largest = blocked ? c->ref_blocks.largest : c->nnz;
        pi.p_bytes = (int64_t)c->P.cap;
    }
    return 0;
}

// The materialised loop of both drivers (flags without PLSA_FUSED, and the reference arithmetic): the reference's kernel
// sequence E-step -> M-step -> k_loglik.  d_sw_m: the weights of the M-step; update_v = false: the refit, topics frozen.
struct MaterialisedBackend {
    plsa_ctx *c;
    const float *d_sw, *d_sw_m;
    float thresh;
    bool update_v;
    MaterialisedBackend(plsa_ctx *c_, const float *d_sw_, const float *d_sw_m_, float thresh_, bool update_v_)
        : c(c_), d_sw(d_sw_), d_sw_m(d_sw_m_), thresh(thresh_), update_v(update_v_) {
        // reference arithmetic: the E-step leaves its tile sums with the weights the M-step will use; no norm_pwz chain
        // follows the E-steps of a refit, their tile sums would be wasted
        c->ref_e_sw = d_sw_m; c->ref_e_no_sums = !update_v;
    }
    ~MaterialisedBackend() { c->ref_e_sw = nullptr; c->ref_e_no_sums = false; }
    int loglik(double *ll) { return run_loglik(c, d_sw, ll); }
    int iteration() { return run_driver_iteration(c, thresh, d_sw_m, update_v); }      // plsa.py:597, 606-628
};

// what the fused backends share: the likelihood a document pass carried, finished from the pass's `blocks` partial sums
struct RidingLikelihood {
    plsa_ctx *c;
    const float *d_sw;
    float thresh;
    int blocks = 0;
    int loglik(double *ll) { return run_loglik(c, d_sw, ll); }
    int ll_send() { return finish_ll(c, blocks, nullptr); }
    int ll_wait(double *ll) { return wait_ll(c, ll); }
    int ll_now(double *ll) { return finish_ll(c, blocks, ll); }
};

// plsa_refit fused: the document pass alone, no look-ahead.  The refit M-step ignores sample weights for P(z|d)
// (plsa.py:806-809); they only enter the log-likelihood, which the pass accumulates when a test is pending.
struct RefitBackend : RidingLikelihood {
    int begin() { return 0; }
    int join() { return 0; }
    int enqueue(bool want_ll) { return run_row_pass(c, false, want_ll, d_sw, thresh, nullptr, &blocks); }
    void advance() { c->cu ^= 1; }
    int enqueue_pair() { return fail(c, "internal: plsa_refit has no look-ahead"); }
    void mark() {}
    void restore() {}
};

// plsa_fit fused.  How the two halves of an iteration share the chip is decided once per call:
enum class Topology {
    // small corpora leave CUs idle inside each kernel (measured: config 1 0.50 -> 0.37 ms, config 2 0.43 -> 0.37 ms per
    // iteration; neutral at config 3, -6 % at config 5): the document pass (VALU-heavy, gathers the small topic table) and
    // the column chain (fabric-bound gathers of P(z|d) rows) read the same current factors and write disjoint outputs, so
    // they run on two streams and their stalls overlap.
    //   PIPELINES: the column chain of successive iterations is one dependency chain (column pass -> tail -> next column
    //   pass): it stays back to back on the second stream, and the two streams only exchange "document pass i done" /
    //   "column chain i done" events.  A fork + join through the first stream put two cross-stream hops (17 us of 121 at
    //   config 1) between tail i and column pass i+1.
    PIPELINES,
    FORK_BOTH,      // fork / join around both passes (a hipGraph is requested, or PLSA_PIPELINE=0)
    // large corpora: both passes saturate the memory system on their own, but the short chain of column sums /
    // normalisation after the column pass leaves the chip nearly idle -- it runs on the second stream underneath the
    // document pass
    FORK_TAIL,
    // PLSA_OVERLAP=0, and PLSA_SHARDED: every collective of the communicator goes on c->stream in program order (accumulator
    // all-reduce, then the likelihood all-reduce) -- no second stream, identical order on every rank
    ONE_STREAM,
};

struct FusedFitBackend : RidingLikelihood {
    const float *d_sw_m;             // the weights of the M-step
    Topology topology;
    plsa::fit::Form form;            // speculate: the loop's look-ahead writes a THIRD set of factor buffers (fit::run_fused)
    bool begun = false;
    int su = 0, sv = 0;              // the factors a stop returns
    // PLSA_GRAPH (flag or environment): the iterations between two likelihood tests replayed from a hipGraph of TWO
    // iterations (the double buffers alternate, a pair returns to the starting buffers; the single eager iteration of a
    // likelihood test flips the parity, hence one graph per starting pair), captured from enqueue()'s launch sequence.
    // Kernel arguments are baked into the graph, so it lives for this call only.  Off by default: measured neutral
    // (the host is not the bound, and a dependent kernel boundary costs the same 1.5 us eager or replayed)
    hipGraphExec_t gexecs[4] = {nullptr, nullptr, nullptr, nullptr};   // one per starting buffer pair (cu, cv)

    FusedFitBackend(plsa_ctx *c_, const float *d_sw_, const float *d_sw_m_, float thresh_, int flags, int n_iter, int n_iter_per_test)
        : RidingLikelihood{c_, d_sw_, thresh_}, d_sw_m(d_sw_m_) {
        const bool overlap = c->overlap && !c->sharded, small = (double)c->nnz * c->kp < c->overlap_full_limit;
        form.graph = ((flags & PLSA_GRAPH) || c->graph) && !c->sharded && !c->timing;
        // Speculation across a likelihood test: the host used to wait for the test's likelihood before enqueuing the next
        // iteration -- an idle chip for one host round trip plus the launch latency of the next passes, every
        // n_iter_per_test iterations (config 2: ~40 us per test = 2.3 % of the run).  n_iter_per_test >= 2: no test rides
        // on the pass enqueued ahead.
        form.speculate = (c->speculate > 0 || (c->speculate < 0 && small)) && !c->sharded && !form.graph &&
                         n_iter_per_test >= 2 && n_iter >= 3;
        topology = !overlap ? Topology::ONE_STREAM
                   : !small ? Topology::FORK_TAIL
                            : (!form.graph && c->pipeline) ? Topology::PIPELINES : Topology::FORK_BOTH;
        c->fit_info.pipelined = topology == Topology::PIPELINES;
        c->fit_info.speculated = form.speculate;
    }
    ~FusedFitBackend() {
        for (auto e : gexecs) if (e) (void)hipGraphExecDestroy(e);
        if (c->rot3) {               // leaves cu, cv in {0, 1} (everything outside the loop addresses the alternate as 1 - cu)
            c->rot3 = false;
            if (c->cu == 2) { std::swap(c->U[2], c->U[0]); c->cu = 0; }
            if (c->cv == 2) { std::swap(c->Vt[2], c->Vt[0]); c->cv = 0; }
        }
        // whatever way the loop is left, the column chain has finished before the call returns
        if (begun && topology == Topology::PIPELINES) (void)hipStreamSynchronize(c->stream2);
    }

    int begin() {
        if (topology == Topology::PIPELINES) {      // everything enqueued so far (factors, corpus) precedes both pipelines
            HIPCHK(c, hipEventRecord(c->ev_row, c->stream));
            HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_row, 0));
            HIPCHK(c, hipEventRecord(c->ev_tail, c->stream2));
        }
        begun = true;
        if (form.speculate) {
            CHK(ensure(c, c->U[2], sizeof(float) * (size_t)c->n * c->kp));
            CHK(ensure(c, c->Vt[2], sizeof(float) * (size_t)c->m * c->kp));
            c->rot3 = true;
        }
        return 0;
    }
    // the last column chain precedes whatever follows
    int join() {
        if (topology == Topology::PIPELINES) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_tail, 0));
        return 0;
    }

    // one fused EM iteration from the factors in (cu, cv) into the alternate buffers (no swap here)
    int enqueue(bool want_ll) {
        if (topology == Topology::ONE_STREAM) {
            CHK(run_row_pass(c, false, want_ll, d_sw, thresh, nullptr, &blocks));
            CHK(run_col_pass(c, false, d_sw_m, thresh, 1));
            return run_col_tail(c);
        }
        const bool pipelines = topology == Topology::PIPELINES, tail_only = topology == Topology::FORK_TAIL;
        if (tail_only) CHK(run_col_pass(c, false, d_sw_m, thresh, 1));
        else {                       // both passes' structures and scratch are built on c->stream before anything forks
            ColLaunch col;
            RowLaunch row;
            CHK(prepare_col_pass(c, false, col));
            CHK(prepare_row_pass(c, false, want_ll, row));
        }
        if (pipelines) {
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_tail, 0));      // P(w|z) of the previous chain
            HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_row, 0));      // P(z|d) of the previous document pass
        } else {
            HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
            HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
        }
        {
            LaunchOn on2(c, c->stream2);
            if (!tail_only) CHK(run_col_pass(c, false, d_sw_m, thresh, 1));
            CHK(run_col_tail(c));
        }
        HIPCHK(c, hipEventRecord(pipelines ? c->ev_tail : c->ev_join, c->stream2));
        CHK(run_row_pass(c, false, want_ll, d_sw, thresh, nullptr, &blocks));
        if (pipelines) HIPCHK(c, hipEventRecord(c->ev_row, c->stream));
        else HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
        return 0;
    }

    int enqueue_pair() {
        hipGraphExec_t &gexec = gexecs[c->cu * 2 + c->cv];
        if (!gexec) {
            hipGraph_t graph = nullptr;
            HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
            int rc = enqueue(false);
            c->cu ^= 1; c->cv ^= 1;
            if (!rc) rc = enqueue(false);
            c->cu ^= 1; c->cv ^= 1;
            const hipError_t e_end = hipStreamEndCapture(c->stream, &graph);
            if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
            HIPCHK(c, e_end);
            const hipError_t e_inst = hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            HIPCHK(c, e_inst);
        }
        HIPCHK(c, hipGraphLaunch(gexec, c->stream));
        c->fit_info.graph_launches++;
        return 0;
    }

    void advance() {
        if (c->rot3) { c->cu = (c->cu + 1) % 3; c->cv = (c->cv + 1) % 3; } else { c->cu ^= 1; c->cv ^= 1; }
    }
    void mark() { su = c->cu; sv = c->cv; }
    void restore() { c->cu = su; c->cv = sv; }
};

// What the variants of the fit (tempered, smoothed, online, the member batch) run: the plain fused schedule in the default
// arithmetic.  The first reason a (context, flags) pair is not that, in the order the refusals report it.
enum class PlainFused { OK, NOT_FUSED, FORMLESS_FLAG, REFERENCE_CONTEXT };

PlainFused plain_fused(const plsa_ctx *c, int flags) {
    if (!(flags & PLSA_FUSED)) return PlainFused::NOT_FUSED;
    if (flags & (PLSA_SHARDED | PLSA_GRAPH | PLSA_REFERENCE_SUMS | PLSA_REFERENCE_LL)) return PlainFused::FORMLESS_FLAG;
    return c->ref_sums || c->ref_ll ? PlainFused::REFERENCE_CONTEXT : PlainFused::OK;
}

// the refusal of a class in the word of the variant (`form`: "tempered", "smoothed", "online"); OK: 0
int plain_fused_refusal(plsa_ctx *c, const char *who, const char *form, PlainFused cls, int flags = 0) {
    if (cls == PlainFused::NOT_FUSED) return fail(c, "%s: %s EM runs the fused passes only (flags without PLSA_FUSED)", who, form);
    if (cls == PlainFused::FORMLESS_FLAG)
        return fail(c, "%s: PLSA_SHARDED, PLSA_GRAPH, PLSA_REFERENCE_SUMS and PLSA_REFERENCE_LL have no %s form (flags=%d)", who, form, flags);
    if (cls == PlainFused::REFERENCE_CONTEXT)
        return fail(c, "%s: the context is in reference arithmetic (plsa_set_arithmetic), which has no %s form", who, form);
    return 0;
}

// A stand-in table in a place the passes read (c->U[c->cu], c->Vt[c->cv]) for the length of one launch chain: the launches
// are stream-ordered, so the pointers they were given stay valid, the buffers only change names on the host.
struct StandIn {
    DevBuf &place, &table;
    StandIn(DevBuf &place_, DevBuf &table_) : place(place_), table(table_) { place.swap(table); }
    ~StandIn() { place.swap(table); }
};

// ---- the call frame of the fit entry points ----
struct FitCall {                     // the C arguments every one of them takes
    const float *sw;
    int n_iter, n_iter_per_test;
    double tolerance;
    int flags;
    int32_t *iters_done;
    float *ll_trace;
    int32_t *n_ll;
};
struct FitRun {                      // what the frame hands a loop: the weights of the likelihood and of the M-step, the tests
    const float *d_sw, *d_sw_m;
    plsa::fit::Tests tests;
    bool trace;
    int iters = 0;
};

plsa::fit::Rule fit_rule(int flags) { return (flags & PLSA_STOP_NO_ZERO_ARM) ? plsa::fit::FIT_NO_ZERO_ARM : plsa::fit::FIT; }

// First half: the refusals every entry point shares, then the reset of fit_info.  An entry point's eligibility and its
// delegation come before it; its scopes (ArithmeticScope, ShardedScope) and what they refuse, between the halves.
int fit_open(plsa_ctx *c, const char *who, const FitCall &a) {
    HIPCHK(c, hipSetDevice(c->device));
    CHK(need_factors(c));
    if (a.n_iter < 0 || a.n_iter_per_test <= 0) return fail(c, "%s: bad n_iter / n_iter_per_test", who);
    c->fit_info = plsa_ctx::FitInfo{};
    return 0;
}

// Second half.  `loop(FitRun &)` builds the backend and calls plsa::fit::run_*: the backend is gone when it returns, so what
// its destructor restores is in place before the synchronise, and the caller's scopes end after it.  A failing loop returns
// at once.  plsa.py:606-628: with use_sample_weights == False the M-step ignores the weights, the log-likelihood
// (plsa.py:591, 631) still applies them.
template <class Loop>
int fit_run(plsa_ctx *c, const FitCall &a, plsa::fit::Rule rule, bool fused, Loop loop) {
    c->fit_info.fused = fused;
    const float *d_sw = nullptr;
    CHK(upload_sw(c, a.sw, &d_sw));
    FitRun run{d_sw, (a.flags & PLSA_SW_LL_ONLY) ? nullptr : d_sw, {a.ll_trace, a.tolerance, rule, a.n_iter_per_test},
               (a.flags & PLSA_TRACE_LL) != 0};
    CHK(loop(run));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (a.iters_done) *a.iters_done = run.iters;
    if (a.n_ll) *a.n_ll = run.tests.count;
    return 0;
}

}  // namespace

extern "C" {

// plsa_fit_inner, enstop/plsa.py:583-640.
//
// Materialised mode (flags without PLSA_FUSED) follows the reference's kernel sequence literally:
// E-step -> M-step -> (every n_iter_per_test iterations) log-likelihood.
//
// Fused mode never writes P(z|w,d); the likelihood of a test is accumulated for free inside the next iteration's document
// pass (fit::run_fused).
int plsa_fit(plsa_ctx *c, const float *sw, int32_t n_iter, int32_t n_iter_per_test, double tolerance,
             float thresh, int32_t flags, int32_t *iters_done, float *ll_trace, int32_t *n_ll) {
    const FitCall call{sw, n_iter, n_iter_per_test, tolerance, flags, iters_done, ll_trace, n_ll};
    CHK(fit_open(c, "plsa_fit", call));
    ArithmeticScope arithmetic_scope(c, flags);
    if ((c->ref_sums || c->ref_ll) && (flags & PLSA_SHARDED))
        return fail(c, "plsa_fit: PLSA_REFERENCE_SUMS / PLSA_REFERENCE_LL have no doc-sharded form (the reference's sums are single chains over all non-zeros)");
    // the reference arithmetic IS the reference's kernel sequence (E-step into P(z|w,d), M-step from it, likelihood): there is
    // one such arithmetic, so PLSA_FUSED has nothing to select there and is ignored
    const bool fused = (flags & PLSA_FUSED) && !c->ref_sums && !c->ref_ll;
    ShardedScope sharded_scope(c, (flags & PLSA_SHARDED) != 0);
    return fit_run(c, call, fit_rule(flags), fused, [&](FitRun &r) {
        if (!fused) {
            MaterialisedBackend backend(c, r.d_sw, r.d_sw_m, thresh, true);
            return plsa::fit::run_materialised(backend, r.tests, n_iter, r.trace, &r.iters);
        }
        FusedFitBackend backend(c, r.d_sw, r.d_sw_m, thresh, flags, n_iter, n_iter_per_test);
        return plsa::fit::run_fused(backend, r.tests, n_iter, r.trace, backend.form, &r.iters);
    });
}

// plsa_refit_inner, enstop/plsa.py:884-920: topics frozen, only P(z|d) moves.
int plsa_refit(plsa_ctx *c, const float *sw, int32_t n_iter, int32_t n_iter_per_test, double tolerance,
               float thresh, int32_t flags, int32_t *iters_done, float *ll_trace, int32_t *n_ll) {
    const FitCall call{sw, n_iter, n_iter_per_test, tolerance, flags, iters_done, ll_trace, n_ll};
    CHK(fit_open(c, "plsa_refit", call));
    ArithmeticScope arithmetic_scope(c, flags);
    const bool fused = (flags & PLSA_FUSED) && !c->ref_sums && !c->ref_ll;
    return fit_run(c, call, plsa::fit::REFIT, fused, [&](FitRun &r) {
        if (!fused) {
            MaterialisedBackend backend(c, r.d_sw, nullptr, thresh, false);
            return plsa::fit::run_materialised(backend, r.tests, n_iter, r.trace, &r.iters);
        }
        RefitBackend backend{{c, r.d_sw, thresh}};
        return plsa::fit::run_fused(backend, r.tests, n_iter, r.trace, plsa::fit::Form{false, false}, &r.iters);
    });
}

}  // extern "C"
