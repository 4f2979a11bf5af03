// plsa_members.hpp -- host side of the batched ensemble members (include/plsa_hip_members.h); part of plsa_hip.hip's
// translation unit (included at its end: it uses the context, the builders and the launch helpers defined there).
//
// Layout of a batch.  Every member slot is a plsa_ctx of its own that BORROWS the leader's streams and base corpus:
// its resample, lane shape and factors are built by the code a standalone fit runs (plsa_bootstrap, mt_init /
// plsa_set_factors), and its structures, scratch and grids come from the two preparations a standalone pass launches from
// (prepare_col_pass, prepare_row_pass), with the member's own n, nnz and kp -- so item lengths, the row-item decision,
// heavy-column lists, chunk counts and grids are the standalone ones by construction.
// The builders' scratch (tmp0..2, cubtmp, the MT19937 words) is the LEADER's, lent for the duration of a call.
// plsa_members_fit then groups the members by kernel instantiation (packed column stream, packed document stream), fills
// one plsa::MemberArgs per member and runs the fused schedule with one launch per kernel and group
// (plsa_member_kernels.hpp); a group of one, and every member of an ineligible call, goes through plsa_fit.
#pragma once

struct plsa_members {
    struct MemberDelete {
        void operator()(plsa_ctx *m) const {
            if (!m) return;
            m->stream.h = nullptr; m->stream2.h = nullptr;        // the leader's
            delete m;                                             // (borrowed DevBufs are not freed)
        }
    };
    using Member = std::unique_ptr<plsa_ctx, MemberDelete>;
    plsa_ctx *leader = nullptr;
    std::vector<Member> ctx;
    std::vector<char> prepared;
    struct Info { int group = -1, group_size = 0, items = 0, rseg = 0, n_chunks = 0, n_heavy = 0, row_grid = 0, norm_blocks = 0; };
    std::vector<Info> info;
    std::vector<double> last_ll;     // the float64 likelihood of each member's last test (plsa_members_last_ll)
    DevBuf table, ll_out;            // plsa::MemberArgs[n], double[n]
    Pinned<double> h_ll;
};

namespace {

int new_member(plsa_ctx *leader, plsa_members::Member &out) {
    plsa_members::Member m(new plsa_ctx());
    m->device = leader->device;
    m->prop = leader->prop;
    m->stream.h = leader->stream.h;
    m->stream2.h = leader->stream2.h;
    m->ls = m->stream;
    if (hipEventCreateWithFlags(&m->ev_fork.h, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev_join.h, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev_row.h, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev_tail.h, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev_ll.h, hipEventDisableTiming) != hipSuccess ||
        host_alloc(m->h_ll, 2) != hipSuccess)
        return fail(leader, "plsa_members: event / pinned buffer creation failed");
    read_knobs(m.get());
    out = std::move(m);
    return 0;
}

// the leader's builder scratch serves the member for the duration of a call (everything runs on the one shared stream)
struct ScratchLoan {
    plsa_ctx *l, *m;
    void swap_all() {
        for (auto p : {&plsa_ctx::tmp0, &plsa_ctx::tmp1, &plsa_ctx::tmp2, &plsa_ctx::cubtmp, &plsa_ctx::pk_count, &plsa_ctx::mt_words,
                       &plsa_ctx::mt_state, &plsa_ctx::mt_fin, &plsa_ctx::mt_poly, &plsa_ctx::mt_seq})
            (l->*p).swap(m->*p);
    }
    ScratchLoan(plsa_ctx *l_, plsa_ctx *m_) : l(l_), m(m_) { swap_all(); }
    ~ScratchLoan() { swap_all(); }
};

// a member's failure is reported through the leader (plsa_last_error of the batch's context)
int member_rc(plsa_ctx *leader, plsa_ctx *m, int rc) {
    if (rc) leader->err = m->err;
    return rc;
}

int members_check(plsa_members *b, int32_t member) {
    if (!b) return fail(nullptr, "plsa_members: NULL batch");
    if (member < 0 || member >= (int32_t)b->ctx.size())
        return fail(b->leader, "plsa_members: member %d outside [0, %d)", member, (int)b->ctx.size());
    return 0;
}

// one member's fused iteration -> one table row: the two preparations a standalone fit launches from (prepare_col_pass,
// prepare_row_pass; every member's document pass may carry the likelihood), copied field by field
int member_args(plsa_ctx *c, double *ll_out, plsa::MemberArgs &a, plsa_members::Info &inf) {
    ColLaunch l;
    RowLaunch r;
    CHK(prepare_col_pass(c, false, l));
    CHK(prepare_row_pass(c, false, true, r));
    a = plsa::MemberArgs{};
    a.item_rec = l.item_rec;
    a.csc_row = l.csc_row;
    a.csc_val = l.csc_val;
    a.slot = l.slot;
    a.partial = l.partial;
    a.chunk_sums = l.colsum_rows;
    a.n_items = l.n_items;
    a.chunk_sums2 = l.colsum_rows2;
    a.norm_pwz = l.norm_pwz;
    a.item_first = l.item_first;
    a.heavy_cols = l.heavy_cols;
    a.n_chunks = l.plan.n_chunks;
    a.norm_blocks = l.plan.norm_blocks;
    a.m = (int)c->m;
    a.n_heavy = l.n_heavy;
    a.heavy_items = l.heavy_items;
    a.reduce_grid = l.plan.reduce_grid;
    a.indptr = r.indptr;
    a.colidx = r.colidx;
    a.vals = r.vals;
    a.sblk = r.sblk;
    a.row_order = r.order;
    a.ritem_row = r.ritem_row;
    a.ritem_start = r.ritem_start;
    a.ritem_first = r.ritem_first;
    a.rpartial = r.rpartial;
    a.ll_partials = r.ll_partials;
    a.ll_out = ll_out;
    a.n_ritems = r.n_ritems;
    a.n = (int)c->n;
    a.rseg = r.rseg;
    a.row_grid = r.plan.grid;
    a.row_reduce_grid = r.plan.reduce_grid;
    for (int i = 0; i < 2; ++i) { a.U[i] = c->U[i].as<float>(); a.Vt[i] = c->Vt[i].as<float>(); }
    inf.items = r.items; inf.rseg = r.rseg; inf.n_chunks = l.plan.n_chunks; inf.n_heavy = l.n_heavy;
    inf.row_grid = r.plan.grid; inf.norm_blocks = l.plan.norm_blocks;
    return 0;
}

// lane shape of the document pass, 32-bit gather offsets only (a batch carries no wide table)
template <class Fn>
int dispatch_narrow_row(plsa_ctx *c, Fn &&fn) {
    if (c->row_lpn == 8 && c->row_ch == 2 && c->kp == 64) { fn(plsa::Shape<8, 2, true>{}); return 0; }
    return dispatch_shape(c, fn);
}

// The fused schedule of plsa_fit for the members `who` (one instantiation group), every kernel launched once for all of
// them.  All live members are at the same iteration, so whether a pass carries the likelihood (the initial one on the
// first document pass, a due test later) is the same for all; the TEST is per member.
int fit_group(plsa_members *b, const std::vector<int> &who, const std::vector<plsa::MemberArgs> &rows, int n_iter,
              int n_iter_per_test, double tolerance, float thresh, int flags, int32_t *iters_done, float *ll_trace, int ll_cap,
              int32_t *n_ll) {
    plsa_ctx *L = b->leader, *c0 = b->ctx[who[0]].get();
    const int G = (int)who.size();
    const bool trace = flags & PLSA_TRACE_LL;
    HIPCHK(L, hipMemcpyAsync(b->table.p, rows.data(), sizeof(plsa::MemberArgs) * (size_t)G, hipMemcpyHostToDevice, L->stream));
    HIPCHK(L, hipStreamSynchronize(L->stream));      // (`rows` is the caller's; and the members' builders have finished)
    const plsa::MemberArgs *table = b->table.as<plsa::MemberArgs>();
    int row_x = 1, reduce_x = 1, chunks_x = 1, norm_x = 0, rr_x = 0;
    for (const auto &a : rows) {
        row_x = std::max(row_x, a.row_grid);
        reduce_x = std::max(reduce_x, a.reduce_grid);
        chunks_x = std::max(chunks_x, a.n_chunks);
        norm_x = std::max(norm_x, a.norm_blocks);
        if (a.ritem_row) rr_x = std::max(rr_x, a.row_reduce_grid);
    }
    const bool pk_row = c0->packed && c0->pk_csr.ok, pk_col = c0->packed && c0->pk_csc.ok;
    const bool tiny = thresh < plsa::TINY_THRESH;
    const int kp = c0->kp;
    using u64 = unsigned long long;
    u64 live = G == 64 ? ~0ull : ((1ull << G) - 1ull), cu = 0, cv = 0;
    for (int g = 0; g < G; ++g) {
        plsa_ctx *c = b->ctx[who[g]].get();
        if (c->cu) cu |= 1ull << g;
        if (c->cv) cv |= 1ull << g;
    }
    using F = std::false_type;           // a batch is fused and untimed: those two choices are fixed
    // The two halves of an iteration read the same current factors and write disjoint outputs: the column chain runs on
    // the leader's second stream underneath the document pass (fork / join per iteration, like plsa_fit's small-corpus form)
    const bool two_streams = L->overlap;
    hipStream_t col_stream = two_streams ? L->stream2.h : L->stream.h;
    auto row_pass = [&](bool want_ll) -> int {
        CHK(dispatch_narrow_row(c0, [&](auto S) {
            using Sh = decltype(S);
            select_row_pass<Sh>(pk_row, F{}, want_ll, tiny, [&](auto SS, auto, auto LL, auto TN) {
                hipLaunchKernelGGL((plsa::k_row_pass_members<decltype(SS), decltype(LL)::value, decltype(TN)::value>),
                                   dim3(row_x, G), dim3(256), 0, L->stream, table, live, cu, cv, kp, thresh);
            });
            if (rr_x > 0)
                hipLaunchKernelGGL((plsa::k_row_reduce_members<Sh>), dim3(rr_x, G), dim3(256), 0, L->stream, table, live, cu, kp);
        }));
        if (want_ll) {
            hipLaunchKernelGGL(plsa::k_ll_final_members, dim3(G), dim3(256), 0, L->stream, table, live);
            HIPCHK(L, hipMemcpyAsync(b->h_ll.get(), b->ll_out.p, sizeof(double) * (size_t)G, hipMemcpyDeviceToHost, L->stream));
        }
        return launch_check(L, "k_row_pass_members");
    };
    auto col_chain = [&]() -> int {
        CHK(dispatch_shape(c0, [&](auto S) {
            using Sh = decltype(S);
            constexpr int GPB = 256 / Sh::LPN;
            const size_t smem = sizeof(double) * (size_t)GPB * kp;
            select_col_pass<Sh>(pk_col, F{}, F{}, tiny, [&](auto SS, auto, auto, auto TN) {
                hipLaunchKernelGGL((plsa::k_col_pass_members<decltype(SS), decltype(TN)::value>), dim3(chunks_x, G), dim3(256),
                                   smem, col_stream, table, live, cu, cv, kp, thresh);
            });
            if (norm_x > 0)
                hipLaunchKernelGGL(plsa::k_norm_reduce_members, dim3(norm_x, G), dim3(256), 0, col_stream, table, live, kp);
            hipLaunchKernelGGL(plsa::k_colsum_final_members, dim3(G), dim3(256), 0, col_stream, table, live, kp);
            hipLaunchKernelGGL((plsa::k_col_reduce_norm_members<Sh>), dim3(reduce_x, G), dim3(256),
                               sizeof(float) * (size_t)(GPB + 1) * kp, col_stream, table, live, cv, kp);
        }));
        return launch_check(L, "k_col_pass_members");
    };
    std::vector<plsa::fit::Tests> tests;
    for (int g = 0; g < G; ++g)
        tests.push_back({ll_trace ? ll_trace + (size_t)who[g] * ll_cap : nullptr, tolerance,
                         fit_rule(flags), n_iter_per_test, ll_cap});
    std::vector<int> iters(G, 0);
    bool pending = false, first = true;
    for (int i = 0; i < n_iter && live; ++i) {
        const bool want_ll = pending || first;
        if (two_streams) {
            HIPCHK(L, hipEventRecord(L->ev_fork, L->stream));
            HIPCHK(L, hipStreamWaitEvent(L->stream2, L->ev_fork, 0));
        }
        CHK(col_chain());
        if (two_streams) HIPCHK(L, hipEventRecord(L->ev_join, L->stream2));
        CHK(row_pass(want_ll));
        if (two_streams) HIPCHK(L, hipStreamWaitEvent(L->stream, L->ev_join, 0));
        if (want_ll) {
            HIPCHK(L, hipStreamSynchronize(L->stream));
            for (int g = 0; g < G; ++g) {
                if (!((live >> g) & 1ull)) continue;
                b->last_ll[who[g]] = b->h_ll[g];
                if (first) tests[g].initial(b->h_ll[g]);
                else if (tests[g].test(b->h_ll[g])) live &= ~(1ull << g);    // this pass is discarded: no swap
            }
            first = false;
        }
        cu ^= live; cv ^= live;
        for (int g = 0; g < G; ++g) if ((live >> g) & 1ull) iters[g]++;
        pending = tests[0].due_after(i);
    }
    HIPCHK(L, hipStreamSynchronize(L->stream));
    for (int g = 0; g < G; ++g) {
        plsa_ctx *c = b->ctx[who[g]].get();
        c->cu = (int)((cu >> g) & 1ull); c->cv = (int)((cv >> g) & 1ull);
        c->p_state.invalidate();
        if (((live >> g) & 1ull) && pending && trace) {      // test of the last iteration: result-neutral (plsa_fit)
            ScratchLoan loan(L, c);
            double ll = 0.0;
            CHK(member_rc(L, c, run_loglik(c, nullptr, &ll)));
            b->last_ll[who[g]] = ll;
            tests[g].trailing(ll);
        }
        iters_done[who[g]] = iters[g];
        n_ll[who[g]] = tests[g].count;
    }
    return 0;
}

}  // namespace

extern "C" {

int plsa_members_create(plsa_ctx *ctx, int32_t n_members, plsa_members **out) {
    if (!out) return fail(ctx, "plsa_members_create: out is NULL");
    *out = nullptr;
    if (!ctx) return fail(nullptr, "plsa_members_create: NULL context");
    if (n_members < 1 || n_members > PLSA_MEMBERS_MAX)
        return fail(ctx, "plsa_members_create: n_members=%d outside [1, %d]", n_members, (int)PLSA_MEMBERS_MAX);
    static_assert(PLSA_MEMBERS_MAX == plsa::MEMBERS_MAX, "the live mask is one 64-bit word");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<plsa_members> b(new plsa_members());
    b->leader = ctx;
    b->ctx.resize(n_members);
    b->prepared.assign(n_members, 0);
    b->info.assign(n_members, plsa_members::Info{});
    b->last_ll.assign(n_members, 0.0);
    for (auto &m : b->ctx) CHK(new_member(ctx, m));
    CHK(ensure(ctx, b->table, sizeof(plsa::MemberArgs) * (size_t)n_members));
    CHK(ensure(ctx, b->ll_out, sizeof(double) * (size_t)n_members));
    if (host_alloc(b->h_ll, (size_t)n_members) != hipSuccess) return fail(ctx, "plsa_members_create: pinned buffer allocation failed");
    *out = b.release();
    return 0;
}

void plsa_members_destroy(plsa_members *b) {
    if (!b) return;
    (void)hipSetDevice(b->leader->device);
    (void)hipStreamSynchronize(b->leader->stream);
    (void)hipStreamSynchronize(b->leader->stream2);
    delete b;
}

int plsa_members_release(plsa_members *b) {
    if (!b) return fail(nullptr, "plsa_members: NULL batch");
    plsa_ctx *L = b->leader;
    HIPCHK(L, hipSetDevice(L->device));
    HIPCHK(L, hipStreamSynchronize(L->stream));
    HIPCHK(L, hipStreamSynchronize(L->stream2));
    for (size_t r = 0; r < b->ctx.size(); ++r) {      // fresh slots: everything a member held goes with its context
        plsa_members::Member fresh;
        CHK(new_member(L, fresh));
        b->ctx[r] = std::move(fresh);
        b->prepared[r] = 0;
        b->info[r] = plsa_members::Info{};
    }
    return 0;
}

int plsa_members_prepare(plsa_members *b, int32_t member, const int64_t *idx, int64_t n_out, int32_t k,
                         uint32_t *mt_state_io, const float *U, const float *V) {
    CHK(members_check(b, member));
    plsa_ctx *L = b->leader, *c = b->ctx[member].get();
    HIPCHK(L, hipSetDevice(L->device));
    if (L->bn <= 0) return fail(L, "plsa_members_prepare: no corpus uploaded");
    if (!mt_state_io && (!U || !V)) return fail(L, "plsa_members_prepare: neither a generator state nor host factors");
    b->prepared[member] = 0;
    // the base corpus is the leader's (uploaded once): the member views it
    if (c->bn != L->bn || c->bm != L->bm || c->bnnz != L->bnnz) c->bal_have_frac = false;
    c->b_indptr.borrow(L->b_indptr.p, L->b_indptr.cap);
    c->b_col.borrow(L->b_col.p, L->b_col.cap);
    c->b_val.borrow(L->b_val.p, L->b_val.cap);
    c->bn = L->bn; c->bm = L->bm; c->bnnz = L->bnnz;
    ScratchLoan loan(L, c);
    CHK(member_rc(L, c, plsa_bootstrap(c, idx, n_out)));
    if (mt_state_io) CHK(member_rc(L, c, mt_init(c, k, mt_state_io, nullptr)));
    else CHK(member_rc(L, c, plsa_set_factors(c, U, V, c->n, c->m, k)));
    b->prepared[member] = 1;
    return 0;
}

int plsa_members_fit(plsa_members *b, int32_t n_active, int32_t n_iter, int32_t n_iter_per_test, double tolerance,
                     float thresh, int32_t flags, int32_t *iters_done, float *ll_trace, int32_t ll_cap, int32_t *n_ll,
                     int32_t *n_batched) {
    if (!b) return fail(nullptr, "plsa_members: NULL batch");
    plsa_ctx *L = b->leader;
    HIPCHK(L, hipSetDevice(L->device));
    if (n_active < 1 || n_active > (int32_t)b->ctx.size()) return fail(L, "plsa_members_fit: n_active=%d outside [1, %d]", n_active, (int)b->ctx.size());
    if (n_iter < 0 || n_iter_per_test <= 0) return fail(L, "plsa_members_fit: bad n_iter / n_iter_per_test");
    if (!iters_done || !n_ll) return fail(L, "plsa_members_fit: iters_done / n_ll is NULL");
    if (ll_trace && ll_cap < n_iter + 2) return fail(L, "plsa_members_fit: ll_cap=%d below n_iter + 2", ll_cap);
    for (int r = 0; r < n_active; ++r) {
        if (!b->prepared[r]) return fail(L, "plsa_members_fit: member %d is not prepared", r);
        if (b->ctx[r]->k != b->ctx[0]->k) return fail(L, "plsa_members_fit: members differ in k");
        b->info[r] = plsa_members::Info{};
    }
    if (n_batched) *n_batched = 0;
    // what a batch carries: the fused schedule in the engine's own arithmetic, eager, untimed, 32-bit gather tables
    const bool call_ok = plain_fused(L, flags) == PlainFused::OK && !L->graph && !L->timing && !L->row_xcd && n_iter > 0;
    std::vector<plsa::MemberArgs> args(n_active);
    std::vector<int> key(n_active, -1);          // instantiation group: packed column stream | packed document stream
    if (call_ok)
        for (int r = 0; r < n_active; ++r) {
            plsa_ctx *c = b->ctx[r].get();
            if (table_is_wide(c, c->n) || table_is_wide(c, c->m) || c->nnz <= 0) continue;
            ScratchLoan loan(L, c);
            CHK(member_rc(L, c, member_args(c, b->ll_out.as<double>(), args[r], b->info[r])));
            key[r] = (c->packed && c->pk_csc.ok ? 1 : 0) | (c->packed && c->pk_csr.ok ? 2 : 0);
        }
    int n_groups = 0, batched = 0;
    for (int kk = 0; kk < 4; ++kk) {
        std::vector<int> who;
        std::vector<plsa::MemberArgs> rows;
        for (int r = 0; r < n_active; ++r) if (key[r] == kk) who.push_back(r);
        if (who.size() < 2) continue;
        for (size_t g = 0; g < who.size(); ++g) {
            rows.push_back(args[who[g]]);
            rows.back().ll_out = b->ll_out.as<double>() + g;
            b->info[who[g]].group = n_groups;
            b->info[who[g]].group_size = (int)who.size();
        }
        CHK(fit_group(b, who, rows, n_iter, n_iter_per_test, tolerance, thresh, flags, iters_done, ll_trace, ll_cap, n_ll));
        for (int r : who) key[r] = -2;
        batched += (int)who.size();
        n_groups++;
    }
    for (int r = 0; r < n_active; ++r) {         // the rest: the classic loop, one member after the other
        if (key[r] == -2) continue;
        plsa_ctx *c = b->ctx[r].get();
        ScratchLoan loan(L, c);
        struct ArithmeticLoan {                  // plsa_set_arithmetic of the leader applies to its members
            plsa_ctx *c; bool s, l;
            ArithmeticLoan(plsa_ctx *c_, plsa_ctx *L_) : c(c_), s(c_->ref_sums), l(c_->ref_ll) { c->ref_sums = L_->ref_sums; c->ref_ll = L_->ref_ll; }
            ~ArithmeticLoan() { c->ref_sums = s; c->ref_ll = l; }
        } arithmetic(c, L);
        CHK(member_rc(L, c, plsa_fit(c, nullptr, n_iter, n_iter_per_test, tolerance, thresh, flags, iters_done + r,
                                     ll_trace ? ll_trace + (size_t)r * ll_cap : nullptr, n_ll + r)));
        b->last_ll[r] = c->h_ll[0];
    }
    if (n_batched) *n_batched = batched;
    return 0;
}

int plsa_members_capacity(plsa_ctx *ctx, int32_t k, int32_t *max_members) {
    if (!ctx || !max_members) return fail(ctx, "plsa_members_capacity: NULL argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->bn <= 0) return fail(ctx, "plsa_members_capacity: no corpus uploaded");
    if (k <= 0 || k > 1024) return fail(ctx, "plsa_members_capacity: k=%d outside [1,1024]", k);
    size_t free_b = 0, total_b = 0;
    HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
    // a member's footprint, from above: resample + row ids + CSC copy + both packed streams (36 bytes per entry, a resample
    // may hold somewhat more entries than the corpus: 25 % head-room), item partials of both passes at the shortest item
    // length (16 entries), two sets of factors + the accumulator, and the buffers' own growth margin
    const double nnz = 1.25 * (double)ctx->bnnz, n = (double)ctx->bn, m = (double)ctx->bm, kp = (k + 3) / 4 * 4;
    const double per = 1.07 * (36.0 * nnz + 4.0 * kp * ((nnz / 16 + m) + (nnz / 16 + n) + 2 * n + 3 * m) + 64.0 * (n + m)) + (1 << 20);
    const double fit = 0.5 * (double)free_b / per;                // half of what is free: the stack and the leader's scratch need room too
    *max_members = (int32_t)std::max(0.0, std::min((double)PLSA_MEMBERS_MAX, fit));
    return 0;
}

int plsa_members_copy_components(plsa_members *b, int32_t member, void *dst) {
    CHK(members_check(b, member));
    if (!dst) return fail(b->leader, "plsa_members_copy_components: dst is NULL");
    plsa_ctx *c = b->ctx[member].get();
    return member_rc(b->leader, c, plsa_copy_components_to_device(c, dst));
}

int plsa_members_context(plsa_members *b, int32_t member, plsa_ctx **out) {
    CHK(members_check(b, member));
    if (!out) return fail(b->leader, "plsa_members_context: out is NULL");
    *out = b->ctx[member].get();
    return 0;
}

int plsa_members_last_ll(plsa_members *b, int32_t member, double *ll) {
    CHK(members_check(b, member));
    if (!ll) return fail(b->leader, "plsa_members_last_ll: ll is NULL");
    *ll = b->last_ll[member];
    return 0;
}

int plsa_members_info(plsa_members *b, int32_t member, int32_t *info) {
    CHK(members_check(b, member));
    if (!info) return fail(b->leader, "plsa_members_info: info is NULL");
    const plsa_members::Info &i = b->info[member];
    const int v[8] = {i.group, i.group_size, i.items, i.rseg, i.n_chunks, i.n_heavy, i.row_grid, i.norm_blocks};
    for (int j = 0; j < 8; ++j) info[j] = v[j];
    return 0;
}

}  // extern "C"
