// plsa_ref.hpp -- the host side of the reference arithmetic (kernels: plsa_ref_kernels.hpp): the reference's statements with the
// reference's roundings.  Part of plsa_hip.hip's translation unit, included after ensure_p: it uses the context, the structure
// builders and the launch helpers defined above it, and the E-step, M-step and likelihood wrappers below it call into it.
// Every count, size and threshold comes from plsa_ref_plan.hpp, which is checked on a CPU; every PLSA_REF_* knob is read by
// ref_knobs.
#pragma once

#include "plsa_ref_plan.hpp"

namespace {

namespace ref_plan = plsa::ref::plan;

// a block of documents of the budgeted reference arithmetic: entries [e0, e0 + nnz) of the COO order, documents [d0, d1)
struct RefSpan {
    i64 e0, nnz; int d0, d1;
    i64 cap;           // non-zeros of the plan's largest block: scratch is sized once for all blocks
    bool first, last;
};

// The knobs of the reference arithmetic, and the moment each is read (tests set the per-call ones around a shared engine):
//   name                 default  read                          effect
//   PLSA_REF_CHAIN       auto     when a context is created     norm_pwz and the sequential likelihood: auto | pairs | serial
//                                 (REF_AT_CREATE; kept in         (chain_mode 0 | 1 | 2; auto: pairs from 4096 non-zeros, until a
//                                 c->ref_chain_mode)              walk had more than a quarter of its chunks on the slow way)
//   PLSA_REF_E_TILED     1        once per process, by the      0: the E-step one thread per non-zero (k_ref_e_step) instead of
//                                 first E-step (REF_AT_E_STEP)    tiles through LDS (k_ref_e_step_tiled)
//   PLSA_REF_FUSE_SUMS   1        every E-step                  0: no tile sums from the E-step, k_ref_pair_sums reads P itself
//   PLSA_REF_HEAVY_MIN   2048     when the list of long         entries from which a column gets a workgroup of its own
//                                 columns is built                (k_ref_col_heavy); 0: none
//   PLSA_REF_LEVELS      2        every pair chain              1: the walk steps through chunks only, no groups of PAIR_R
//   PLSA_REF_CHUNK       unset    every pair chain              addends per chunk: a multiple of 64 in 64..4096, else ignored
//   PLSA_REF_ROW_TILED   unset    every document pass           1 / 0: the tiled document pass always / never (unset: from
//                                                                 300 000 documents on)
enum RefKnobsAt { REF_AT_CREATE, REF_AT_E_STEP, REF_AT_CALL };
struct RefKnobs {
    bool e_tiled, fuse_sums, two_levels;                   // e_tiled: REF_AT_E_STEP only
    int chain_mode, heavy_min, chunk, row_tiled;           // chunk: 0 unset; row_tiled: -1 unset
};
RefKnobs ref_knobs(const plsa_ctx *c, RefKnobsAt at = REF_AT_CALL) {
    auto num = [](const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; };
    RefKnobs k{};
    const char *mode = at == REF_AT_CREATE ? getenv("PLSA_REF_CHAIN") : nullptr;
    k.chain_mode = !mode ? c->ref_chain_mode : (!strcmp(mode, "pairs") ? 1 : (!strcmp(mode, "serial") ? 2 : 0));
    if (at == REF_AT_CREATE) return k;
    if (at == REF_AT_E_STEP) { static const bool tiled = num("PLSA_REF_E_TILED", 1) != 0; k.e_tiled = tiled; }
    k.fuse_sums = num("PLSA_REF_FUSE_SUMS", 1) != 0;
    k.heavy_min = num("PLSA_REF_HEAVY_MIN", 2048);
    k.two_levels = num("PLSA_REF_LEVELS", 2) != 1;
    k.chunk = num("PLSA_REF_CHUNK", 0);
    const int tiled_rows = num("PLSA_REF_ROW_TILED", INT32_MIN);
    k.row_tiled = tiled_rows == INT32_MIN ? -1 : (tiled_rows != 0 ? 1 : 0);
    return k;
}

// fn(integral_constant<int, V>) for the V among Vs that equals v; false: none does
template <int... Vs, class Fn> bool with_int(int v, Fn &&fn) { return ((v == Vs && (fn(std::integral_constant<int, Vs>{}), true)) || ...); }

// topics per lane (NZ) of the reference-arithmetic kernels: fn(integral_constant<int, NZ>)
template <class Fn> int with_nz(plsa_ctx *c, int kp, Fn &&fn) {
    return with_int<1, 2, 4, 8, 16>(ref_plan::topics_per_lane(kp), fn) ? 0 : fail(c, "unsupported topic count k=%d (max 1024)", c->k);
}

// lanes per document / column (G) and topics per lane (NZ) of the passes: z = lane + G t; below 64 lanes a lane holds one topic
template <class Fn> int dispatch_ref_group(plsa_ctx *c, Fn &&fn) {
    if (with_int<8, 16, 32>(ref_plan::group_lanes(c->kp), [&](auto G) { fn(G, std::integral_constant<int, 1>{}); })) return 0;
    return with_nz(c, c->kp, [&](auto NZ) { fn(std::integral_constant<int, 64>{}, NZ); });
}

// does this context evaluate its long chains from parity pairs right now?
bool ref_pairs_now(const plsa_ctx *c) { return ref_plan::pairs_now(c->ref_chain_mode, c->ref_pairs_off, c->nnz); }

// plsa.py:91-105 with one float32 norm per entry, topics in order (P allocated by run_e_step); span: the entries of one block of
// documents into the block's P (allocated by run_ref_em_blocked)
int run_ref_e_step(plsa_ctx *c, float thresh, const RefSpan *span = nullptr) {
    CHK(ensure_rowidx(c));
    const RefKnobs knobs = ref_knobs(c, REF_AT_E_STEP);
    const i64 e0 = span ? span->e0 : 0, nnz = span ? span->nnz : c->nnz;
    const int *ri = c->rowidx.ids.as<int>() + e0, *ci = c->col + e0;
    const float *xv = c->val + e0;
    if (knobs.e_tiled && nnz > 0) {
        Scope s(c, "k_ref_e_step");
        const int kp = c->kp;
        // with tile sums for the chain's k_ref_pair_sums, where the chain will run from pairs
        const bool fuse = knobs.fuse_sums && ref_pairs_now(c) && !c->ref_e_no_sums;
        int rc_alloc = 0;
        CHK(with_nz(c, kp, [&](auto NZ) {
            constexpr int nz = decltype(NZ)::value;
            const i64 tiles = ref_plan::e_step_tiles(nnz, nz);
            const i64 cap_tiles = span ? ref_plan::e_step_tiles(span->cap, nz) : tiles;    // (blocks: sized once, for the largest)
            if (fuse && (rc_alloc = ensure(c, c->ref_tsum.sums, sizeof(float) * (size_t)cap_tiles * kp)) != 0) return;
            with_flag(fuse, [&](auto FUSE) {
                constexpr bool f = decltype(FUSE)::value;
                hipLaunchKernelGGL((plsa::ref::k_ref_e_step_tiled<nz, f>), dim3(grid_for(c, tiles, 2)), dim3(128),
                                   (size_t)ref_plan::tile_lds_bytes(kp, nz), c->stream, ri, ci, nnz, c->U[c->cu].as<float>(),
                                   c->Vt[c->cv].as<float>(), p_base(c), kp, thresh, f ? xv : nullptr, f ? c->ref_e_sw : nullptr,
                                   f ? c->ref_tsum.sums.as<float>() : nullptr);
            });
            if (fuse) { c->ref_tsum.valid = true; c->ref_tsum.sw = c->ref_e_sw; c->ref_tsum.tj = 64 / nz; }
        }));
        if (rc_alloc) return rc_alloc;
    } else {
        Scope s(c, "k_ref_e_step");
        hipLaunchKernelGGL(plsa::ref::k_ref_e_step, dim3(grid_for(c, nnz, 256)), dim3(256), 0, c->stream, ri, ci, nnz,
                           c->U[c->cu].as<float>(), c->Vt[c->cv].as<float>(), p_base(c), c->kp, thresh);
    }
    CHK(launch_check(c, "k_ref_e_step"));
    c->p_state.valid = true;
    return 0;
}

// the reference arithmetic's long columns (heavy_min entries or more; 0: none): list [count, columns...]
int ensure_ref_heavy(plsa_ctx *c) {
    if (c->ref_heavy.valid) return 0;
    c->ref_heavy.min = ref_knobs(c).heavy_min;
    c->ref_heavy.n = 0;
    if (c->ref_heavy.min > 0 && c->nnz > 0) {
        CHK(ensure(c, c->ref_heavy.cols, sizeof(int) * (size_t)(c->m + 1)));
        HIPCHK(c, hipMemsetAsync(c->ref_heavy.cols.p, 0, sizeof(int), c->stream));
        hipLaunchKernelGGL(plsa::ref::k_ref_heavy_cols, dim3((unsigned)((c->m + 255) / 256)), dim3(256), 0, c->stream,
                           c->csc.colptr.as<int>(), (int)c->m, c->ref_heavy.min, c->ref_heavy.cols.as<int>() + 1, c->ref_heavy.cols.as<int>());
        CHK(launch_check(c, "k_ref_heavy_cols"));
        int n = 0;
        HIPCHK(c, hipMemcpyAsync(&n, c->ref_heavy.cols.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->ref_heavy.n = n;
    }
    c->ref_heavy.valid = true;
    return 0;
}

// The one launch of k_ref_norm_chain (unchecked): norm_pwz's serial chain (GATHER false: one workgroup over the entries) or the
// long columns (GATHER true: one workgroup per listed column); carry: a block after the first starts from what `out` holds
struct RefChainLaunch {
    int grid; hipStream_t stream;
    const int *rowidx; const float *vals; i64 nnz; float *out;             // the entries and where the sums go
    const int *pos, *heavy, *colptr; i64 e0, e1; int first;                // GATHER / a block of documents
};
template <class Gather> int launch_ref_norm_chain(plsa_ctx *c, Gather, bool carry, const float *d_sw, const RefChainLaunch &a) {
    return with_nz(c, c->kp, [&](auto NZ) {
        with_flag(d_sw != nullptr, [&](auto SW) {
            with_flag(carry, [&](auto CARRY) {
                hipLaunchKernelGGL((plsa::ref::k_ref_norm_chain<decltype(NZ)::value, decltype(SW)::value, Gather::value, decltype(CARRY)::value>),
                                   dim3(a.grid), dim3(plsa::ref::CHAIN_THREADS), 0, a.stream, a.rowidx, a.vals, a.nnz, p_base(c), d_sw,
                                   c->kp, a.out, a.pos, a.heavy, a.colptr, a.e0, a.e1, a.first);
            });
        });
    });
}

// One chain of float32 additions over the non-zeros in order, per "topic" z < kp, WITHOUT the chain (plsa_ref_kernels.hpp: chunk
// sums -> prefix -> (parity -> increment) pairs -> one checking walk per 64 topics), on c->ls.  kind / P / kp: PAIR_PLAIN or
// PAIR_WEIGHTED over P(z|w,d) (norm_pwz, plsa.py:193), PAIR_NEG_TERMS over the likelihood terms with kp = 1 (plsa.py:322).
// span: the entries of one block of documents, P the block's rows; a block after the first starts its chains from `out`.
// Two levels (default): chunks of 256 addends, walked in groups of PAIR_R; one: chunks only, longer on large corpora.
int run_ref_pair_chain(plsa_ctx *c, int kind, const float *P, int kp, const float *d_sw, float *out, unsigned long long *stats,
                       const RefSpan *span = nullptr) {
    const i64 e0 = span ? span->e0 : 0, nnz = span ? span->nnz : c->nnz;
    const bool carry = span && !span->first;
    const int *ri = c->rowidx.ids.as<int>() + e0;
    const float *xv = c->val + e0;
    const bool ll = kind == plsa::ref::PAIR_NEG_TERMS;              // (timing names: the likelihood's launches apart from norm_pwz's)
    const RefKnobs knobs = ref_knobs(c);
    const bool two = knobs.two_levels;
    const ref_plan::PairChain pc = ref_plan::pair_chain(nnz, span ? span->cap : c->nnz, c->nnz, kp, two, knobs.chunk);
    if (two) {
        CHK(ensure(c, c->ref_pairs2, (size_t)pc.pairs2_bytes));
        CHK(ensure(c, c->ref_exps2, (size_t)pc.exps2_bytes));
    }
    CHK(ensure(c, c->ref_csum, (size_t)pc.csum_bytes));
    CHK(ensure(c, c->ref_pairs, (size_t)pc.pairs_bytes));
    CHK(ensure(c, c->ref_exps, (size_t)pc.exps_bytes));
    const int L = pc.L;
    const i64 n_chunks = pc.span.n_chunks, n_groups = pc.span.n_groups, n_pad = pc.span.n_pad;
    const int grid = grid_for(c, pc.span.n_super, 4);
    double *csum = c->ref_csum.as<double>();
    uint4 *prs = c->ref_pairs.as<uint4>(), *prs2 = c->ref_pairs2.as<uint4>();
    unsigned *exps = c->ref_exps.as<unsigned>(), *exps2 = c->ref_exps2.as<unsigned>();
    CHK(with_nz(c, kp, [&](auto NZ) {
        constexpr int nz = decltype(NZ)::value;
        auto go = [&](auto KIND) {
            constexpr int kd = decltype(KIND)::value;
            if (!ll && c->ref_tsum.valid && c->ref_tsum.sw == d_sw && P == p_base(c) && c->p_state.valid && L % c->ref_tsum.tj == 0) {
                // the E-step that wrote this P left the sums of its tiles: no second pass over P
                Scope s(c, "k_ref_pair_sums");
                const i64 n_tiles = (nnz + c->ref_tsum.tj - 1) / c->ref_tsum.tj;
                hipLaunchKernelGGL(plsa::ref::k_ref_pair_sums_from_tiles, dim3(grid_for(c, n_chunks * kp, 256)), dim3(256), 0, c->ls,
                                   c->ref_tsum.sums.as<float>(), kp, L / c->ref_tsum.tj, n_tiles, n_chunks, n_pad, csum);
            } else {
                Scope s(c, ll ? "k_ref_ll_pair_sums" : "k_ref_pair_sums");
                hipLaunchKernelGGL((plsa::ref::k_ref_pair_sums<nz, kd>), dim3(grid), dim3(256), 0, c->ls, ri, xv, nnz, P,
                                   d_sw, kp, L, n_chunks, n_pad, csum);
            }
            {
                Scope s(c, ll ? "k_ref_ll_pair_prefix" : "k_ref_pair_prefix");
                with_flag(carry, [&](auto CARRY) {
                    hipLaunchKernelGGL(plsa::ref::k_ref_pair_prefix<decltype(CARRY)::value>, dim3(kp), dim3(256), 0, c->ls, csum,
                                       n_chunks, n_pad, carry ? out : nullptr);
                });
            }
            {
                Scope s(c, ll ? "k_ref_ll_pair_build" : "k_ref_pair_build");
                hipLaunchKernelGGL((plsa::ref::k_ref_pair_build<nz, kd>), dim3(grid), dim3(256), 0, c->ls, ri, xv, nnz, P,
                                   d_sw, kp, L, n_chunks, n_pad, csum, prs, exps);
            }
            if (two) {
                Scope s(c, ll ? "k_ref_ll_pair_compose" : "k_ref_pair_compose");
                hipLaunchKernelGGL(plsa::ref::k_ref_pair_compose, dim3(grid_for(c, n_groups * kp, 256)), dim3(256), 0, c->ls, prs, exps,
                                   kp, n_chunks, n_groups, prs2, exps2);
            }
            // the walk steps through the groups' records (two levels) or the chunks' own
            Scope s(c, ll ? "k_ref_ll_pair_walk" : "k_ref_pair_walk");
            with_flag(two, [&](auto TWO) {
                with_flag(carry, [&](auto CARRY) {
                    constexpr bool tw = decltype(TWO)::value;
                    hipLaunchKernelGGL((plsa::ref::k_ref_pair_walk<kd, tw, decltype(CARRY)::value>), dim3((kp + 63) / 64),
                                       dim3(plsa::ref::WALK_THREADS), 0, c->ls, ri, xv, nnz, P, d_sw, kp, L, tw ? n_groups : n_chunks,
                                       tw ? prs2 : prs, tw ? exps2 : exps, out, stats, n_chunks, prs, exps);
                });
            });
        };
        with_int<plsa::ref::PAIR_PLAIN, plsa::ref::PAIR_WEIGHTED>(kind, go);
        if constexpr (nz == 1) with_int<plsa::ref::PAIR_NEG_TERMS>(kind, go);        // (the likelihood's chain: kp = 1)
    }));
    return launch_check(c, "k_ref_pair_walk");
}

// norm_pwz[z] = the reference's ONE float32 running sum over all non-zeros (plsa.py:193) on c->ls: from per-chunk parity pairs and a
// walk (k_ref_pair_*), or by the serial chain (k_ref_norm_chain); same bits either way.
// span: the chain over one block's entries, started (after the first block) from what norm_pwz holds; the walk's counts add up
// over the blocks and are read back after the last.
int run_ref_norm_pwz(plsa_ctx *c, const float *d_sw, const RefSpan *span = nullptr) {
    const int kp = c->kp;
    const i64 e0 = span ? span->e0 : 0, nnz = span ? span->nnz : c->nnz;
    const bool carry = span && !span->first, last = !span || span->last;
    float *out = c->norm_pwz.as<float>();
    if (c->nnz <= 0) { HIPCHK(c, hipMemsetAsync(out, 0, sizeof(float) * (size_t)kp, c->ls)); return 0; }
    // the last walk's count of slow chunks, if it has arrived (never waited for)
    if (c->ref_stats_pending && hipEventQuery(c->ev_ref_stats) == hipSuccess) {
        c->ref_stats_pending = false;
        const unsigned long long slow = c->h_ref_stats[0], chunks = c->h_ref_stats[1];
        c->ref_slow_total += slow; c->ref_chunks_total += chunks;
        if (c->ref_chain_mode == 0 && ref_plan::walk_too_slow(slow, chunks)) c->ref_pairs_off = true;
    }
    if (!ref_pairs_now(c)) {
        Scope s(c, "k_ref_norm_chain");
        CHK(launch_ref_norm_chain(c, std::false_type{}, carry, d_sw,
                                  {1, c->ls, c->rowidx.ids.as<int>() + e0, c->val + e0, nnz, out, nullptr, nullptr, nullptr, 0, 0, 0}));
        return launch_check(c, "k_ref_norm_chain");
    }
    CHK(ensure(c, c->ref_stats, 32));
    if (!c->h_ref_stats) {
        HIPCHK(c, host_alloc(c->h_ref_stats, 2));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_ref_stats.h, hipEventDisableTiming));
    }
    unsigned long long *stats = c->ref_stats.as<unsigned long long>();
    if (!carry) HIPCHK(c, hipMemsetAsync(stats, 0, 16, c->ls));
    CHK(run_ref_pair_chain(c, d_sw ? plsa::ref::PAIR_WEIGHTED : plsa::ref::PAIR_PLAIN, p_base(c), kp, d_sw, out, stats, span));
    if (last && !c->ref_stats_pending) {       // (one read-back in flight at a time; a walk whose count is skipped is simply not counted)
        HIPCHK(c, hipMemcpyAsync(c->h_ref_stats.get(), stats, 16, hipMemcpyDeviceToHost, c->ls));
        HIPCHK(c, hipEventRecord(c->ev_ref_stats, c->ls));
        c->ref_stats_pending = true;
    }
    return 0;
}

// The norm_pwz chain (one workgroup, nnz dependent additions per topic, or the pair chain) on the second stream, beside what the
// caller enqueues on the first after this: forked from c->stream here, ev_join recorded behind it
int fork_ref_norm_pwz(plsa_ctx *c, const float *d_sw, const RefSpan *span = nullptr) {
    HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
    LaunchOn on2(c, c->stream2);
    CHK(run_ref_norm_pwz(c, d_sw, span));
    HIPCHK(c, hipEventRecord(c->ev_join, c->stream2));
    return 0;
}

// The document pass, the column pass and the long columns of the reference M-step on c->stream, from the P(z|w,d) of all
// non-zeros or (span) of one block of documents: that block's documents, and every column's entries inside the block with the
// accumulators carried in Vacc from block to block.
// (order: the length-sorted document order of the whole corpus; a block walks its documents in their own order)
int run_ref_passes(plsa_ctx *c, const float *d_sw, bool update_v, float *d_norm_pdz, int heavy_min, const int *order,
                   const RefSpan *span = nullptr) {
    const int d0 = span ? span->d0 : 0, nd = span ? span->d1 - span->d0 : (int)c->n, first = !span || span->first;
    const i64 e0 = span ? span->e0 : 0, e1 = span ? span->e0 + span->nnz : 0;
    const bool row_tiled = ref_plan::row_tiled(c->n, ref_knobs(c).row_tiled);
    CHK(dispatch_ref_group(c, [&](auto G, auto NZ) {
        constexpr int g = decltype(G)::value, nz = decltype(NZ)::value;
        with_flag(span != nullptr, [&](auto BLK) {
            constexpr bool blk = decltype(BLK)::value;
            {
                Scope s(c, "k_ref_row_pass");
                if (row_tiled) {
                    hipLaunchKernelGGL((plsa::ref::k_ref_row_pass_tiled<nz, blk>), dim3(grid_for(c, ref_plan::e_step_tiles(nd, nz), 2)), dim3(128),
                                       (size_t)ref_plan::tile_lds_bytes(c->kp, nz), c->stream, c->indptr, c->val, nd, order,
                                       p_base(c), c->U[out_u(c)].as<float>(), d_norm_pdz, c->kp, d0, e0);
                } else {
                    hipLaunchKernelGGL((plsa::ref::k_ref_row_pass<g, nz, blk>), dim3(grid_for(c, nd, 256 / g)), dim3(256),
                                       sizeof(float) * (size_t)(256 / g) * c->kp, c->stream, c->indptr, c->val, nd, order,
                                       p_base(c), c->U[out_u(c)].as<float>(), d_norm_pdz, c->kp, d0, e0);
                }
            }
            if (update_v) {
                Scope s(c, "k_ref_col_pass");
                hipLaunchKernelGGL((plsa::ref::k_ref_col_pass<g, nz, blk>), dim3(grid_for(c, c->m, 256 / g)), dim3(256), 0, c->stream,
                                   c->csc.colptr.as<int>(), c->csc.row.as<int>(), c->csc.val.as<float>(), c->csc.pos.as<int>(),
                                   (int)c->m, p_base(c), d_sw, c->Vacc.as<float>(), c->kp, heavy_min, e0, e1, first);
            }
        });
    }));
    if (update_v && c->ref_heavy.n > 0) {
        // the long columns: one workgroup each, the norm_pwz chain's kernel over the column's entries (6.4 ns per entry where a
        // group's own walk costs ~160: the Zipf head was the pass -- 24.6 ms at the config-3 150 k sample, 157 ms at the whole)
        Scope s(c, "k_ref_col_heavy");
        CHK(launch_ref_norm_chain(c, std::true_type{}, span != nullptr, d_sw,
                                  {c->ref_heavy.n, c->stream, c->csc.row.as<int>(), c->csc.val.as<float>(), 0, c->Vacc.as<float>(),
                                   c->csc.pos.as<int>(), c->ref_heavy.cols.as<int>() + 1, c->csc.colptr.as<int>(), e0, e1, first}));
    }
    return launch_check(c, "k_ref_row_pass / k_ref_col_pass");
}

// what the vocabulary half needs before its first launch; *heavy_min: the length from which a column goes to a workgroup of its own
int prepare_ref_v(plsa_ctx *c, int *heavy_min) {
    CHK(ensure_csc(c));
    CHK(ensure_rowidx(c));
    CHK(ensure_ref_heavy(c));
    if (c->ref_heavy.n > 0) *heavy_min = c->ref_heavy.min;
    return ensure(c, c->norm_pwz, sizeof(float) * (size_t)c->kp);
}

// after the passes and the chain (ev_join): P(w|z) = Vacc / norm_pwz where positive (plsa.py:196-199)
int run_ref_v_normalise(plsa_ctx *c) {
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    Scope s(c, "k_v_normalise");
    const i64 total4 = c->m * c->kp / 4;
    hipLaunchKernelGGL(plsa::k_v_normalise, dim3(grid_for(c, total4, 256)), dim3(256), c->kp * sizeof(float), c->stream,
                       c->Vacc.as<float>(), c->Vt[out_v(c)].as<float>(), (int)c->m, c->kp, c->norm_pwz.as<float>());
    return launch_check(c, "k_v_normalise");
}

// plsa.py:172-204 / 277-310 / 795-816 from the materialised P: U[out], (update_v) Vt[out]; swaps the buffers in.
// The norm_pwz chain runs on the second stream beside the document and column passes.
int run_ref_m_step(plsa_ctx *c, const float *d_sw, bool update_v, float *d_norm_pdz) {
    if (c->sharded) return fail(c, "the reference arithmetic has no doc-sharded form (norm_pwz is ONE chain over all non-zeros)");
    const int *order = nullptr;
    CHK(ensure_roworder(c, &order));               // (here: the sort is enqueued before the fork to the second stream)
    int heavy_min = INT32_MAX;
    if (update_v) {
        CHK(prepare_ref_v(c, &heavy_min));
        CHK(fork_ref_norm_pwz(c, d_sw));
    }
    CHK(run_ref_passes(c, d_sw, update_v, d_norm_pdz, heavy_min, order));
    if (update_v) CHK(run_ref_v_normalise(c));
    c->cu ^= 1;
    if (update_v) c->cv ^= 1;
    return 0;
}

// The block plan of plsa_set_p_budget for the active matrix (plsa_ref_plan.hpp: block_plan)
int ensure_ref_blocks(plsa_ctx *c) {
    plsa_ctx::RefBlocks &pl = c->ref_blocks;
    if (pl.valid && pl.budget == c->p_budget && pl.kp == c->kp) return 0;
    pl.valid = false;                              // (a rebuild that fails leaves no plan behind)
    const i64 max_rows = ref_plan::block_max_rows(c->kp, c->p_budget);
    std::vector<int> ip;
    if (max_rows >= 1 && c->nnz > max_rows) {      // more than one block: the cut needs the documents' lengths
        ip.resize((size_t)c->n + 1);
        HIPCHK(c, hipMemcpyAsync(ip.data(), c->indptr, sizeof(int) * ip.size(), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    ref_plan::BlockPlan bp = ref_plan::block_plan(ip.data(), c->n, c->nnz, c->kp, c->p_budget);
    const int64_t row_bytes = (int64_t)sizeof(float) * c->kp;
    if (bp.status == ref_plan::BlockPlan::NO_ROW)
        return fail(c, "plsa_set_p_budget: a budget of %lld bytes holds no row of P(z|w,d): the least usable budget at k = %d is "
                       "%lld bytes ((1 + 64) * %d * 4)", (long long)c->p_budget, c->k, (long long)(65 * row_bytes), c->kp);
    if (bp.status == ref_plan::BlockPlan::DOC_TOO_LONG)
        return fail(c, "plsa_set_p_budget: document %lld has %lld non-zeros, its P(z|w,d) rows alone need %lld bytes "
                       "((non-zeros + 64) * %d * 4) and the budget is %lld bytes", (long long)bp.bad_doc, (long long)bp.bad_len,
                    (long long)((bp.bad_len + 64) * row_bytes), c->kp, (long long)c->p_budget);
    pl.doc = std::move(bp.doc); pl.ent = std::move(bp.ent);
    pl.budget = c->p_budget; pl.kp = c->kp; pl.largest = bp.largest; pl.valid = true;
    return 0;
}

// One EM iteration of the reference arithmetic with P(z|w,d) of ONE BLOCK of documents at a time (plsa_set_p_budget): per block
// the E-step of its entries, its documents' half of the M-step (complete inside the block), and its part of every column's chain
// and of the norm_pwz chain, each started from what the block before left (Vacc, norm_pwz) -- the additions of run_ref_m_step in
// the same order.  Streams: the norm_pwz chain of block b runs on the second stream beside the passes of block b, as in the
// unblocked step; the E-step of block b + 1 overwrites the buffer, so it waits for that chain (ev_join) and, in stream order, for
// the passes; chain b + 1 follows chain b in the second stream's own order.
int run_ref_em_blocked(plsa_ctx *c, float thresh, const float *d_sw, bool update_v) {
    if (c->sharded) return fail(c, "the reference arithmetic has no doc-sharded form (norm_pwz is ONE chain over all non-zeros)");
    const plsa_ctx::RefBlocks &pl = c->ref_blocks;
    c->ref_tsum.invalidate(); c->p_state.invalidate();
    CHK(ensure_p(c, pl.largest));
    CHK(ensure_rowidx(c));
    int heavy_min = INT32_MAX;
    if (update_v) CHK(prepare_ref_v(c, &heavy_min));
    // (whatever way the loop is left: P holds one block, not the responsibilities of the matrix)
    struct Forget { plsa_ctx *c; ~Forget() { c->ref_tsum.invalidate(); c->p_state.invalidate(); } } forget{c};
    const int nb = pl.blocks();
    for (int b = 0; b < nb; ++b) {
        const RefSpan span{pl.ent[b], pl.ent[b + 1] - pl.ent[b], (int)pl.doc[b], (int)pl.doc[b + 1], pl.largest, b == 0, b == nb - 1};
        if (update_v && b > 0) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));     // the chain of block b - 1 has read P
        c->ref_tsum.invalidate();
        CHK(run_ref_e_step(c, thresh, &span));
        if (update_v) CHK(fork_ref_norm_pwz(c, d_sw, &span));
        CHK(run_ref_passes(c, d_sw, update_v, nullptr, heavy_min, nullptr, &span));
    }
    if (update_v) CHK(run_ref_v_normalise(c));
    c->cu ^= 1;
    if (update_v) c->cv ^= 1;
    return 0;
}

// plsa.py:372-386 as ONE float32 running sum over the non-zeros (PLSA_REFERENCE_LL)
int run_ref_loglik(plsa_ctx *c, const float *d_sw, double *out) {
    if (c->sharded) return fail(c, "the reference arithmetic has no doc-sharded form");
    CHK(ensure_rowidx(c));
    CHK(ensure(c, c->ref_terms, sizeof(float) * (size_t)std::max<i64>(c->nnz, 1)));
    CHK(ensure(c, c->ll_out, sizeof(double)));
    {
        Scope s(c, "k_ref_ll_terms");
        hipLaunchKernelGGL(plsa::ref::k_ref_ll_terms, dim3(grid_for(c, c->nnz, 256)), dim3(256), 0, c->stream,
                           c->rowidx.ids.as<int>(), c->col, c->val, c->nnz, c->U[c->cu].as<float>(), c->Vt[c->cv].as<float>(),
                           d_sw, c->kp, c->ref_terms.as<float>());
    }
    if (ref_pairs_now(c)) {
        // the chain of the NEGATED terms from parity pairs (one "topic"); its slow-chunk counts go to their own slots, unread
        CHK(ensure(c, c->ref_stats, 32));
        CHK(ensure(c, c->ref_ll_neg, sizeof(float)));
        unsigned long long *stats = c->ref_stats.as<unsigned long long>();
        CHK(run_ref_pair_chain(c, plsa::ref::PAIR_NEG_TERMS, c->ref_terms.as<float>(), 1, nullptr, c->ref_ll_neg.as<float>(), stats + 2));
        hipLaunchKernelGGL(plsa::ref::k_ref_ll_from_walk, dim3(1), dim3(1), 0, c->stream, c->ref_ll_neg.as<float>(), c->ll_out.as<double>());
    } else {
        Scope s(c, "k_ref_ll_chain");
        hipLaunchKernelGGL(plsa::ref::k_ref_ll_chain, dim3(1), dim3(64), 0, c->stream, c->ref_terms.as<float>(), c->nnz,
                           c->ll_out.as<double>());
    }
    CHK(launch_check(c, "k_ref_ll_chain"));
    HIPCHK(c, hipMemcpyAsync(c->h_ll.get(), c->ll_out.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out = c->h_ll[0];
    return 0;
}

}  // namespace
