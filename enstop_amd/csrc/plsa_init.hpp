// plsa_init.hpp -- how factors get onto a context and off it again: host factors (plsa_set_factors), the counter-based device
// initialisation (plsa_init_factors_device), the reference's own MT19937 stream evaluated on the device (mt_init behind
// plsa_init_factors_mt19937 / plsa_refit_init_mt19937) and the read-back (plsa_get_factors, plsa_copy_components_to_device).
// Part of plsa_hip.hip's translation unit, included among its entry points (inside their extern "C" block), before
// plsa_members.hpp, whose members run mt_init / plsa_set_factors.  Every way in goes through alloc_factors.  The arithmetic of
// mt_init is plsa_init_plan.hpp's, which is checked on a CPU; the kernels are plsa_init_kernels.hpp's.
#pragma once

extern "C++" {
namespace {

namespace iplan = plsa::init::plan;

static_assert(plsa::init::SEQ_L == plsa::MT_SEQ_L, "the scratch plan and the marginal kernels disagree on the chunk length");

// Factor buffers of the active matrix for k topics: the lane shape set, U[0..1], Vt[0..1] and the accumulator sized, P(z|w,d)
// history, P(z|d) current in buffer 0 -- and P(w|z) too, unless the resident topics stay (plsa_set_factors without V).
int alloc_factors(plsa_ctx *c, int k, bool keep_topics = false) {
    set_shape(c, k);
    const size_t kp = (size_t)c->kp;
    c->fac_n = c->n; c->fac_m = c->m;
    for (int i = 0; i < 2; ++i) CHK(ensure(c, c->U[i], sizeof(float) * (size_t)c->n * kp));
    for (int i = 0; i < 2; ++i) CHK(ensure(c, c->Vt[i], sizeof(float) * (size_t)c->m * kp));
    CHK(ensure(c, c->Vacc, sizeof(float) * (size_t)c->m * kp));
    c->p_state.invalidate();
    c->cu = 0;
    if (!keep_topics) c->cv = 0;
    return 0;
}

// src: V [k, m] in the reference layout, on the device -> dst: Vt [m, kp]
int launch_v_to_vt(plsa_ctx *c, const float *src, float *dst, int k) {
    const iplan::Grid2 g = iplan::transpose_grid(c->m, c->kp);
    hipLaunchKernelGGL(plsa::k_v_to_vt, dim3(g.x, g.y), dim3(256), 0, c->stream, src, dst, k, (int)c->m, c->kp);
    return launch_check(c, "k_v_to_vt");
}

// the current Vt [m, kp] -> dst: V [k, m] in the reference layout, on the device
int launch_vt_to_v(plsa_ctx *c, float *dst) {
    const iplan::Grid2 g = iplan::transpose_grid(c->m, c->kp);
    hipLaunchKernelGGL(plsa::k_vt_to_v, dim3(g.x, g.y), dim3(256), 0, c->stream, c->Vt[c->cv].as<float>(), dst, c->k, (int)c->m, c->kp);
    return launch_check(c, "k_vt_to_v");
}

}  // namespace
}  // extern "C++"

int plsa_set_factors(plsa_ctx *c, const float *U, const float *V, int64_t n, int64_t m, int32_t k) {
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n <= 0) return fail(c, "plsa_set_factors: upload a corpus first");
    if (n != c->n || m != c->m)
        return fail(c, "plsa_set_factors: factor shapes (n=%lld, m=%lld) do not match the active matrix (%lld x %lld)",
                    (long long)n, (long long)m, (long long)c->n, (long long)c->m);
    if (k <= 0 || k > 1024) return fail(c, "plsa_set_factors: k=%d outside [1,1024]", k);
    if (!U) return fail(c, "plsa_set_factors: U is NULL");
    if (!V && (k != c->k || !c->Vt[0].p)) return fail(c, "plsa_set_factors: V is NULL but no topics with k=%d are resident", k);
    CHK(alloc_factors(c, k, /*keep_topics=*/!V));
    const int kp = c->kp;
    if (kp != k) HIPCHK(c, hipMemsetAsync(c->U[0].p, 0, sizeof(float) * (size_t)n * kp, c->stream));
    if (kp == k)
        CHK(copy_to_device(c, c->U[0].p, U, sizeof(float) * (size_t)n * k));
    else
        HIPCHK(c, hipMemcpy2DAsync(c->U[0].p, sizeof(float) * kp, U, sizeof(float) * k, sizeof(float) * k,
                                   (size_t)n, hipMemcpyHostToDevice, c->stream));
    if (V) {
        CHK(ensure(c, c->tmp0, sizeof(float) * (size_t)k * m));
        HIPCHK(c, hipMemcpyAsync(c->tmp0.p, V, sizeof(float) * (size_t)k * m, hipMemcpyHostToDevice, c->stream));
        CHK(launch_v_to_vt(c, c->tmp0.as<float>(), c->Vt[0].as<float>(), k));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// Throughput-mode initialisation on the device (counter-based RNG; not the reference's stream).
int plsa_init_factors_device(plsa_ctx *c, int32_t k, uint64_t seed) {
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n <= 0) return fail(c, "plsa_init_factors_device: upload a corpus first");
    if (k <= 0 || k > 1024) return fail(c, "plsa_init_factors_device: k=%d outside [1,1024]", k);
    CHK(alloc_factors(c, k));
    const i64 n = c->n, m = c->m;
    const int kp = c->kp;
    // P(w|z): uniform draws per (topic, word), topic rows normalised -> generate [k, m] then transpose
    CHK(ensure(c, c->tmp0, sizeof(float) * (size_t)std::max<i64>(k, 4) * m));
    hipLaunchKernelGGL(plsa::k_init_rows, dim3(grid_for(c, k, 4)), dim3(256), 0, c->stream, c->tmp0.as<float>(),
                       (i64)k, (int)m, (int)m, (unsigned long long)plsa::mix64(seed ^ 0x5157ull));
    CHK(launch_v_to_vt(c, c->tmp0.as<float>(), c->Vt[0].as<float>(), k));
    hipLaunchKernelGGL(plsa::k_init_rows, dim3(grid_for(c, n, 4)), dim3(256), 0, c->stream, c->U[0].as<float>(),
                       n, k, kp, (unsigned long long)plsa::mix64(seed ^ 0xD0C5ull));
    CHK(launch_check(c, "k_init_rows"));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// plsa_init(X, k, init="random", rng) + the float32 casts of plsa_fit (plsa.py:455-456, 510-511,
// 709-710) with the reference's own MT19937 stream, evaluated on the device.  state_io: the 624 key
// words + position of numpy.random.RandomState.get_state(); on return it holds the advanced state.
// V_host == nullptr: plsa_init (topics drawn first, then the document rows).  V_host != nullptr: the
// refit initialisation (plsa.py:979-981) -- only rand(n, k) is drawn, the topics are the given ones.
static int mt_init(plsa_ctx *c, int32_t k, uint32_t *state_io /*[625]*/, const float *V_host) {
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n <= 0) return fail(c, "plsa_init_factors_mt19937: upload a corpus first");
    if (k <= 0 || k > 1024) return fail(c, "plsa_init_factors_mt19937: k=%d outside [1,1024]", k);
    const i64 n = c->n, m = c->m;
    // plan.  The stream is split into pieces that start 2^b blocks apart (csrc/mt_jump.hpp) once it is long enough to pay for
    // the jumps; the words produced are those of the one sequential stream.
    const iplan::MtStream ms = iplan::mt_stream(n, m, k, !V_host, state_io[624], c->mt_streams, c->mt_min_blocks);
    if (!ms.ok) return fail(c, "plsa_init_factors_mt19937: bad generator position");
    const iplan::MtScratch sc = iplan::mt_scratch(k, m, ms.streams_p2, ms.levels, c->mt_chain);
    const int pos0 = (int)state_io[624];
    std::vector<uint32_t> polys((size_t)ms.levels * 624);
    for (int l = 0; l < ms.levels; ++l)     // level l jumps by step(l) * per_stream blocks
        if (!mtjump::block_jump_polynomial(ms.exponent(l), polys.data() + (size_t)l * 624))
            return fail(c, "plsa_init_factors_mt19937: MT19937 characteristic polynomial not recovered");
    // ensure
    CHK(alloc_factors(c, k));
    const int kp = c->kp;
    DevBuf &words = c->mt_words, &st = c->mt_state, &fin = c->mt_fin, &gp = c->mt_poly;
    CHK(ensure(c, words, (size_t)ms.words_bytes()));
    CHK(ensure(c, st, (size_t)sc.state_bytes));
    CHK(ensure(c, fin, (size_t)sc.fin_bytes));
    if (ms.levels) CHK(ensure(c, gp, (size_t)sc.poly_bytes));
    if (!V_host && !c->mt_chain) CHK(ensure(c, c->mt_seq, (size_t)sc.seq_bytes));
    // launch: the pieces' start states, the words, the topics, the document rows
    HIPCHK(c, hipMemsetAsync(st.p, 0, (size_t)sc.state_bytes, c->stream));
    HIPCHK(c, hipMemcpyAsync(st.p, state_io, sizeof(unsigned) * 624, hipMemcpyHostToDevice, c->stream));
    if (ms.levels) {
        HIPCHK(c, hipMemcpyAsync(gp.p, polys.data(), (size_t)sc.poly_bytes, hipMemcpyHostToDevice, c->stream));
        Scope s(c, "k_mt_jump");
        for (int l = 0; l < ms.levels; ++l)
            hipLaunchKernelGGL(plsa::k_mt_jump, dim3(iplan::jump_grid(ms, l), plsa::MT_JUMP_SLICES), dim3(256), 0, c->stream,
                               gp.as<unsigned>() + (size_t)l * 624, st.as<unsigned>(), ms.step(l), ms.n_streams);
    }
    { Scope s(c, "k_mt19937_fill");
      hipLaunchKernelGGL(plsa::k_mt19937_fill, dim3((unsigned)ms.n_streams), dim3(PLSA_MT_THREADS), 0, c->stream,
                         st.as<unsigned>(), words.as<unsigned>(), pos0, ms.per_stream, ms.n_words, ms.n_streams, fin.as<unsigned>()); }
    float *Vtmp = c->Vt[1].as<float>();     // [m*kp] floats >= k*m: free scratch here
    if (V_host) {
        HIPCHK(c, hipMemcpyAsync(Vtmp, V_host, sizeof(float) * (size_t)k * m, hipMemcpyHostToDevice, c->stream));
    } else {
        // V[k, m] in the reference layout (words are consumed in that order), then the layout transpose
        double *marg = reinterpret_cast<double *>(fin.as<unsigned>() + sc.marg_word);   // k <= 1024 doubles behind the state
        if (c->mt_chain) {       // PLSA_MT_CHAIN=1: the plain chain of m dependent adds per topic (A/B, tests)
            hipLaunchKernelGGL(plsa::k_mt_marginal_v, dim3((unsigned)k), dim3(64), 0, c->stream, words.as<unsigned>(), k, (int)m, marg);
        } else {                 // the same roundings from per-chunk parity pairs (plsa_init_kernels.hpp: k_mt_chunk_pairs)
            char *seq = c->mt_seq.as<char>();
            plsa::u64 *csum = reinterpret_cast<plsa::u64 *>(seq + sc.csum_off), *pairs = reinterpret_cast<plsa::u64 *>(seq + sc.pairs_off);
            double *tsum = reinterpret_cast<double *>(seq + sc.tsum_off);
            int *guess = reinterpret_cast<int *>(seq + sc.guess_off);
            const dim3 tiles(iplan::chunk_grid(sc, k).x, iplan::chunk_grid(sc, k).y);
            hipLaunchKernelGGL(plsa::k_mt_chunk_sums, tiles, dim3(64), 0, c->stream, words.as<unsigned>(), (int)m, sc.nch, csum, tsum);
            hipLaunchKernelGGL(plsa::k_mt_chunk_pairs, tiles, dim3(64), 0, c->stream, words.as<unsigned>(), (int)m, sc.nch,
                               csum, tsum, pairs, guess);
            hipLaunchKernelGGL(plsa::k_mt_marginal_walk, dim3((unsigned)k), dim3(64), 0, c->stream, words.as<unsigned>(),
                               (int)m, sc.nch, pairs, guess, marg);
        }
        hipLaunchKernelGGL(plsa::k_mt_scale_v, dim3(grid_for(c, (i64)k * m, 256)), dim3(256), 0, c->stream,
                           words.as<unsigned>(), marg, k, (int)m, Vtmp);
    }
    CHK(launch_v_to_vt(c, Vtmp, c->Vt[0].as<float>(), k));
    hipLaunchKernelGGL(plsa::k_mt_init_u, dim3(iplan::init_u_grid(n)), dim3(64), 0, c->stream,
                       words.as<unsigned>(), ms.v_doubles, n, k, kp, c->U[0].as<float>());
    CHK(launch_check(c, "k_mt_init_u"));
    HIPCHK(c, hipMemcpyAsync(state_io, fin.p, sizeof(unsigned) * 625, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int plsa_init_factors_mt19937(plsa_ctx *c, int32_t k, uint32_t *state_io /*[625]*/) {
    if (!state_io) return fail(c, "plsa_init_factors_mt19937: state_io is NULL");
    return mt_init(c, k, state_io, nullptr);
}

int plsa_mt_marginals(plsa_ctx *c, double *out, int32_t k) {
    HIPCHK(c, hipSetDevice(c->device));
    if (!out || k <= 0 || k > 1024 || !c->mt_fin.p || k != c->k)
        return fail(c, "plsa_mt_marginals: no MT19937 initialisation with k=%d on this context", k);
    HIPCHK(c, hipMemcpy(out, c->mt_fin.as<unsigned>() + plsa::init::MARG_WORD, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost));
    return 0;
}

int plsa_refit_init_mt19937(plsa_ctx *c, const float *V, int64_t m, int32_t k, uint32_t *state_io /*[625]*/) {
    if (!state_io || !V) return fail(c, "plsa_refit_init_mt19937: NULL argument");
    if (m != c->m) return fail(c, "plsa_refit_init_mt19937: topics have %lld words, the active matrix %lld", (long long)m, (long long)c->m);
    return mt_init(c, k, state_io, V);
}

int plsa_host_mt19937_jump(uint32_t *key, int32_t log2_blocks) {
    if (!key || log2_blocks < 0 || log2_blocks > 40) return 1;
    uint32_t g[624];
    if (!mtjump::block_jump_polynomial(log2_blocks, g)) return 1;
    mtjump::apply_jump(key, g);
    return 0;
}

int plsa_get_factors(plsa_ctx *c, float *U, float *V) {
    HIPCHK(c, hipSetDevice(c->device));
    CHK(need_factors(c));
    if (V) {        // transposed on the device first: it is in flight while P(z|d) travels
        CHK(ensure(c, c->tmp0, sizeof(float) * (size_t)c->k * c->m));
        CHK(launch_vt_to_v(c, c->tmp0.as<float>()));
    }
    if (U) {
        if (c->kp == c->k)      // rows are contiguous: one linear copy (the strided 2-D form ran at 10 GB/s from 1 M x 64)
            CHK(copy_to_host(c, U, c->U[c->cu].p, sizeof(float) * (size_t)c->n * c->k));
        else
            HIPCHK(c, hipMemcpy2DAsync(U, sizeof(float) * c->k, c->U[c->cu].p, sizeof(float) * c->kp,
                                       sizeof(float) * c->k, (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
    }
    if (V) CHK(copy_to_host(c, V, c->tmp0.p, sizeof(float) * (size_t)c->k * c->m));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int plsa_copy_components_to_device(plsa_ctx *c, void *dst) {
    HIPCHK(c, hipSetDevice(c->device));
    CHK(need_factors(c));
    CHK(launch_vt_to_v(c, reinterpret_cast<float *>(dst)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
