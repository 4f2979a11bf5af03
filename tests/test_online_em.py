"""Online (stepwise) EM on the device (include/plsa_hip_online.h, enstop_amd/online.py).

The definitions the tests restate.  State: topics V, statistic S (host arrays [k, m]), step counter t.  One step on a block:
(1) inner_iter frozen-topic iterations over the block's rows under the state's V; (2) the fused accumulate of
plsa_em_accumulate under the state's V -- the block's P(z|d) is then final, its accumulator holds the block's sums Vacc;
(3) S' = fmaf(b, Vacc, a S) in float32 with a = (float)(1 - rho), b = (float)(rho scale); norm = float64 fixed-order column
sums of S' rounded to float32; V' = S' / norm.  rho_t = (tau0 + t)^(-kappa); scale = 1 / weighted tokens of the block;
set_topics(V0) sets S_0 = V0 / k and t = 0.

Kernel-level tests run on matrix_corpus(k) of test_pass_matrix.py (640 x 480: empty documents, the heavy word, the 300-word
document, the subnormal block) cut into 3 blocks by row_ranges_by_nnz, for k in {3, 6, 16, 21, 64, 130, 300}: padding topics,
the 8 x 2 document pass at kp = 64, two- and four-chunk lanes, and one and two column sweeps of the blend (kp = 132, 300).

  1. a step at rho = 1, scale = 1, inner_iter = 0 has the bits of em_accumulate + em_finish on a sibling engine
  2. the blend from the device's own accumulator: S' within one float32 ulp of round32(b acc + round32(a S)) evaluated in
     float64 (a double rounding is the only slack), V' within 4 * 2^-24 relative of S' / colsum64(S')
  3. a step with inner_iter = j is j single refit iterations on a sibling, then the step with inner_iter = 0
  4. plsa_fit_online is the step iterated; the hand-driven run synchronises after every step, the driver never does, so a
     missing dependency between two block contexts shows as a difference
  5. refusals launch nothing and leave everything as it was; the state survives its block contexts
  6. partial_fit is three hand-driven steps
  7. end to end on the planted corpus of tests/online_model.py: not worse than 20 batch iterations on the device, and within
     a measured gap of the float64 model

The pad columns k .. kp of S and V cannot be read through the ABI (its host tables are [k, m]); what can be seen of them is
checked: the accumulator the blend reads has zero pads, and every visible result equals a computation that never sees them.

Measured on an MI355X (test 7; written into DESIGN.md section 17): see GAP_L and GAP_P below.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import online_model as om
from test_fit_driver import PLSA_FUSED, PLSA_GRAPH, PLSA_SHARDED, same_bits
from test_pass_matrix import C_FACTOR, U32, check, matrix_corpus
from test_tempered_em import ulp_distance

PLSA_REFERENCE_SUMS, PLSA_REFERENCE_LL = 256, 512
THRESH = 1e-32
K_ONLINE = [3, 6, 16, 21, 64, 130, 300]
N_BLOCKS = 3
# largest relative gaps between the device and the float64 model on the planted corpus, as measured on an MI355X: per-epoch
# L_e and final held-out perplexity.  The test asserts 10 x these; a gap above 1e-3 means the two runs have left each other.
GAP_L = 4.3e-8          # measured 4.252e-08 (epochs 1 and 2)
GAP_P = 2.6e-8          # measured 2.599e-08 (274.1856 on both sides)


@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


@functools.lru_cache(maxsize=None)
def blocks_of(k):
    """matrix_corpus(k) cut into 3 blocks of whole documents: ([(X_b, U_b, sw_b)], V, ranges)"""
    from enstop_amd.sharded import row_ranges_by_nnz
    X, U, V, sw = matrix_corpus(k)
    ranges = row_ranges_by_nnz(X.indptr, N_BLOCKS)
    assert ranges[0][0] == 0 and ranges[-1][1] == X.shape[0] and all(b > a for a, b in ranges)
    return [(X[a:b], U[a:b], sw[a:b]) for a, b in ranges], V, ranges


def tokens_of(X, sw=None):
    rows = np.asarray(X.astype(np.float32).astype(np.float64).sum(axis=1)).ravel()
    return float(rows.sum() if sw is None else np.dot(rows, np.asarray(sw, np.float64)))


def other_topics(V):
    """topics a block context holds for itself and a step must never read"""
    W = np.roll(V, 1, axis=0)[:, ::-1].copy()
    return W


def planted_statistic(k, m, seed=0):
    """finite, positive, with some exact zeros and one all-zero word"""
    rs = np.random.RandomState(4000 + 7 * k + seed)
    S = (rs.rand(k, m) * 1e-3).astype(np.float32)
    S[rs.rand(k, m) < 0.05] = 0.0
    S[:, 17] = 0.0
    return S


def block_engine(amd, Xb, Ub, V):
    eng = amd.Engine()
    eng.upload_csr(Xb)
    eng.set_factors(Ub, V)
    return eng


# ------------------------------------------------------------------------------------------------
# 1. rho = 1: accumulate + finish
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K_ONLINE)
def test_a_step_at_rho_one_is_accumulate_and_finish(amd, k):
    blocks, V, _ = blocks_of(k)
    m = V.shape[1]
    with amd.Engine() as home, amd.OnlineState(home, m, k) as state:
        for b, (Xb, Ub, swb) in enumerate(blocks):
            for weighted in (False, True):
                sw = swb if weighted else None
                with block_engine(amd, Xb, Ub, V) as sib:
                    ll_ref = sib.em_accumulate(sw, THRESH, want_ll=True)
                    acc_ref = sib.accumulator_get().reshape(m, -1)
                    sib.em_finish()
                    U_ref, V_ref = sib.get_factors()
                own = other_topics(V)
                with block_engine(amd, Xb, Ub, own) as eng:
                    state.set_topics(V).statistic_set(planted_statistic(k, m, b))
                    assert state.steps == 0
                    ll = state.step(eng, 1.0, 1.0, 0, sw, THRESH, want_ll=True, flags=PLSA_FUSED)
                    tag = "k=%d block %d weighted=%s" % (k, b, weighted)
                    same_bits(state.get_topics(), V_ref, tag + ": V")
                    U1, V1 = eng.get_factors()
                    same_bits(U1, U_ref, tag + ": P(z|d)")
                    same_bits(V1, own, tag + ": the block's own topic table moved")
                    same_bits(np.float64(ll), np.float64(ll_ref), tag + ": ll_partial")
                    acc = eng.accumulator_get().reshape(m, -1)
                    same_bits(acc, acc_ref, tag + ": accumulator")
                    assert (acc[:, k:] == 0).all()
                    same_bits(state.statistic_get(), np.ascontiguousarray(acc[:, :k].T), tag + ": S' = Vacc at a = 0, b = 1")
                    assert state.steps == 1


# ------------------------------------------------------------------------------------------------
# 2. the blend, from the device's own accumulator
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K_ONLINE)
def test_the_blend_from_the_devices_own_accumulator(amd, k):
    blocks, V, _ = blocks_of(k)
    m = V.shape[1]
    rho = 0.3
    worst_s, worst_v = 0, 0.0
    with amd.Engine() as home, amd.OnlineState(home, m, k) as state:
        for b, (Xb, Ub, swb) in enumerate(blocks):
            scale = 1.0 / tokens_of(Xb, swb)
            S0 = planted_statistic(k, m, b)
            with block_engine(amd, Xb, Ub, other_topics(V)) as eng:
                state.set_topics(V).statistic_set(S0)
                state.step(eng, rho, scale, 0, swb, THRESH, flags=PLSA_FUSED)
                acc = eng.accumulator_get().reshape(m, -1)
            assert (acc[:, k:] == 0).all()                       # the pads the blend reads
            acc = np.ascontiguousarray(acc[:, :k].T)             # [k, m] like the host tables
            S1, V1 = state.statistic_get(), state.get_topics()
            a, bb = np.float32(1.0 - rho), np.float32(rho * scale)
            aS = (np.float64(a) * S0.astype(np.float64)).astype(np.float32)
            want = (np.float64(bb) * acc.astype(np.float64) + aS.astype(np.float64)).astype(np.float32)
            d = ulp_distance(S1, want)
            assert d.max() <= 1, "k=%d block %d: S' %d ulp from round32(b acc + round32(a S))" % (k, b, d.max())
            assert (S1[(S0 == 0) & (acc == 0)] == 0).all()
            worst_s = max(worst_s, int(d.max()))
            S64 = S1.astype(np.float64)
            norm = S64.sum(axis=1, keepdims=True)
            assert (norm > 0).all()
            worst_v = max(worst_v, check("k=%d block %d: V'" % (k, b), V1, S64 / norm, C_FACTOR * U32))
    print("\nk=%d: S' at most %d ulp from the rounded blend, V' at %.3f of its bound" % (k, worst_s, worst_v))


# ------------------------------------------------------------------------------------------------
# 3. inner iterations
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K_ONLINE)
def test_inner_iterations_are_single_refit_iterations_before_the_step(amd, k):
    blocks, V, _ = blocks_of(k)
    m = V.shape[1]
    rho = 0.3
    Xb, Ub, swb = blocks[1]
    scale = 1.0 / tokens_of(Xb, swb)
    S0 = planted_statistic(k, m)
    with amd.Engine() as home, amd.OnlineState(home, m, k) as state:
        for j in (1, 3):
            with block_engine(amd, Xb, Ub, V) as sib:
                for _ in range(j):
                    iters, _ = sib.refit(swb, 1, 1, 0.0, THRESH, PLSA_FUSED)
                    assert iters == 1
                Uj, _ = sib.get_factors()
            results = []
            for U_start, inner in ((Uj, 0), (Ub, j)):
                with block_engine(amd, Xb, U_start, other_topics(V)) as eng:
                    state.set_topics(V).statistic_set(S0)
                    ll = state.step(eng, rho, scale, inner, swb, THRESH, want_ll=True, flags=PLSA_FUSED)
                    results.append((eng.get_factors()[0], state.get_topics(), state.statistic_get(), np.float64(ll)))
            for name, x, y in zip(("P(z|d)", "V", "S", "ll_partial"), *results):
                same_bits(x, y, "k=%d inner_iter=%d: %s" % (k, j, name))
            assert not np.array_equal(results[0][0], Ub)


@pytest.mark.gpu
def test_a_fold_is_refit_iterations_under_the_states_topics_and_nothing_else(amd):
    k = 21
    blocks, V, _ = blocks_of(k)
    m = V.shape[1]
    Xb, Ub, swb = blocks[0]
    with amd.Engine() as home, amd.OnlineState(home, m, k) as state, block_engine(amd, Xb, Ub, V) as sib, \
            block_engine(amd, Xb, Ub, other_topics(V)) as eng:
        S0 = planted_statistic(k, m)
        state.set_topics(V).statistic_set(S0)
        for _ in range(2):
            sib.refit(swb, 1, 1, 0.0, THRESH, PLSA_FUSED)
        state.fold(eng, 2, swb, THRESH, PLSA_FUSED)
        same_bits(eng.get_factors()[0], sib.get_factors()[0], "fold: P(z|d)")
        same_bits(state.get_topics(), V, "fold moved V")
        same_bits(state.statistic_get(), S0, "fold moved S")
        assert state.steps == 0


# ------------------------------------------------------------------------------------------------
# 4. the loop is the step iterated, and steps are ordered
# ------------------------------------------------------------------------------------------------
def hand_driven(amd, X, U0, V0, sw, n_blocks, n_epochs, inner_iter, kappa=0.7, tau0=10.0, perm=None):
    """the steps of plsa_fit_online through Engine and OnlineState, the host waiting for the device after every one"""
    from enstop_amd.sharded import row_ranges_by_nnz
    n, m = X.shape
    k = U0.shape[1]
    order = np.arange(n) if perm is None else perm
    Xp, Up, swp = X[order], U0[order], sw[order]
    ranges = row_ranges_by_nnz(Xp.indptr, n_blocks)
    engines = []
    L, rhos, t = [], [], 0
    with amd.Engine() as home, amd.OnlineState(home, m, k) as state:
        try:
            for a, b in ranges:
                eng = block_engine(amd, Xp[a:b], Up[a:b], V0)
                eng.set_sample_weight(swp[a:b])
                engines.append(eng)
            state.set_topics(V0)
            for e in range(n_epochs):
                Le = 0.0
                for eng, (a, b) in zip(engines, ranges):
                    rho = (tau0 + t) ** (-kappa)
                    Le += state.step(eng, rho, 1.0 / tokens_of(Xp[a:b], swp[a:b]), inner_iter, None, THRESH, want_ll=True,
                                     flags=PLSA_FUSED)
                    eng.synchronize()
                    rhos.append(rho)
                    t += 1
                L.append(Le)
            U = np.zeros((n, k), np.float32)
            for eng, (a, b) in zip(engines, ranges):
                state.fold(eng, max(inner_iter, 1), None, THRESH, PLSA_FUSED)
                eng.synchronize()
                U[order[a:b]] = eng.get_factors(want_v=False)[0]
            V = state.get_topics()
            assert state.steps == n_blocks * n_epochs
        finally:
            for eng in engines:
                eng.close()
    return U, V, L, rhos, ranges


def start_of(k):
    """matrix_corpus(k) with its factors as a driver starts from them: tuple factors go through plsa_init like plsa_fit's, which
    normalises their rows in float64 before the float32 cast (the subnormal documents become ordinary ones)"""
    from enstop_amd._driver import host_factors
    X, U0, V0, sw = matrix_corpus(k)
    U0, V0 = host_factors(k, (U0, V0), None, X=X)
    return X, U0, V0, sw


@pytest.mark.gpu
@pytest.mark.parametrize("k", [6, 64])
def test_the_loop_is_the_step_iterated_and_steps_are_ordered(amd, k):
    X, U0, V0, sw = start_of(k)
    U_ref, V_ref, L_ref, rho_ref, ranges = hand_driven(amd, X, U0, V0, sw, N_BLOCKS, 2, 3)
    kwargs = dict(sample_weight=sw, init=(U0, V0), n_batches=N_BLOCKS, n_epochs=2, inner_iter=3, tolerance=0.0,
                  shuffle_documents=False, e_step_thresh=THRESH, random_state=0)
    for attempt in range(2):
        U, V, info = amd.plsa_fit_online(X, k, return_info=True, **kwargs)
        same_bits(U, U_ref, "k=%d run %d: P(z|d)" % (k, attempt))
        same_bits(V, V_ref, "k=%d run %d: P(w|z)" % (k, attempt))
        np.testing.assert_array_equal(np.array(info["log_likelihoods"]), np.array(L_ref))
        assert info["rho"] == rho_ref == [(10.0 + t) ** -0.7 for t in range(2 * N_BLOCKS)]
        assert info["n_epochs"] == 2 and info["n_steps"] == 2 * N_BLOCKS and info["block_ranges"] == ranges
        assert info["permutation"] is None
        assert info["bytes_per_block_context"] == 3 * 4 * X.shape[1] * ((k + 3) // 4 * 4)
    # without the likelihoods no step waits for the device: the ordering between the block contexts is the event's alone
    for attempt in range(2):
        U, V = amd.plsa_fit_online(X, k, **kwargs)
        same_bits(U, U_ref, "k=%d enqueue-only run %d: P(z|d)" % (k, attempt))
        same_bits(V, V_ref, "k=%d enqueue-only run %d: P(w|z)" % (k, attempt))
    assert not np.array_equal(V_ref, V0)


@pytest.mark.gpu
def test_shuffled_documents_come_back_in_the_callers_order(amd):
    k = 16
    X, U0, V0, sw = start_of(k)
    perm = np.random.RandomState(5).permutation(X.shape[0])          # tuple factors draw nothing: the permutation comes first
    U_ref, V_ref, L_ref, _, _ = hand_driven(amd, X, U0, V0, sw, N_BLOCKS, 2, 1, perm=perm)
    U, V, info = amd.plsa_fit_online(X, k, sample_weight=sw, init=(U0, V0), n_batches=N_BLOCKS, n_epochs=2, inner_iter=1,
                                     tolerance=0.0, shuffle_documents=True, e_step_thresh=THRESH, random_state=5,
                                     return_info=True)
    np.testing.assert_array_equal(info["permutation"], perm)
    same_bits(U, U_ref, "shuffled: P(z|d) in the caller's order")
    same_bits(V, V_ref, "shuffled: P(w|z)")
    np.testing.assert_array_equal(np.array(info["log_likelihoods"]), np.array(L_ref))
    plain = amd.plsa_fit_online(X, k, sample_weight=sw, init=(U0, V0), n_batches=N_BLOCKS, n_epochs=2, inner_iter=1,
                                tolerance=0.0, shuffle_documents=False, e_step_thresh=THRESH, random_state=5)
    assert not np.array_equal(plain[1], V)                           # the order of the documents matters to the result


@pytest.mark.gpu
def test_the_driver_refuses_what_it_cannot_run(amd):
    X, U0, V0, sw = matrix_corpus(6)
    for kwargs in (dict(n_batches=0), dict(n_batches=257), dict(inner_iter=-1), dict(rho=1.5), dict(tau0=0.5)):
        with pytest.raises(ValueError):
            amd.plsa_fit_online(X, 6, init=(U0, V0), **kwargs)
    empty = sp.csr_matrix((4, X.shape[1]), dtype=np.float32)
    with pytest.raises(ValueError, match="no tokens"):
        amd.plsa_fit_online(empty, 6, n_batches=2, random_state=0)


# ------------------------------------------------------------------------------------------------
# 5. refusals, and the state outlives its block contexts
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_launch_nothing_and_leave_state_and_factors(amd):
    k = 16
    blocks, V, _ = blocks_of(k)
    m = V.shape[1]
    Xb, Ub, swb = blocks[0]
    own = other_topics(V)
    S0 = planted_statistic(k, m)
    nan, inf = float("nan"), float("inf")
    with amd.Engine() as home, amd.OnlineState(home, m, k) as state, block_engine(amd, Xb, Ub, own) as eng:
        state.set_topics(V).statistic_set(S0)
        state.step(eng, 0.5, 1.0, 0, swb, THRESH, flags=PLSA_FUSED)       # t = 1 and everything allocated, then the refusals
        U1, _ = eng.get_factors()
        V1, S1 = state.get_topics(), state.statistic_get()
        eng.timing(True)
        eng.timing_reset()
        bad = [(dict(flags=0), "PLSA_FUSED"), (dict(flags=PLSA_FUSED | PLSA_SHARDED), "PLSA_SHARDED"),
               (dict(flags=PLSA_FUSED | PLSA_GRAPH), "PLSA_GRAPH"), (dict(flags=PLSA_FUSED | PLSA_REFERENCE_SUMS), "PLSA_REFERENCE_SUMS"),
               (dict(flags=PLSA_FUSED | PLSA_REFERENCE_LL), "PLSA_REFERENCE_LL"),
               (dict(rho=0.0), "rho"), (dict(rho=-0.5), "rho"), (dict(rho=1.0000001), "rho"), (dict(rho=nan), "rho"),
               (dict(rho=inf), "rho"), (dict(scale=0.0), "scale"), (dict(scale=-1.0), "scale"), (dict(scale=nan), "scale"),
               (dict(scale=inf), "scale"), (dict(inner_iter=-1), "inner_iter")]
        for change, word in bad:
            args = dict(dict(rho=0.5, scale=1.0, inner_iter=1, flags=PLSA_FUSED), **change)
            with pytest.raises(amd.DeviceError, match=word):
                state.step(eng, args["rho"], args["scale"], args["inner_iter"], swb, THRESH, want_ll=True, flags=args["flags"])
        with pytest.raises(amd.DeviceError, match="PLSA_SHARDED"):
            state.fold(eng, 1, swb, THRESH, PLSA_FUSED | PLSA_SHARDED)
        with pytest.raises(amd.DeviceError, match="n_iter"):
            state.fold(eng, -1, swb, THRESH, PLSA_FUSED)
        for arithmetic in ("reference", "reference_source"):
            eng.set_arithmetic(arithmetic)
            with pytest.raises(amd.DeviceError, match="reference arithmetic"):
                state.step(eng, 0.5, 1.0, 0, swb, THRESH, flags=PLSA_FUSED)
            with pytest.raises(amd.DeviceError, match="reference arithmetic"):
                state.fold(eng, 1, swb, THRESH, PLSA_FUSED)
        eng.set_arithmetic(None)
        with amd.OnlineState(home, m + 4, k) as wider, amd.OnlineState(home, m, k + 1) as deeper:
            for other in (wider, deeper):
                other.set_topics(np.full((other.k, other.m), 1.0 / other.m, np.float32))
                with pytest.raises(amd.DeviceError, match="words with k="):
                    other.step(eng, 0.5, 1.0, 0, swb, THRESH, flags=PLSA_FUSED)
                with pytest.raises(amd.DeviceError, match="words with k="):
                    other.fold(eng, 1, swb, THRESH, PLSA_FUSED)
                assert other.steps == 0
        with amd.Engine() as bare:                                        # a context without corpus or factors
            with pytest.raises(amd.DeviceError):
                state.step(bare, 0.5, 1.0, 0, None, THRESH, flags=PLSA_FUSED)
        assert eng.timing_report() == {}, eng.timing_report()             # nothing was launched
        eng.timing(False)
        U2, V2 = eng.get_factors()
        same_bits(U2, U1, "a refusal moved the block's P(z|d)")
        same_bits(V2, own, "a refusal moved the block's topic table")
        same_bits(state.get_topics(), V1, "a refusal moved V")
        same_bits(state.statistic_get(), S1, "a refusal moved S")
        assert state.steps == 1


@pytest.mark.gpu
def test_the_state_survives_release_scratch_and_the_destruction_of_a_block_context(amd):
    k = 64
    blocks, V, _ = blocks_of(k)
    m = V.shape[1]
    (Xa, Ua, swa), (Xb, Ub, swb) = blocks[0], blocks[1]
    steps = ((Xa, Ua, swa, 0.5), (Xb, Ub, swb, 0.4), (Xa, Ua, swa, 0.3))

    def run(disturb):
        with amd.Engine() as home, amd.OnlineState(home, m, k) as state:
            state.set_topics(V)
            for X_, U_, sw_, rho in steps:
                eng = block_engine(amd, X_, U_, other_topics(V))
                state.step(eng, rho, 1.0 / tokens_of(X_, sw_), 1, sw_, THRESH, flags=PLSA_FUSED)
                if disturb:
                    eng.release_scratch()
                    state.fold(eng, 1, sw_, THRESH, PLSA_FUSED)
                    eng.close()                                           # destroyed with the step just enqueued
                else:
                    state.fold(eng, 1, sw_, THRESH, PLSA_FUSED)
                    eng.synchronize()
                    eng.close()
            return state.get_topics(), state.statistic_get(), state.steps

    quiet, disturbed = run(False), run(True)
    same_bits(disturbed[0], quiet[0], "V after release_scratch / destroy of the block contexts")
    same_bits(disturbed[1], quiet[1], "S after release_scratch / destroy of the block contexts")
    assert quiet[2] == disturbed[2] == 3 and np.isfinite(quiet[0]).all()


# ------------------------------------------------------------------------------------------------
# 6. partial_fit
# ------------------------------------------------------------------------------------------------
def count_corpus(k):
    """matrix_corpus(k) as integer counts (float input would be row-normalised by the estimator, like PLSA's)"""
    X, _, _, sw = matrix_corpus(k)
    Xi = sp.csr_matrix((np.ceil(X.data).astype(np.int32), X.indices.copy(), X.indptr.copy()), shape=X.shape)
    return Xi, sw


@pytest.mark.gpu
@pytest.mark.parametrize("k", [6, 64])
def test_partial_fit_is_three_hand_driven_steps(amd, k):
    from enstop_amd.sharded import row_ranges_by_nnz
    from enstop_amd.utils import normalize
    X, sw = count_corpus(k)
    n, m = X.shape
    ranges = row_ranges_by_nnz(X.indptr, N_BLOCKS)
    seed, inner = 11, 3
    est = amd.OnlinePLSA(n_components=k, inner_iter=inner, random_state=seed)
    rng = np.random.RandomState(seed)
    V0 = rng.rand(k, m)
    normalize(V0, axis=1)
    with amd.Engine() as eng, amd.OnlineState(eng, m, k) as state:
        state.set_topics(V0.astype(np.float32))
        topics = state.get_topics()
        same_bits(topics, V0.astype(np.float32), "set_topics / get_topics round trip")
        for t, (a, b) in enumerate(ranges):
            assert est.partial_fit(X[a:b], sample_weight=sw[a:b]) is est
            U = rng.rand(b - a, k)
            normalize(U, axis=1)
            eng.upload_csr(X[a:b])
            eng.set_factors(U.astype(np.float32), topics)
            state.step(eng, (10.0 + t) ** -0.7, 1.0 / tokens_of(X[a:b], sw[a:b]), inner, sw[a:b], THRESH, flags=PLSA_FUSED)
            topics = state.get_topics()
            same_bits(est.components_, topics, "k=%d call %d: components_" % (k, t))
            same_bits(est.embedding_, eng.get_factors(want_v=False)[0], "k=%d call %d: embedding_" % (k, t))
            assert est.n_steps_ == t + 1 == state.steps
    np.testing.assert_allclose(est.components_.sum(axis=1), 1.0, rtol=1e-5)
    T = est.transform(X[:50])
    assert T.shape == (50, k) and np.isfinite(T).all()
    nonempty = np.diff(X[:50].indptr) > 0
    np.testing.assert_allclose(T[nonempty].sum(axis=1), 1.0, rtol=1e-5)
    with pytest.raises(ValueError, match="words"):
        est.partial_fit(sp.csr_matrix(X[:10, :m - 1]))
    assert est.n_steps_ == N_BLOCKS


@pytest.mark.gpu
def test_the_estimator_fits_through_plsa_fit_online(amd):
    k = 16
    X, sw = count_corpus(k)
    params = dict(n_batches=N_BLOCKS, n_epochs=2, inner_iter=2, tolerance=0.0, random_state=3)
    est = amd.OnlinePLSA(n_components=k, **params)
    E = est.fit_transform(X, sample_weight=sw)
    good = np.diff(X.indptr) > 0
    U, V, info = amd.plsa_fit_online(X[good], k, sample_weight=sw[good], return_info=True, **params)
    same_bits(est.components_, V, "components_")
    same_bits(np.ascontiguousarray(E[good]).astype(np.float32), U, "embedding_")
    assert (E[~good] == 0).all() and est.n_iter_ == 2 and est.n_steps_ == 2 * N_BLOCKS
    assert est.online_info_["rho"] == info["rho"]
    assert np.isfinite(est.perplexity(X[good][:100], method="fold_in"))


# ------------------------------------------------------------------------------------------------
# 7. end to end on the planted corpus
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_end_to_end_on_the_planted_corpus(amd):
    observed, held, scored, U0, V0 = om.the_split()
    model = om.model()
    f = om.FIT
    U, V, info = amd.plsa_fit_online(observed, f["k"], init=(U0, V0), n_batches=f["n_batches"], n_epochs=om.EPOCHS,
                                     inner_iter=f["inner_iter"], kappa=f["kappa"], tau0=f["tau0"], tolerance=0.0,
                                     shuffle_documents=True, random_state=f["random_state"], return_info=True)
    np.testing.assert_array_equal(info["permutation"], model["perm"])
    assert info["n_epochs"] == om.EPOCHS and info["n_steps"] == om.EPOCHS * f["n_batches"]
    online = om.perplexity(held, scored, U.astype(np.float64), V.astype(np.float64))
    Ub, Vb, binfo = amd.plsa_fit(observed, f["k"], None, init=(U0, V0), n_iter=f["batch_iterations"], n_iter_per_test=10,
                                 tolerance=0.0, return_info=True)
    assert binfo["n_iter"] == f["batch_iterations"]
    batch = om.perplexity(held, scored, Ub.astype(np.float64), Vb.astype(np.float64))
    L_dev, L_model = np.array(info["log_likelihoods"]), np.array(model["L"][:om.EPOCHS])
    gap_l = float(np.max(np.abs(L_dev - L_model) / np.abs(L_model)))
    gap_p = abs(online - model["online_perplexity"][om.EPOCHS - 1]) / model["online_perplexity"][om.EPOCHS - 1]
    gap_b = abs(batch - model["batch_perplexity"]) / model["batch_perplexity"]
    print("\nheld-out perplexity after %d epochs: device %.4f, model %.4f; batch EM after %d iterations: device %.4f, model %.4f"
          % (om.EPOCHS, online, model["online_perplexity"][om.EPOCHS - 1], f["batch_iterations"], batch, model["batch_perplexity"]))
    print("largest relative gap device / float64 model: L_e %.3e, perplexity %.3e (batch EM's perplexity %.3e)"
          % (gap_l, gap_p, gap_b))
    print("L_e device %r model %r" % (L_dev.tolist(), L_model.tolist()))
    assert online <= batch, (online, batch)
    assert gap_l <= 10 * GAP_L, gap_l
    assert gap_p <= 10 * GAP_P, gap_p
