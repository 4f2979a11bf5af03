"""Online variational Bayes LDA on the device (enstop_amd/include/plsa_hip_lda_online.h, enstop_amd/lda_online.py; DESIGN.md
section 21).

    one step on block b:  doc_iter - 1 gamma-only rounds and one full round under the state's tables B (the block's own topic
                          table is never read or written), the block's raw counts n_wz left in its accumulator;
                          lambda' = fmaf(b, n_wz, fmaf(a, lambda, c)), a = (float)(1 - rho), b = (float)(rho scale),
                          c = (float)(rho eta); B and its sums re-formed from lambda' (k_lda_online_blend leaves the slab sums
                          k_lda_topic_partial would have computed).

The kernel-level tests run on test_lda_em.corpus(k) (640 x 480, about 4 000 non-zeros: empty documents, the 300-word document,
the heavy word, word 9 without entries) cut into 3 blocks of whole documents, for k in {3, 6, 21, 64, 130, 300, 1024}: kq = 1,
pads, the 8 x 2 document shape, and one, two and four column sweeps of the blend (kp = 132 and 300: a last sweep narrower than
256 columns).  Priors (0.5, 0.5) and (0.1, 0.05), the start of test_lda_em.start.  Every block context holds
other_topics(lambda) as its own topic table, which must come back untouched.

Nearly everything is held to bits: a step at rho = 1 and scale = 1 IS an iteration of plsa_lda_fit on the block
(fmaf(1, acc, fmaf(0, lambda, eta_f)) is acc + eta_f rounded once), a fold is plsa_lda_refit, bound_partial is plsa_lda_bound
without topics, and the driver is the step iterated.  The blend itself is held to one float32 ulp of
round32(b acc + round32(a lambda + c)) evaluated in float64 from the device's own accumulator: the float64 evaluation rounds
a lambda + c before it rounds to float32 (and b acc + that likewise), a double rounding, which is the only slack.

The pad columns k .. kp of lambda and B cannot be read through the ABI.  The blend writes 0 there by the plan's mask, which
tests/test_lda_online_plan_host.py checks for every active lane; here every later step is held to a computation on a fresh
context, which never sees a pad.
"""
import functools
import pickle

import numpy as np
import pytest
import scipy.sparse as sp

import lda_online_model as M
import test_lda_em as le
from test_fit_driver import PLSA_FUSED, PLSA_GRAPH, PLSA_SHARDED, same_bits
from test_online_em import other_topics
from test_tempered_em import ulp_distance

PLSA_REFERENCE_SUMS, PLSA_REFERENCE_LL = 256, 512
THRESH = le.THRESH
K = [3, 6, 21, 64, 130, 300, 1024]
PRIORS = [(0.5, 0.5), (0.1, 0.05)]
N_BLOCKS = 3
# largest relative gaps between the device and the float64 model on the planted corpus, as measured on an MI355X: per-epoch
# L_e and final held-out perplexity.  The test asserts 10 x these -- room for run-to-run differences in nothing but launch
# geometry knobs -- and that 10 x measured stays below 1e-3: a gap above that means the two runs have left each other.
GAP_L = 2.6e-8          # measured 2.539e-08 (epoch 2: -1271912.1799 on the device, -1271912.2122 in the model)
GAP_P = 6.2e-8          # measured 6.127e-08 (268.5289 on both sides; batch LDA after 20 iterations 297.7707 / 297.7706)


@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


@functools.lru_cache(maxsize=None)
def blocks_of(k):
    """test_lda_em.corpus(k) cut into 3 blocks of whole documents: (X, [X_b], ranges)"""
    from enstop_amd.sharded import row_ranges_by_nnz
    X, _, _ = le.corpus(k)
    ranges = row_ranges_by_nnz(X.indptr, N_BLOCKS)
    assert ranges[0][0] == 0 and ranges[-1][1] == X.shape[0] and all(b > a for a, b in ranges)
    return X, [X[a:b] for a, b in ranges], ranges


def block_engine(amd, Xb, gamma, lam):
    eng = amd.Engine()
    eng.upload_csr(Xb)
    eng.set_factors(gamma, lam)
    return eng


def one_iteration(doc_iter=1):
    return dict(le.ONE, doc_iter=doc_iter)


def planted_lambda(k, alpha, eta, seed=0):
    """the start's lambda with one entry in twenty tiny (1e-6 .. 2e-6): positive, far below eta and the counts"""
    lam = le.start(k, alpha, eta)[1].copy()
    rs = np.random.RandomState(5000 + 7 * k + seed)
    tiny = rs.rand(*lam.shape) < 0.05
    lam[tiny] = (1e-6 * (1.0 + rs.rand(int(tiny.sum())))).astype(np.float32)
    return lam


def blend64(lam, acc, rho, scale, eta):
    """round32(b acc + round32(a lambda + c)) evaluated in float64, with the float32 coefficients of the header"""
    a, b, c = np.float32(1.0 - rho), np.float32(rho * scale), np.float32(rho * eta)
    inner = (np.float64(a) * lam.astype(np.float64) + np.float64(c)).astype(np.float32)
    return (np.float64(b) * acc.astype(np.float64) + inner.astype(np.float64)).astype(np.float32), inner


def counts_of(eng, k):
    """the block's raw counts n_wz as [k, m], read back from its accumulator; the pads the blend reads are 0"""
    m = eng.shape[1]
    acc = eng.accumulator_get().reshape(m, -1)
    assert (acc[:, k:] == 0).all()
    return np.ascontiguousarray(acc[:, :k].T)


# ------------------------------------------------------------------------------------------------
# 1. rho = 1, scale = 1: an iteration of plsa_lda_fit
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_a_step_at_rho_one_is_a_batch_iteration(amd, k):
    X, blocks, ranges = blocks_of(k)
    m = X.shape[1]
    with amd.Engine() as home, amd.LdaOnlineState(home, m, k) as state:
        for b, (Xb, (lo, hi)) in enumerate(zip(blocks, ranges)):
            with amd.Engine() as sib, amd.Engine() as eng:
                sib.upload_csr(Xb)
                eng.upload_csr(Xb)
                for alpha, eta in PRIORS:
                    gamma0, lam0 = le.start(k, alpha, eta)
                    own = other_topics(lam0)
                    for doc_iter in (1, 3):
                        tag = "k=%d block %d alpha=%g eta=%g doc_iter=%d" % (k, b, alpha, eta, doc_iter)
                        sib.set_factors(gamma0[lo:hi], lam0)
                        iters, _ = sib.lda_fit(alpha, eta, **one_iteration(doc_iter))
                        assert iters == 1
                        gamma_ref, lam_ref = sib.get_factors()
                        eng.set_factors(gamma0[lo:hi], own)
                        state.set_lambda(lam0)
                        assert state.steps == 0
                        same_bits(state.get_lambda(), lam0, tag + ": set_lambda / get_lambda round trip")
                        assert state.step(eng, alpha, eta, 1.0, 1.0, doc_iter, THRESH, flags=PLSA_FUSED) is None
                        gamma, own_after = eng.get_factors()
                        same_bits(gamma, gamma_ref, tag + ": gamma")
                        same_bits(state.get_lambda(), lam_ref, tag + ": lambda")
                        same_bits(own_after, own, tag + ": the block's own topic table moved")
                        assert state.steps == 1
                        assert not np.array_equal(lam_ref, lam0)


# ------------------------------------------------------------------------------------------------
# 2. the blend, from the device's own accumulator
# ------------------------------------------------------------------------------------------------
RHO, SCALE = 0.3, 37.5


@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_the_blend_from_the_devices_own_accumulator(amd, k):
    X, blocks, ranges = blocks_of(k)
    m = X.shape[1]
    worst = 0
    with amd.Engine() as home, amd.LdaOnlineState(home, m, k) as state:
        for alpha, eta in PRIORS:
            gamma0, _ = le.start(k, alpha, eta)
            for b, (Xb, (lo, hi)) in enumerate(zip(blocks, ranges)):
                lam0 = planted_lambda(k, alpha, eta, b)
                with block_engine(amd, Xb, gamma0[lo:hi], other_topics(lam0)) as eng:
                    state.set_lambda(lam0)
                    state.step(eng, alpha, eta, RHO, SCALE, 1, THRESH, flags=PLSA_FUSED)
                    acc = counts_of(eng, k)
                lam1 = state.get_lambda()
                want, inner = blend64(lam0, acc, RHO, SCALE, eta)
                d = ulp_distance(lam1, want)
                tag = "k=%d alpha=%g eta=%g block %d" % (k, alpha, eta, b)
                assert d.max() <= 1, "%s: lambda' %d ulp from round32(b acc + round32(a lambda + c))" % (tag, d.max())
                assert (lam1 > 0).all() and acc.max() > 0, tag
                # a word without entries in the block -- word 9 in every block -- gets round32(a lambda + c)
                unused = np.asarray(Xb.sum(axis=0)).ravel() == 0
                assert unused[le.UNUSED_WORD] and (acc[:, unused] == 0).all(), tag
                assert ulp_distance(lam1[:, unused], inner[:, unused]).max() <= 1, tag
                worst = max(worst, int(d.max()))
    print("\nk=%d: lambda' at most %d ulp from the rounded blend" % (k, worst))


# ------------------------------------------------------------------------------------------------
# 3. the tables in force are the tables of lambda'
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_the_tables_in_force_are_the_tables_of_the_blended_lambda(amd, k):
    """the step of test 2 on block 0, then a step at rho = 1 on block 1: an iteration of plsa_lda_fit on a fresh context that
    holds block 1 and the lambda' read back.  A slab partial in the wrong place or added in another order out of the fused
    sweep moves S_z, and with it every entry of B; a stale B is the table of another lambda altogether."""
    X, blocks, ranges = blocks_of(k)
    m = X.shape[1]
    (lo0, hi0), (lo1, hi1) = ranges[0], ranges[1]
    with amd.Engine() as home, amd.LdaOnlineState(home, m, k) as state:
        for alpha, eta in PRIORS:
            gamma0, _ = le.start(k, alpha, eta)
            lam0 = planted_lambda(k, alpha, eta)
            state.set_lambda(lam0)
            with block_engine(amd, blocks[0], gamma0[lo0:hi0], other_topics(lam0)) as eng:
                state.step(eng, alpha, eta, RHO, SCALE, 1, THRESH, flags=PLSA_FUSED)
            lam1 = state.get_lambda()
            for doc_iter in (1, 3):
                tag = "k=%d alpha=%g eta=%g doc_iter=%d" % (k, alpha, eta, doc_iter)
                with block_engine(amd, blocks[1], gamma0[lo1:hi1], lam1) as sib:
                    sib.lda_fit(alpha, eta, **one_iteration(doc_iter))
                    gamma_ref, lam_ref = sib.get_factors()
                with block_engine(amd, blocks[1], gamma0[lo1:hi1], other_topics(lam0)) as eng:
                    state.step(eng, alpha, eta, 1.0, 1.0, doc_iter, THRESH, flags=PLSA_FUSED)
                    same_bits(eng.get_factors(want_v=False)[0], gamma_ref, tag + ": gamma of the second step")
                same_bits(state.get_lambda(), lam_ref, tag + ": lambda of the second step")
                # back to lambda' for the next doc_iter: set_lambda forms the tables by k_lda_topic_partial's own sweep, and
                # the two ways to the tables agree (the second step above ran on the blend's)
                state.set_lambda(lam1)


# ------------------------------------------------------------------------------------------------
# 4. a fold is the refit
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_a_fold_is_refit_iterations_under_the_states_tables_and_nothing_else(amd, k):
    X, blocks, ranges = blocks_of(k)
    m = X.shape[1]
    alpha, eta = PRIORS[1]
    gamma0, lam0 = le.start(k, alpha, eta)
    own = other_topics(lam0)
    with amd.Engine() as home, amd.LdaOnlineState(home, m, k) as state:
        state.set_lambda(lam0)
        for b, (Xb, (lo, hi)) in enumerate(zip(blocks, ranges)):
            for n_rounds in (0, 1, 3):
                with block_engine(amd, Xb, gamma0[lo:hi], lam0) as sib:
                    iters, _ = sib.lda_refit(alpha, n_iter=n_rounds, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH,
                                             flags=PLSA_FUSED)
                    assert iters == n_rounds
                    gamma_ref = sib.get_factors(want_v=False)[0]
                with block_engine(amd, Xb, gamma0[lo:hi], own) as eng:
                    state.fold(eng, alpha, n_rounds, THRESH, PLSA_FUSED)
                    gamma, own_after = eng.get_factors()
                tag = "k=%d block %d fold(%d)" % (k, b, n_rounds)
                same_bits(gamma, gamma_ref, tag + ": gamma")
                same_bits(own_after, own, tag + ": the block's own topic table moved")
                same_bits(state.get_lambda(), lam0, tag + ": lambda moved")
                assert state.steps == 0


# ------------------------------------------------------------------------------------------------
# 5. bound_partial
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_bound_partial_is_the_bound_without_topics_at_the_new_gamma_and_the_old_lambda(amd, k):
    """the same kernels in the same geometry on a sibling that holds (X_b, gamma', lambda_old): the same bits"""
    X, blocks, ranges = blocks_of(k)
    m = X.shape[1]
    with amd.Engine() as home, amd.LdaOnlineState(home, m, k) as state:
        for alpha, eta in PRIORS:
            gamma0, _ = le.start(k, alpha, eta)
            for b, (Xb, (lo, hi)) in enumerate(zip(blocks, ranges)):
                lam0 = planted_lambda(k, alpha, eta, b)
                got = {}
                for want_bound in (True, False):
                    with block_engine(amd, Xb, gamma0[lo:hi], other_topics(lam0)) as eng:
                        state.set_lambda(lam0)
                        bound = state.step(eng, alpha, eta, RHO, SCALE, 3, THRESH, want_bound, PLSA_FUSED)
                        got[want_bound] = (bound, eng.get_factors(want_v=False)[0], state.get_lambda())
                tag = "k=%d alpha=%g eta=%g block %d" % (k, alpha, eta, b)
                assert got[False][0] is None
                same_bits(got[True][1], got[False][1], tag + ": asking for the bound moved gamma")
                same_bits(got[True][2], got[False][2], tag + ": asking for the bound moved lambda")
                with block_engine(amd, Xb, got[True][1], lam0) as sib:
                    want = sib.lda_bound(alpha)
                same_bits(np.float64(got[True][0]), np.float64(want), tag + ": bound_partial")
                assert np.isfinite(want)


# ------------------------------------------------------------------------------------------------
# 6. the driver is the step iterated, and steps are ordered
# ------------------------------------------------------------------------------------------------
def hand_driven(amd, X, gamma0, lam0, alpha, eta, n_blocks, n_epochs, doc_iter, kappa=0.7, tau0=10.0, perm=None):
    """the steps of lda_fit_online through Engine and LdaOnlineState, the host waiting for the device after every one"""
    from enstop_amd.sharded import row_ranges_by_nnz
    n, m = X.shape
    k = gamma0.shape[1]
    order = np.arange(n) if perm is None else perm
    Xp, Gp = X[order], gamma0[order]
    ranges = row_ranges_by_nnz(Xp.indptr, n_blocks)
    engines = []
    L, rhos, t = [], [], 0
    with amd.Engine() as home, amd.LdaOnlineState(home, m, k) as state:
        try:
            for a, b in ranges:
                engines.append(block_engine(amd, Xp[a:b], Gp[a:b], lam0))
            state.set_lambda(lam0)
            for e in range(n_epochs):
                Le = 0.0
                for eng, (a, b) in zip(engines, ranges):
                    rho = (tau0 + t) ** (-kappa)
                    Le += state.step(eng, alpha, eta, rho, float(n) / (b - a), doc_iter, THRESH, True, PLSA_FUSED)
                    eng.synchronize()
                    rhos.append(rho)
                    t += 1
                L.append(Le)
            gamma = np.zeros((n, k), np.float32)
            for eng, (a, b) in zip(engines, ranges):
                state.fold(eng, alpha, max(doc_iter, 1), THRESH, PLSA_FUSED)
                eng.synchronize()
                gamma[order[a:b]] = eng.get_factors(want_v=False)[0]
            lam = state.get_lambda()
            assert state.steps == n_blocks * n_epochs
        finally:
            for eng in engines:
                eng.close()
    return gamma, lam, L, rhos, ranges


@pytest.mark.gpu
@pytest.mark.parametrize("k", [6, 64])
def test_the_driver_is_the_step_iterated_and_steps_are_ordered(amd, k):
    X, _, _ = blocks_of(k)
    alpha, eta = PRIORS[1]
    gamma0, lam0 = le.start(k, alpha, eta)
    g_ref, l_ref, L_ref, rho_ref, ranges = hand_driven(amd, X, gamma0, lam0, alpha, eta, N_BLOCKS, 2, 3)
    kwargs = dict(doc_topic_prior=alpha, topic_word_prior=eta, init=(gamma0, lam0), n_batches=N_BLOCKS, n_epochs=2, doc_iter=3,
                  tolerance=0.0, shuffle_documents=False, e_step_thresh=THRESH, random_state=0)
    for attempt in range(2):
        gamma, lam, info = amd.lda_fit_online(X, k, return_info=True, **kwargs)
        same_bits(gamma, g_ref, "k=%d run %d: gamma" % (k, attempt))
        same_bits(lam, l_ref, "k=%d run %d: lambda" % (k, attempt))
        same_bits(np.array(info["bounds"]), np.array(L_ref), "k=%d run %d: L_e" % (k, attempt))
        assert info["rho"] == rho_ref == [(10.0 + t) ** -0.7 for t in range(2 * N_BLOCKS)]
        assert info["n_epochs"] == 2 and info["n_steps"] == 2 * N_BLOCKS and info["block_ranges"] == ranges
        assert info["permutation"] is None
        assert info["bytes_per_block_context"] == 3 * 4 * X.shape[1] * ((k + 3) // 4 * 4)
    # without the bounds no step waits for the device: the ordering between the block contexts is the event's alone
    for attempt in range(2):
        gamma, lam = amd.lda_fit_online(X, k, **kwargs)
        same_bits(gamma, g_ref, "k=%d enqueue-only run %d: gamma" % (k, attempt))
        same_bits(lam, l_ref, "k=%d enqueue-only run %d: lambda" % (k, attempt))
    assert not np.array_equal(l_ref, lam0)
    # shuffled: tuple factors draw nothing, so the permutation is the first draw of the seed; gamma in the caller's order
    perm = np.random.RandomState(5).permutation(X.shape[0])
    g_ref, l_ref, L_ref, _, _ = hand_driven(amd, X, gamma0, lam0, alpha, eta, N_BLOCKS, 2, 3, perm=perm)
    gamma, lam, info = amd.lda_fit_online(X, k, return_info=True, **dict(kwargs, shuffle_documents=True, random_state=5))
    np.testing.assert_array_equal(info["permutation"], perm)
    same_bits(gamma, g_ref, "shuffled: gamma in the caller's order")
    same_bits(lam, l_ref, "shuffled: lambda")
    same_bits(np.array(info["bounds"]), np.array(L_ref), "shuffled: L_e")


# ------------------------------------------------------------------------------------------------
# 7. refusals, and the state outlives its block contexts
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_launch_nothing_and_leave_state_and_block(amd):
    k = 21
    X, blocks, ranges = blocks_of(k)
    m = X.shape[1]
    alpha, eta = PRIORS[1]
    gamma0, lam0 = le.start(k, alpha, eta)
    lo, hi = ranges[0]
    own = other_topics(lam0)
    nan, inf = float("nan"), float("inf")
    with amd.Engine() as home, amd.LdaOnlineState(home, m, k) as state, block_engine(amd, blocks[0], gamma0[lo:hi], own) as eng:
        state.set_lambda(lam0)
        state.step(eng, alpha, eta, 0.5, 2.0, 2, THRESH, True, PLSA_FUSED)      # t = 1 and everything allocated, then the refusals
        gamma1 = eng.get_factors(want_u=True, want_v=False)[0]
        lam1 = state.get_lambda()
        eng.timing(True)
        eng.timing_reset()
        good = dict(alpha=alpha, eta=eta, rho=0.5, scale=2.0, doc_iter=1, flags=PLSA_FUSED)
        bad = [(dict(flags=0), "PLSA_FUSED"), (dict(flags=PLSA_FUSED | PLSA_SHARDED), "PLSA_SHARDED"),
               (dict(flags=PLSA_FUSED | PLSA_GRAPH), "PLSA_GRAPH"), (dict(flags=PLSA_FUSED | PLSA_REFERENCE_SUMS), "PLSA_REFERENCE_SUMS"),
               (dict(flags=PLSA_FUSED | PLSA_REFERENCE_LL), "PLSA_REFERENCE_LL"),
               (dict(alpha=0.0), "alpha="), (dict(alpha=-0.1), "alpha="), (dict(alpha=nan), "alpha="), (dict(alpha=inf), "alpha="),
               (dict(eta=0.0), "eta="), (dict(eta=-1.0), "eta="), (dict(eta=nan), "eta="), (dict(eta=inf), "eta="),
               (dict(doc_iter=0), "doc_iter"), (dict(doc_iter=-2), "doc_iter"),
               (dict(rho=0.0), "rho"), (dict(rho=-0.5), "rho"), (dict(rho=1.0000001), "rho"), (dict(rho=nan), "rho"),
               (dict(rho=inf), "rho"), (dict(scale=0.0), "scale"), (dict(scale=-1.0), "scale"), (dict(scale=nan), "scale"),
               (dict(scale=inf), "scale")]
        for change, word in bad:
            a = dict(good, **change)
            with pytest.raises(amd.DeviceError, match=word):
                state.step(eng, a["alpha"], a["eta"], a["rho"], a["scale"], a["doc_iter"], THRESH, True, a["flags"])
        for flags, word in ((0, "PLSA_FUSED"), (PLSA_FUSED | PLSA_SHARDED, "PLSA_SHARDED"), (PLSA_FUSED | PLSA_GRAPH, "PLSA_GRAPH")):
            with pytest.raises(amd.DeviceError, match=word):
                state.fold(eng, alpha, 1, THRESH, flags)
        for bad_alpha in (0.0, -1.0, nan, inf):
            with pytest.raises(amd.DeviceError, match="alpha="):
                state.fold(eng, bad_alpha, 1, THRESH, PLSA_FUSED)
        with pytest.raises(amd.DeviceError, match="n_rounds"):
            state.fold(eng, alpha, -1, THRESH, PLSA_FUSED)
        for arithmetic in ("reference", "reference_source"):
            eng.set_arithmetic(arithmetic)
            with pytest.raises(amd.DeviceError, match="reference arithmetic"):
                state.step(eng, alpha, eta, 0.5, 2.0, 1, THRESH, flags=PLSA_FUSED)
            with pytest.raises(amd.DeviceError, match="reference arithmetic"):
                state.fold(eng, alpha, 1, THRESH, PLSA_FUSED)
        eng.set_arithmetic(None)
        with amd.LdaOnlineState(home, m + 4, k) as wider, amd.LdaOnlineState(home, m, k + 1) as deeper, \
                amd.LdaOnlineState(home, m, k + 3) as padded:
            assert (padded.k + 3) // 4 == (k + 3) // 4          # the same kp, another k
            for other in (wider, deeper, padded):
                other.set_lambda(np.full((other.k, other.m), 0.5, np.float32))
                with pytest.raises(amd.DeviceError, match="words with k="):
                    other.step(eng, alpha, eta, 0.5, 2.0, 1, THRESH, flags=PLSA_FUSED)
                with pytest.raises(amd.DeviceError, match="words with k="):
                    other.fold(eng, alpha, 1, THRESH, PLSA_FUSED)
                assert other.steps == 0
        with amd.Engine() as bare:                                        # a context without corpus or factors
            with pytest.raises(amd.DeviceError):
                state.step(bare, alpha, eta, 0.5, 2.0, 1, THRESH, flags=PLSA_FUSED)
            with pytest.raises(amd.DeviceError):
                state.fold(bare, alpha, 1, THRESH, PLSA_FUSED)
        # (a block context on another device than the state is refused by the same chain; the suite runs on one GPU)
        assert eng.timing_report() == {}, eng.timing_report()             # nothing was launched
        eng.timing(False)
        gamma2, own2 = eng.get_factors()
        same_bits(gamma2, gamma1, "a refusal moved the block's gamma")
        same_bits(own2, own, "a refusal moved the block's topic table")
        same_bits(state.get_lambda(), lam1, "a refusal moved lambda")
        assert state.steps == 1
        for bad_table in (lam0[:, :-1], lam0[:-1]):
            with pytest.raises(ValueError, match="shape"):
                state.set_lambda(bad_table)


@pytest.mark.gpu
def test_a_shard_of_a_communicator_is_refused(amd, tmp_path):
    from enstop_amd import comm
    k = 21
    X, blocks, ranges = blocks_of(k)
    alpha, eta = PRIORS[1]
    gamma0, lam0 = le.start(k, alpha, eta)
    lo, hi = ranges[0]
    with amd.Engine() as home, amd.LdaOnlineState(home, X.shape[1], k) as state, \
            block_engine(amd, blocks[0], gamma0[lo:hi], lam0) as eng:
        state.set_lambda(lam0)
        c = comm.RcclComm(eng, 0, 1, comm.rendezvous_id(0, str(tmp_path / "rccl.id")))
        try:
            eng.timing(True)
            eng.timing_reset()
            with pytest.raises(amd.DeviceError, match="communicator"):
                state.step(eng, alpha, eta, 0.5, 2.0, 1, THRESH, flags=PLSA_FUSED)
            with pytest.raises(amd.DeviceError, match="communicator"):
                state.fold(eng, alpha, 1, THRESH, PLSA_FUSED)
            assert eng.timing_report() == {}, eng.timing_report()
            same_bits(eng.get_factors(want_v=False)[0], gamma0[lo:hi], "a refusal moved gamma")
        finally:
            c.close()
        state.step(eng, alpha, eta, 0.5, 2.0, 1, THRESH, flags=PLSA_FUSED)
        assert state.steps == 1 and "k_lda_online_blend" in eng.timing_report()


def test_the_python_refusals_come_before_any_engine(monkeypatch):
    import enstop_amd
    from enstop_amd import engine, lda, lda_online, online, plsa

    def no_engine(*args, **kwargs):
        raise AssertionError("an engine was asked for")
    for module in (engine, lda, lda_online, online, plsa):
        monkeypatch.setattr(module, "get_engine", no_engine)
    monkeypatch.setattr(lda_online, "Engine", no_engine)
    X = sp.random(12, 9, density=0.5, format="csr", random_state=0, dtype=np.float32)
    nan = float("nan")
    for kw in (dict(doc_topic_prior=0.0), dict(doc_topic_prior=-0.1), dict(doc_topic_prior=nan), dict(topic_word_prior=float("inf")),
               dict(doc_topic_prior="asymmetric"), dict(doc_topic_prior="auto"), dict(topic_word_prior="auto"),
               dict(doc_topic_prior=[0.1, 0.2, 0.3]), dict(doc_topic_prior=np.full(3, 0.1)), dict(topic_word_prior=[0.1] * 3),
               dict(doc_topic_prior="sparse"), dict(topic_word_prior=True), dict(doc_iter=0), dict(doc_iter=1.5),
               dict(n_batches=0), dict(n_batches=257), dict(n_epochs=-1), dict(tolerance=-1.0), dict(rho=1.5), dict(rho=0.0),
               dict(tau0=0.5), dict(kappa=-1.0)):
        with pytest.raises(ValueError):
            enstop_amd.lda_fit_online(X, 3, **kw)
        with pytest.raises(ValueError):
            enstop_amd.OnlineLDA(n_components=3, **kw).fit(X)
        if not set(kw) & {"n_batches", "n_epochs", "tolerance"}:          # (those do not enter partial_fit)
            with pytest.raises(ValueError):
                enstop_amd.OnlineLDA(n_components=3, **kw).partial_fit(X)
    for kw in (dict(init="nndsvd"), dict(init=(np.ones((12, 3)), np.ones((3, 8)))), dict(init=(np.zeros((12, 3)), np.ones((3, 9))))):
        with pytest.raises(ValueError):
            enstop_amd.lda_fit_online(X, 3, **kw)
    for k in (0, 1025, 2.5):
        with pytest.raises(ValueError):
            enstop_amd.lda_fit_online(X, k)
    with pytest.raises(ValueError):
        enstop_amd.lda_fit_online(-X, 3)
    for total in (0, -5.0, nan, float("inf"), True):
        with pytest.raises(ValueError, match="total_samples"):
            enstop_amd.OnlineLDA(n_components=3, total_samples=total).partial_fit(X)


@pytest.mark.gpu
def test_the_state_survives_release_scratch_and_the_destruction_of_a_block_context(amd):
    k = 64
    X, blocks, ranges = blocks_of(k)
    m = X.shape[1]
    alpha, eta = PRIORS[1]
    gamma0, lam0 = le.start(k, alpha, eta)
    steps = ((0, 0.5), (1, 0.4), (0, 0.3))

    def run(disturb):
        with amd.Engine() as home, amd.LdaOnlineState(home, m, k) as state:
            state.set_lambda(lam0)
            last = None
            for b, rho in steps:
                lo, hi = ranges[b]
                eng = block_engine(amd, blocks[b], gamma0[lo:hi], other_topics(lam0))
                state.step(eng, alpha, eta, rho, 3.0, 1, THRESH, flags=PLSA_FUSED)
                if disturb:
                    eng.release_scratch()                                 # the block's side tables go; the state's stay
                state.fold(eng, alpha, 1, THRESH, PLSA_FUSED)
                if not disturb:
                    eng.synchronize()
                last = eng.get_factors(want_v=False)[0]
                eng.close()                                               # (disturb: destroyed with the fold just enqueued)
            return state.get_lambda(), last, state.steps

    quiet, disturbed = run(False), run(True)
    same_bits(disturbed[0], quiet[0], "lambda after release_scratch / destroy of the block contexts")
    same_bits(disturbed[1], quiet[1], "gamma of the last fold")
    assert quiet[2] == disturbed[2] == 3 and np.isfinite(quiet[0]).all() and (quiet[0] > 0).all()


# ------------------------------------------------------------------------------------------------
# 8. partial_fit
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [6, 64])
def test_partial_fit_is_three_hand_driven_steps(amd, k):
    X, blocks, ranges = blocks_of(k)
    n, m = X.shape
    seed, doc_iter, total = 11, 2, 5000.0
    alpha, eta = 0.2, 0.05
    est = amd.OnlineLDA(n_components=k, doc_topic_prior=alpha, topic_word_prior=eta, doc_iter=doc_iter, random_state=seed,
                        total_samples=total)
    rng = np.random.RandomState(seed)
    lam = rng.gamma(100.0, 0.01, (k, m)).astype(np.float32)
    with amd.Engine() as eng, amd.LdaOnlineState(eng, m, k) as state:
        state.set_lambda(lam)
        for t, (Xb, (a, b)) in enumerate(zip(blocks, ranges)):
            assert est.partial_fit(Xb) is est
            gamma0 = rng.gamma(100.0, 0.01, (b - a, k)).astype(np.float32)
            eng.upload_csr(Xb)
            eng.set_factors(gamma0, lam)
            state.step(eng, alpha, eta, (10.0 + t) ** -0.7, total / (b - a), doc_iter, THRESH, flags=PLSA_FUSED)
            lam = state.get_lambda()
            gamma = eng.get_factors(want_v=False)[0]
            same_bits(est.components_, lam, "k=%d call %d: components_" % (k, t))
            same_bits(est.embedding_, gamma / gamma.sum(axis=1, keepdims=True), "k=%d call %d: embedding_" % (k, t))
            same_bits(est.topic_word_, lam / lam.sum(axis=1, keepdims=True), "k=%d call %d: topic_word_" % (k, t))
            assert est.n_steps_ == t + 1 == state.steps
    assert (est.components_ > 0).all() and est.topic_word_prior_ == eta and (est.doc_topic_prior_ == alpha).all()
    T = est.transform(X[:50])                                             # LDA's fold-in against components_
    assert T.shape == (50, k) and (T > 0).all()
    np.testing.assert_allclose(T.astype(np.float64).sum(axis=1), 1.0, rtol=1e-5)
    with pytest.raises(ValueError, match="words"):
        est.partial_fit(sp.csr_matrix(X[:10, :m - 1]))
    assert est.n_steps_ == N_BLOCKS
    # a pickled copy carries the model, not the device handles: it starts afresh
    copy = pickle.loads(pickle.dumps(est))
    assert "_partial" not in copy.__dict__ and "_partial" in est.__dict__
    same_bits(copy.components_, est.components_, "the copy's components_")
    fresh = amd.OnlineLDA(n_components=k, doc_topic_prior=alpha, topic_word_prior=eta, doc_iter=doc_iter, random_state=seed,
                          total_samples=total).partial_fit(blocks[0])
    copy.partial_fit(blocks[0])
    assert copy.n_steps_ == 1
    same_bits(copy.components_, fresh.components_, "a pickled copy starts afresh")


@pytest.mark.gpu
def test_the_estimator_fits_through_lda_fit_online(amd):
    k = 21
    X, _, _ = blocks_of(k)
    params = dict(doc_topic_prior=0.1, topic_word_prior=0.05, n_batches=N_BLOCKS, n_epochs=2, doc_iter=2, tolerance=0.0, random_state=3)
    est = amd.OnlineLDA(n_components=k, **params)
    E = est.fit_transform(X)
    gamma, lam, info = amd.lda_fit_online(X, k, return_info=True, **params)
    same_bits(est.components_, lam, "components_")
    same_bits(E, gamma / gamma.sum(axis=1, keepdims=True), "embedding_")
    assert est.n_iter_ == 2 and est.n_steps_ == 2 * N_BLOCKS and est.online_info_["rho"] == info["rho"]
    assert list(est.bound_trace_) == info["bounds"] and est.bound_ == info["bounds"][-1]
    assert np.isfinite(est.perplexity(X[:100])) and np.isfinite(est.score(X[:100]))


# ------------------------------------------------------------------------------------------------
# 9. end to end on the planted corpus
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_end_to_end_on_the_planted_corpus(amd):
    observed, held, scored, gamma0, lam0 = M.the_split()
    model = M.model()
    f = M.FIT
    gamma, lam, info = amd.lda_fit_online(observed, f["k"], f["alpha"], f["eta"], init=(gamma0, lam0), n_batches=f["n_batches"],
                                          n_epochs=M.EPOCHS, doc_iter=f["doc_iter"], kappa=f["kappa"], tau0=f["tau0"], tolerance=0.0,
                                          shuffle_documents=True, random_state=f["random_state"], return_info=True)
    np.testing.assert_array_equal(info["permutation"], model["perm"])
    assert info["n_epochs"] == M.EPOCHS and info["n_steps"] == M.EPOCHS * f["n_batches"]
    online = M.perplexity(held, scored, gamma, lam)
    gb, lb, binfo = amd.lda_fit(observed, f["k"], f["alpha"], f["eta"], init=(gamma0, lam0), n_iter=f["batch_iterations"],
                                tolerance=0.0, return_info=True)
    assert binfo["n_iter"] == f["batch_iterations"]
    batch = M.perplexity(held, scored, gb, lb)
    want = model["online_perplexity"][M.EPOCHS - 1]
    L_dev, L_model = np.array(info["bounds"]), np.array(model["L"][:M.EPOCHS])
    gap_l = float(np.max(np.abs(L_dev - L_model) / np.abs(L_model)))
    gap_p = abs(online - want) / want
    gap_b = abs(batch - M.batch_perplexity()) / M.batch_perplexity()
    print("\nheld-out perplexity after %d epochs: device %.4f, model %.4f; batch LDA after %d iterations: device %.4f, model %.4f"
          % (M.EPOCHS, online, want, f["batch_iterations"], batch, M.batch_perplexity()))
    print("largest relative gap device / float64 model: L_e %.3e, perplexity %.3e (batch LDA's perplexity %.3e)"
          % (gap_l, gap_p, gap_b))
    print("L_e device %r model %r" % (L_dev.tolist(), L_model.tolist()))
    assert online <= batch, (online, batch)
    assert 10 * GAP_L < 1e-3 and 10 * GAP_P < 1e-3
    assert gap_l <= 10 * GAP_L, gap_l
    assert gap_p <= 10 * GAP_P, gap_p
