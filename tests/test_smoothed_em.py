"""Smoothed (MAP) EM on the device (include/plsa_hip_diag.h: plsa_fit_smoothed, plsa_refit_smoothed, plsa_log_posterior;
enstop_amd/smoothed.py) against the float64 model of tests/smoothed_model.py.

    P(z|d) = (n_dz + a) / (N_d + k a)        P(w|z) = (n_wz + b) / (N_z + m b)
    F = sum sw_d x_dw log sum_z P(w|z) P(z|d)  +  a sum_d sw_d sum_z log P(z|d)  +  b sum_z sum_w log P(w|z)

Kernel-level tests run on matrix_corpus(k) of test_pass_matrix.py (640 x 480, about 4 000 non-zeros: two empty documents, the
300-word document of the row-item path, the heavy word, stored zeros) with its weights in (0.5, 1.5), for
k in {3, 6, 21, 64, 130, 1024}: kq = 1, padding topics, the 8 x 2 document shape, rows that straddle workgroups raggedly
(kq = 33), rows that are whole workgroups (kq = 256).  (a, b) runs over {(0.5, 0), (0, 0.05), (0.5, 0.05), (1e-3, 1e-6)}.

Error model (u = 2^-24; s = 4 (L + k) u is the bound of a plain step's entry and of its norm, test_pass_matrix.py's docstring).
  P(z|d): the device forms fmaf(u_z, N_d, a) / (N_d + ka) from the pass's u_z (error s) and N_d (error s).  u_z N_d carries
    s + s, adding a >= 0 does not raise a relative error, the denominator carries s once more, and there are four roundings
    (the fused multiply-add, (float)(k a) and the sum, the division): 3 s + 4 u.
  P(w|z): (Vacc + b) / (float)(N_z + m b): the entry's s, the norm's s, four roundings (the sum, (float)b, the conversion of
    the denominator, the division): 2 s + 4 u.
  A side whose pseudo-count is 0 is the plain step and is held to s -- and to the plain step's bits.
  Row sums: sum_z (u_z N_d + a) against N_d + ka.  N_d is a float32 sum of the k numerators in some order, (k - 1) u from
    their exact sum; every entry carries four roundings (the pass's division, the multiply-add, the denominator's sum, the
    division) and k (float)a differs from (float)(k a) by one more: (k + 4) u to first order, asserted as (k + 5) u.
  Topic sums: sum_w (Vacc + b) against (float)(N_z + m b).  N_z adds float32 strand sums of at most ceil(m / 256) entries in
    float64 and is rounded once: ceil(m / 256) u; every entry carries two roundings, the denominator's conversion one,
    m (float)b against m b one: (ceil(m / 256) + 4) u to first order, asserted as (ceil(m / 256) + 5) u.
  F: check_ll's bound for the likelihood plus 2^-50 sum |prior terms| for the float64 prior sums.

The pad columns k .. kp of the two tables cannot be read through the ABI (its host tables are [n, k] and [k, m]).  The kernels
write 0 there by the plan's mask, which tests/test_smoothed_plan_host.py checks for every float4; here every following step is
held to the model, which never sees a pad.

The communicator refusal runs on a one-rank RCCL communicator (all a single GPU can host), created on a private engine the
way tests/test_hip_parity.py creates one.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import smoothed_model as sm
from test_capped_grids import CAP, knobs as cap_knobs, sizes
from test_fit_driver import PLSA_FUSED, PLSA_GRAPH, PLSA_SHARDED, make_engine, same_bits
from test_pass_matrix import C_FACTOR, EMPTY_DOCS, U32, check, matrix_corpus, step64

PLSA_REFERENCE_SUMS, PLSA_REFERENCE_LL = 256, 512
THRESH = 1e-32
K = [3, 6, 21, 64, 130, 1024]
AB = [(0.5, 0.0), (0.0, 0.05), (0.5, 0.05), (1e-3, 1e-6)]
ONE = dict(n_iter=1, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED)


@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


@pytest.fixture(scope="module")
def worst():
    out = {}
    yield out
    for k in sorted(out):
        print("\nsmoothed EM k=%d: worst error / bound: " % k + ", ".join("%s %.3g" % kv for kv in sorted(out[k].items())))


@functools.lru_cache(maxsize=None)
def plain_step(k):
    """step64 of matrix_corpus(k) with its weights, computed once"""
    X, U0, V0, sw = matrix_corpus(k)
    return step64(X, U0, V0, THRESH, sw)


def bounds(s, k, a, b):
    """(bound of P(z|d), bound of P(w|z)) for one step with the pseudo-counts a, b"""
    s_row, s_col = C_FACTOR * (s["L_row"] + k) * U32, C_FACTOR * (s["L_col"] + k) * U32
    return (3 * s_row + 4 * U32 if a > 0 else s_row), (2 * s_col + 4 * U32 if b > 0 else s_col)


def check_step(tag, U1, V1, want, k, a, b, ratios, topics=True):
    b_u, b_v = bounds(want, k, a, b)
    check("P(z|d) " + tag, U1, want["U"], b_u, ratios)
    if topics:
        check("P(w|z) " + tag, V1, want["V"], b_v, ratios)
    m = V1.shape[1]
    if a > 0:
        rows = np.abs(U1.astype(np.float64).sum(1) - 1.0)
        assert rows.max() <= (k + 5) * U32, (tag, rows.max() / U32)
        assert np.isfinite(U1).all() and (U1 > 0).all(), tag
    if b > 0 and topics:
        cols = np.abs(V1.astype(np.float64).sum(1) - 1.0)
        assert cols.max() <= (-(-m // 256) + 5) * U32, (tag, cols.max() / U32)
        assert (V1 > 0).all(), tag


# ------------------------------------------------------------------------------------------------
# 4. one step, entry by entry
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_one_step_against_the_model(amd, worst, k):
    X, U0, V0, sw = matrix_corpus(k)
    plain = plain_step(k)
    ratios = worst.setdefault(k, {})
    with make_engine(amd, {}, X) as eng:
        eng.timing(True)
        for a, b in AB:
            want = sm.smooth_step(plain, V0, a, b)
            eng.set_factors(U0, V0)
            eng.timing_reset()
            iters, trace = eng.fit_smoothed(a, b, sw, trace=True, **ONE)
            names = eng.timing_report()
            U1, V1 = eng.get_factors()
            tag = "a=%g b=%g" % (a, b)
            assert iters == 1 and len(trace) == 2, tag
            check_step(tag, U1, V1, want, k, a, b, ratios)
            # which kernels ran: the new ones only on the side that is smoothed, the plain tail on the other
            assert ("k_smooth_rows" in names) == (a > 0) and ("k_smooth_topics" in names) == (b > 0), (tag, sorted(names))
            assert ("k_col_reduce_norm" in names) == (b == 0) and ("k_col_reduce" in names) == (b > 0), (tag, sorted(names))
            assert names["k_log_prior"][0] == 2 * ((a > 0) + (b > 0)), (tag, names)
            if a > 0:                                                       # an empty document gets the prior mean
                for d in EMPTY_DOCS:
                    check("empty document " + tag, U1[d], np.full(k, 1.0 / k), bounds(plain, k, a, b)[0], ratios)
            # the trace is F before and after the step
            for slot, (U, V) in enumerate(((U0, V0), (U1, V1))):
                f, ll_scale, prior_scale = sm.objective64(X, U, V, a, b, sw)
                err = abs(float(trace[slot]) - f)
                assert err <= C_FACTOR * (k + 1) * U32 * ll_scale + 2.0 ** -50 * prior_scale + abs(f) * U32, (tag, slot, trace[slot], f)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [6, 130])
def test_one_step_through_the_row_items(amd, worst, k):
    """documents cut into row items of 16 entries (the 300-word document makes 19): N_d comes from k_row_reduce"""
    X, U0, V0, sw = matrix_corpus(k)
    a, b = 0.5, 0.05
    want = sm.smooth_step(plain_step(k), V0, a, b)
    with make_engine(amd, {"PLSA_ROW_ITEMS": "1", "PLSA_ROW_SEG": "16"}, X) as eng:
        eng.timing(True)
        eng.set_factors(U0, V0)
        eng.timing_reset()
        eng.fit_smoothed(a, b, sw, **ONE)
        assert "k_row_reduce" in eng.timing_report()
        U1, V1 = eng.get_factors()
        check_step("row items", U1, V1, want, k, a, b, worst.setdefault(k, {}))


# ------------------------------------------------------------------------------------------------
# 5. bits
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_zero_pseudo_counts_keep_the_plain_bits(amd, k):
    X, U0, V0, sw = matrix_corpus(k)
    loop = dict(n_iter=5, n_iter_per_test=2, tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED, trace=True)
    with make_engine(amd, {}, X) as eng:
        eng.set_factors(U0, V0)
        it_p, tr_p = eng.fit(sw, **loop)
        Up, Vp = eng.get_factors()
        eng.set_factors(U0, V0)
        it_s, tr_s = eng.fit_smoothed(0.0, 0.0, sw, **loop)
        Us, Vs = eng.get_factors()
        assert it_p == it_s == 5
        same_bits(tr_p, tr_s, "trace at a = b = 0")
        same_bits(Up, Us, "P(z|d) at a = b = 0")
        same_bits(Vp, Vs, "P(w|z) at a = b = 0")
        # one plain step, then each side alone
        eng.set_factors(U0, V0)
        eng.fit(sw, **ONE)
        U1, V1 = eng.get_factors()
        eng.set_factors(U0, V0)
        eng.fit_smoothed(0.5, 0.0, sw, **ONE)
        Ua, Va = eng.get_factors()
        same_bits(Va, V1, "P(w|z) with b = 0")
        assert (Ua != U1).any()
        eng.set_factors(U0, V0)
        eng.fit_smoothed(0.0, 0.05, sw, **ONE)
        Ub, Vb = eng.get_factors()
        same_bits(Ub, U1, "P(z|d) with a = 0")
        assert (Vb != V1).any()
        # the refit at a = 0 is the refit
        eng.set_factors(U0, V0)
        eng.refit(sw, **ONE)
        Ur, _ = eng.get_factors()
        eng.set_factors(U0, V0)
        eng.refit_smoothed(0.0, sw, **ONE)
        same_bits(eng.get_factors()[0], Ur, "refit at a = 0")


# ------------------------------------------------------------------------------------------------
# 6. the objective
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_log_posterior(amd, worst, k):
    X, U0, V0, sw = matrix_corpus(k)
    ratios = worst.setdefault(k, {})
    with make_engine(amd, {}, X) as eng:
        eng.set_factors(U0, V0)
        for weights in (None, sw):
            ll = eng.log_likelihood(weights)
            f0 = eng.log_posterior(weights, 0.0, 0.0)
            assert np.float64(ll).view(np.uint64) == np.float64(f0).view(np.uint64), (ll, f0)
            for a, b in AB:
                f, ll_scale, prior_scale = sm.objective64(X, U0, V0, a, b, weights)
                got = eng.log_posterior(weights, a, b)
                bound = C_FACTOR * (k + 1) * U32 * ll_scale + 2.0 ** -50 * prior_scale
                assert abs(got - f) <= bound, (a, b, got, f, bound)
                ratios["F"] = max(ratios.get("F", 0.0), abs(got - f) / bound)
        # an entry equal to 0 adds nothing
        Uz = U0.copy()
        Uz[5, 0] = 0.0
        eng.set_factors(Uz, V0)
        f, ll_scale, prior_scale = sm.objective64(X, Uz, V0, 0.5, 0.05, sw)
        got = eng.log_posterior(sw, 0.5, 0.05)
        assert np.isfinite(got) and abs(got - f) <= C_FACTOR * (k + 1) * U32 * ll_scale + 2.0 ** -50 * prior_scale


@pytest.mark.gpu
def test_the_prior_does_not_depend_on_the_launch_geometry(amd):
    """A corpus whose stored values are all 0 has a log-likelihood of exactly 0, so F IS the prior part: a context capped at one
    workgroup per CU and a free one agree on it bit for bit (k = 1024: 163 840 and 122 880 float4s, more than a capped grid
    of 256 workgroups holds in one trip), and both are the model's within 2^-50 sum |terms|."""
    k = 1024
    X, U0, V0, sw = matrix_corpus(k)
    X0 = sp.csr_matrix((np.zeros_like(X.data), X.indices, X.indptr), shape=X.shape)
    got = {}
    for capped in (True, False):
        with cap_knobs(CAP if capped else {}):
            eng = amd.Engine()
        with eng:
            eng.upload_csr(X0)
            eng.set_factors(U0, V0)
            assert eng.log_likelihood(sw) == 0.0
            got[capped] = [eng.log_posterior(sw, a, b) for a, b in AB]
    for (a, b), f_capped, f_free in zip(AB, got[True], got[False]):
        assert np.float64(f_capped).view(np.uint64) == np.float64(f_free).view(np.uint64), (a, b, f_capped, f_free)
        prior, scale = sm.log_prior64(U0, V0, a, b, sw)
        assert abs(f_free - prior) <= 2.0 ** -50 * scale, (a, b, f_free, prior)


# ------------------------------------------------------------------------------------------------
# 7. the refit
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_one_refit_step_against_the_model(amd, worst, k):
    X, U0, V0, sw = matrix_corpus(k)
    plain = plain_step(k)
    ratios = worst.setdefault(k, {})
    with make_engine(amd, {}, X) as eng:
        eng.timing(True)
        for a in (0.5, 1e-3):
            want = sm.smooth_step(plain, V0, a, 0.0, update_v=False)
            eng.set_factors(U0, V0)
            eng.timing_reset()
            iters, trace = eng.refit_smoothed(a, sw, trace=True, **ONE)
            names = eng.timing_report()
            U1, V1 = eng.get_factors()
            assert iters == 1 and len(trace) == 2
            check_step("refit a=%g" % a, U1, V1, want, k, a, 0.0, ratios, topics=False)
            same_bits(V1, V0, "the refit wrote the topics")
            assert "k_smooth_rows" in names and not [name for name in names if name.startswith("k_col")], sorted(names)
            f, ll_scale, prior_scale = sm.objective64(X, U1, V0, a, 0.0, sw)
            assert abs(float(trace[1]) - f) <= C_FACTOR * (k + 1) * U32 * ll_scale + 2.0 ** -50 * prior_scale + abs(f) * U32


# ------------------------------------------------------------------------------------------------
# 8. the loop, one iteration at a time
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [6, 130])
def test_the_loop_is_the_step_iterated(amd, worst, k):
    """three n_iter = 1 calls, each held to the model started from the device's previous factors (so the per-step bound
    applies), then one call of three iterations from the same start: the same bits, and a trace that is F of every stage"""
    X, U0, V0, sw = matrix_corpus(k)
    a, b = 0.5, 0.05
    ratios = worst.setdefault(k, {})
    with make_engine(amd, {}, X) as eng:
        eng.set_factors(U0, V0)
        U, V, stages = U0, V0, []
        for step in range(3):
            want = sm.smoothed_step64(X, U, V, THRESH, a, b, sw)
            iters, trace = eng.fit_smoothed(a, b, sw, trace=True, **ONE)
            U, V = eng.get_factors()
            check_step("loop step %d" % step, U, V, want, k, a, b, ratios)
            stages.append(trace)
        eng.set_factors(U0, V0)
        iters, trace = eng.fit_smoothed(a, b, sw, n_iter=3, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH,
                                        flags=PLSA_FUSED, trace=True)
        U3, V3 = eng.get_factors()
        assert iters == 3 and len(trace) == 4
        same_bits(U3, U, "three iterations: P(z|d)")
        same_bits(V3, V, "three iterations: P(w|z)")
        same_bits(trace, np.array([stages[0][0], stages[0][1], stages[1][1], stages[2][1]], np.float32), "trace")
        # a test every second iteration: the likelihood after iterations 0 and 2 only, the last one because it is traced
        eng.set_factors(U0, V0)
        iters, sparse = eng.fit_smoothed(a, b, sw, n_iter=3, n_iter_per_test=2, tolerance=0.0, e_step_thresh=THRESH,
                                         flags=PLSA_FUSED, trace=True)
        assert iters == 3
        same_bits(sparse, trace[[0, 1, 3]], "trace with a test every second iteration")
        same_bits(eng.get_factors()[0], U, "a test every second iteration: P(z|d)")


# ------------------------------------------------------------------------------------------------
# 9. the objective never decreases
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_monotone_objective(amd):
    """Planted corpus of tests/smoothed_model.py (seed 3), a = 0.1, b = 0.01, positive random start, weights in (0.5, 1.5),
    tolerance 0, a test after every one of 30 iterations: every value of the trace is at least its predecessor minus
    check_ll's bound.  The float64 model (test_smoothed_model_host.py): F rises from -159 941.6 to -118 795.8, its smallest
    increase is 13.04 against a bound of 0.340 -- a margin of 38."""
    X, _, sw, U0, V0 = sm.planted()
    F, scales = sm.planted_trace()
    k = sm.PLANTED["topics"]
    bound = C_FACTOR * (k + 1) * U32 * scales.max()
    assert np.diff(F).min() >= 10 * bound
    with make_engine(amd, {}, X) as eng:
        eng.set_factors(U0, V0)
        iters, trace = eng.fit_smoothed(0.1, 0.01, sw, n_iter=30, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH,
                                        flags=PLSA_FUSED, trace=True)
    assert iters == 30 and len(trace) == 31
    trace = trace.astype(np.float64)
    print("\nplanted corpus on the device: F %.1f -> %.1f, smallest increase %.3f (model %.3f), bound %.3f"
          % (trace[0], trace[-1], np.diff(trace).min(), np.diff(F).min(), bound))
    assert (np.diff(trace) >= -bound).all(), np.diff(trace).min()
    assert abs(trace[0] - F[0]) <= bound + abs(F[0]) * U32


# ------------------------------------------------------------------------------------------------
# 10. what it is for
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_smoothed_model_scores_unseen_words(amd):
    X, X_test, _, _, _ = sm.planted()
    unseen = np.setdiff1d(np.unique(X_test.indices), np.unique(X.indices))
    assert unseen.size > 0
    plain = amd.PLSA(n_components=8, random_state=0).fit(X)
    scores = amd.held_out_scores(X_test, plain.components_, method="completion")
    assert scores["unscored"].sum() > 0                  # the precondition: words absent from training have no probability
    assert plain.perplexity(X_test) == np.inf
    model = amd.PLSA(n_components=8, random_state=0, doc_topic_smoothing=0.1, topic_word_smoothing=0.01).fit(X)
    assert model.components_.min() > 0 and model.embedding_.min() > 0
    scores = amd.held_out_scores(X_test, model.components_, method="completion", doc_topic_smoothing=0.1)
    assert scores["unscored"].sum() == 0
    p = model.perplexity(X_test)
    assert np.isfinite(p) and p > 1
    print("\nplanted corpus: held-out perplexity of the smoothed model %.1f (on_zero='inf'); the unsmoothed model leaves %g "
          "tokens unscored" % (p, amd.held_out_scores(X_test, plain.components_)["unscored"].sum()))
    # the fold-in of a smoothed model is the smoothed refit: strictly positive document vectors, rows that sum to 1
    T = model.transform(X_test)
    assert T.shape == (X_test.shape[0], 8) and (T > 0).all() and np.abs(T.astype(np.float64).sum(1) - 1).max() <= 13 * U32
    assert np.isfinite(model.score_samples(X_test)).all()
    # the functions
    U, V, info = amd.plsa_fit_smoothed(X, 8, None, 0.1, 0.01, n_iter=20, random_state=0, return_info=True)
    assert (U > 0).all() and (V > 0).all() and len(info["log_posterior_trace"]) >= 2
    assert (np.diff(info["log_posterior_trace"].astype(np.float64)) > 0).all()
    R = amd.plsa_refit_smoothed(X_test, V, None, 0.1, random_state=1)
    assert R.shape == (X_test.shape[0], 8) and (R > 0).all()


# ------------------------------------------------------------------------------------------------
# 11. refusals
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_launch_nothing_and_leave_the_factors(amd):
    k = 21
    X, U0, V0, sw = matrix_corpus(k)
    kw = dict(n_iter=2, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH)
    nan, inf = float("nan"), float("inf")
    with make_engine(amd, {}, X) as eng:
        eng.set_factors(U0, V0)
        eng.timing(True)
        eng.timing_reset()
        bad = [(0.5, 0.05, 0, "PLSA_FUSED"), (0.0, 0.0, 0, "PLSA_FUSED"), (0.5, 0.05, PLSA_FUSED | PLSA_SHARDED, "PLSA_SHARDED"),
               (0.5, 0.05, PLSA_FUSED | PLSA_GRAPH, "PLSA_GRAPH"), (0.0, 0.0, PLSA_FUSED | PLSA_GRAPH, "PLSA_GRAPH"),
               (0.5, 0.05, PLSA_FUSED | PLSA_REFERENCE_SUMS, "PLSA_REFERENCE_SUMS"),
               (0.5, 0.05, PLSA_FUSED | PLSA_REFERENCE_LL, "PLSA_REFERENCE_LL"),
               (-1e-9, 0.05, PLSA_FUSED, "a="), (nan, 0.05, PLSA_FUSED, "a="), (inf, 0.0, PLSA_FUSED, "a="),
               (0.5, -1.0, PLSA_FUSED, "b="), (0.5, nan, PLSA_FUSED, "b="), (0.0, inf, PLSA_FUSED, "b=")]
        for a, b, flags, word in bad:
            with pytest.raises(amd.DeviceError, match=word):
                eng.fit_smoothed(a, b, sw, flags=flags, **kw)
            if word != "b=":
                with pytest.raises(amd.DeviceError, match=word):
                    eng.refit_smoothed(a, sw, flags=flags, **kw)
            if flags == PLSA_FUSED:
                with pytest.raises(amd.DeviceError, match=word):
                    eng.log_posterior(sw, a, b)
        for arithmetic in ("reference", "reference_source"):
            eng.set_arithmetic(arithmetic)
            for a, b in ((0.5, 0.05), (0.0, 0.0)):
                with pytest.raises(amd.DeviceError, match="reference arithmetic"):
                    eng.fit_smoothed(a, b, sw, flags=PLSA_FUSED, **kw)
                with pytest.raises(amd.DeviceError, match="reference arithmetic"):
                    eng.refit_smoothed(a, sw, flags=PLSA_FUSED, **kw)
                with pytest.raises(amd.DeviceError, match="reference arithmetic"):
                    eng.log_posterior(sw, a, b)
        eng.set_arithmetic(None)
        assert eng.timing_report() == {}, eng.timing_report()        # nothing was launched
        U, V = eng.get_factors()
        same_bits(U, U0, "a refusal moved U")
        same_bits(V, V0, "a refusal moved V")
        iters, _ = eng.fit_smoothed(0.5, 0.05, sw, flags=PLSA_FUSED, **kw)
        names = eng.timing_report()
        assert iters == 2 and names["k_smooth_rows"][0] == 2 and names["k_smooth_topics"][0] == 2
        # the scratch goes with release_scratch and comes back with the next call
        eng.release_scratch()
        eng.set_factors(U0, V0)
        iters, _ = eng.fit_smoothed(0.5, 0.05, sw, flags=PLSA_FUSED, **kw)
        assert iters == 2
    # the Python layer refuses before an engine is touched
    for bad_kw in (dict(doc_topic_smoothing=-1.0), dict(topic_word_smoothing=nan), dict(doc_topic_smoothing="much"),
                   dict(doc_topic_smoothing=0.1, flags=0), dict(doc_topic_smoothing=0.1, flags=PLSA_FUSED | PLSA_REFERENCE_SUMS)):
        with pytest.raises(ValueError):
            amd.plsa_fit_smoothed(X, k, None, **bad_kw)


@pytest.mark.gpu
def test_a_shard_of_a_communicator_is_refused(amd, tmp_path):
    """a context with a communicator (one rank: RCCL refuses two ranks on one device) refuses all three entry points, at
    positive pseudo-counts and at (0, 0), launches nothing and keeps its factors; without the communicator it fits again"""
    from enstop_amd import comm
    k = 21
    X, U0, V0, sw = matrix_corpus(k)
    kw = dict(n_iter=2, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED)
    with make_engine(amd, {}, X) as eng:
        eng.set_factors(U0, V0)
        c = comm.RcclComm(eng, 0, 1, comm.rendezvous_id(0, str(tmp_path / "rccl.id")))
        try:
            assert eng.comm_info() == (0, 1)
            eng.timing(True)
            eng.timing_reset()
            for a, b in ((0.5, 0.05), (0.5, 0.0), (0.0, 0.05), (0.0, 0.0)):
                with pytest.raises(amd.DeviceError, match="communicator"):
                    eng.fit_smoothed(a, b, sw, **kw)
                with pytest.raises(amd.DeviceError, match="communicator"):
                    eng.refit_smoothed(a, sw, **kw)
                with pytest.raises(amd.DeviceError, match="communicator"):
                    eng.log_posterior(sw, a, b)
            assert eng.timing_report() == {}, eng.timing_report()        # nothing was launched
            U, V = eng.get_factors()
            same_bits(U, U0, "a refusal moved U")
            same_bits(V, V0, "a refusal moved V")
        finally:
            c.close()
        iters, _ = eng.fit_smoothed(0.5, 0.05, sw, **kw)
        assert iters == 2 and eng.timing_report()["k_smooth_rows"][0] == 2


# ------------------------------------------------------------------------------------------------
# 12. capped grids
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_capped_grid_computes_the_same_bits(amd):
    """k = 6 (kq = 2, pads in the second quarter).  n and m come from the CU count as in test_capped_grids.sizes: under
    PLSA_GRID_MULT=1 both k_smooth_rows (n kq float4s) and k_smooth_topics (m kq) make three trips at least with a ragged last
    one -- n kq and m kq above 2 CUs 256 and no multiple of CUs 256."""
    k, kq = 6, 2
    with amd.Engine() as probe:
        cus = probe.device_info()["cus"]
    n, m = sizes(k, cus)
    for count in (n, m):
        assert count * kq > 2 * cus * 256 and (count * kq) % (cus * 256) != 0, (count, cus)
    rs = np.random.RandomState(12)
    per_doc = 3
    rows = np.repeat(np.arange(n), per_doc)
    rows[:per_doc] = 1                                    # document 0 is empty
    cols = rs.randint(0, m, size=rows.shape[0])
    cols[-m:] = np.arange(m)                              # every word occurs
    X = sp.csr_matrix((rs.randint(1, 5, size=rows.shape[0]).astype(np.float32), (rows, cols)), shape=(n, m))
    X.sum_duplicates()
    U0 = rs.rand(n, k).astype(np.float32) + 0.05
    U0 /= U0.sum(1, keepdims=True)
    V0 = rs.rand(k, m).astype(np.float32) + 0.05
    V0 /= V0.sum(1, keepdims=True)
    sw = (0.5 + rs.rand(n)).astype(np.float32)
    got = {}
    for capped in (True, False):
        with cap_knobs(CAP if capped else {}):
            eng = amd.Engine()
        with eng:
            eng.upload_csr(X)
            eng.set_factors(U0, V0)
            iters, trace = eng.fit_smoothed(0.5, 0.05, sw, trace=True, **ONE)
            got[capped] = eng.get_factors()
    same_bits(got[True][0], got[False][0], "capped: P(z|d)")
    same_bits(got[True][1], got[False][1], "capped: P(w|z)")
    U1, V1 = got[True]
    np.testing.assert_allclose(U1[0], 1.0 / k, rtol=8 * U32)
    assert (U1 > 0).all() and (V1 > 0).all()
    assert np.abs(U1.astype(np.float64).sum(1) - 1).max() <= (k + 5) * U32
    assert np.abs(V1.astype(np.float64).sum(1) - 1).max() <= (-(-m // 256) + 5) * U32
