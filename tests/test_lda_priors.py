"""LDA with a vector document-topic prior and learned priors on the device (enstop_amd/include/plsa_hip_lda_priors.h:
plsa_lda_prior_fit, plsa_lda_prior_refit, plsa_lda_prior_bound, plsa_lda_prior_stats; enstop_amd/lda.py)
against the float64 model of tests/lda_prior_model.py.

    gamma_dz = alpha_z + sum_w x_dw phi_dwz        lambda_zw = eta + sum_d x_dw phi_dwz
    T_z = sum_d (psi(gamma_dz) - psi(S_d))         T'_z = sum_w (psi(lambda_zw) - psi(S_z))
    F(alpha) = n [lgamma(sum alpha) - sum lgamma(alpha_z)] + sum alpha_z T_z        F(eta) = k [lgamma(m eta) - m lgamma(eta)] + eta sum_z T'_z

Kernel-level tests run on test_lda_em.corpus(k) (640 x 480, about 4 000 non-zeros, empty documents, a word without entries,
stored zeros) for k in {3, 6, 21, 64, 130, 1024}, with the prior vectors 0.5 uniform, 0.5 / (1 + z) and 0.5 with one
component 10^-3, eta = 0.05, from gamma0 = alpha + 20 U0, lambda0 = eta + 50 V0.

Error model of the sums (u53 = 2^-53).  A term is psi(x) - psi(S), two digammas, each within 2^-47 max(1, |psi|) of SciPy's
(test_lda_math_host.py establishes that for the device's digamma against scipy.special.psi, so it covers both sides).  S is a
float64 sum of L float32 entries on either side (L = k for a document, m = 480 for a topic, in different orders): L u53
relative, which psi carries into the term times S psi'(S) <= 1 + 1 / S.  The float64 sum of the terms: 2^-50 sum |terms|, as
check_bound allows for the bound's sums.  So for every topic
    |T - model| <= sum_terms [2^-47 (max(1, |psi(x)|) + max(1, |psi(S)|)) + (1 + 1 / S) L u53] + 2^-50 sum |terms| .

The step and the bound under a vector prior are held to test_lda_em.py's bounds (step_bounds, check_bound): the arithmetic is
the scalar form's with alpha_z in the place of alpha.
"""
import functools

import numpy as np
import pytest
from scipy.special import psi

import lda_model as lm
import lda_prior_model as pm
import test_lda_em as em
from test_capped_grids import CAP, knobs as cap_knobs
from test_fit_driver import PLSA_FUSED, PLSA_GRAPH, PLSA_SHARDED, make_engine, same_bits
from test_pass_matrix import C_FACTOR, EMPTY_DOCS, U32, check

THRESH = em.THRESH
K = em.K
ETA = 0.05
FLOOR = 1e-6
ONE = em.ONE
VECTORS = ("uniform", "decreasing", "one small")


def vector(kind, k):
    if kind == "uniform":
        return np.full(k, 0.5)
    if kind == "decreasing":
        return 0.5 / (1.0 + np.arange(k))
    alpha = np.full(k, 0.5)
    alpha[k // 2] = 1e-3
    return alpha


@functools.lru_cache(maxsize=None)
def start(k, kind):
    X, U0, V0 = em.corpus(k)
    alpha = vector(kind, k).astype(np.float32)
    return (alpha[None, :] + 20 * U0).astype(np.float32), (np.float32(ETA) + 50 * V0).astype(np.float32)


@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


@pytest.fixture(scope="module")
def worst():
    out = {}
    yield out
    for k in sorted(out):
        print("\nLDA priors k=%d: worst error / bound: " % k + ", ".join("%s %.3g" % kv for kv in sorted(out[k].items())))


def sums_bounds(gamma, lam):
    """the bound of the docstring for T [k] and T' [k]"""
    g, l = lm.state64(gamma, lam)
    out = []
    for T, S, L in ((g, g.sum(1, keepdims=True), g.shape[1]), (l.T, l.sum(1, keepdims=True).T, l.shape[1])):
        terms = psi(T) - psi(S)
        per = 2.0 ** -47 * (np.maximum(1.0, np.abs(psi(T))) + np.maximum(1.0, np.abs(psi(S)))) + (1.0 + 1.0 / S) * L * 2.0 ** -53
        out.append(per.sum(0) + 2.0 ** -50 * np.abs(terms).sum(0))
    return out


def check_vector_bound(tag, got, X, gamma, lam, k, alpha, eta, ratios, float32=True):
    want, ll_scale, scale = pm.bound64_v(X, gamma, lam, alpha, eta)
    bound = C_FACTOR * (k + 1) * U32 * ll_scale + 2.0 ** -50 * scale + (abs(want) * U32 if float32 else 0.0)
    err = abs(float(got) - want)
    print("%s: L %.6f, model %.6f, error %.3g, bound %.3g" % (tag, got, want, err, bound))
    assert err <= bound, (tag, got, want, err, bound)
    ratios["L"] = max(ratios.get("L", 0.0), err / bound)


# ------------------------------------------------------------------------------------------------
# 1. the sums
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_sums_against_the_model(amd, worst, k):
    X, _, _ = em.corpus(k)
    ratios = worst.setdefault(k, {})
    with make_engine(amd, {}, X) as eng:
        eng.timing(True)
        for kind in VECTORS:
            gamma0, lam0 = start(k, kind)
            eng.set_factors(gamma0, lam0)
            eng.timing_reset()
            t_doc, t_topic = eng.lda_prior_stats()
            names = eng.timing_report()
            assert names["k_lda_logmean"][0] == 2 and names["k_lda_logmean_sums"][0] == 2, names
            want_doc, want_topic, _, _ = pm.sums64(gamma0, lam0)
            b_doc, b_topic = sums_bounds(gamma0, lam0)
            for name, got, want, bound in (("T", t_doc, want_doc, b_doc), ("T'", t_topic, want_topic, b_topic)):
                r = float((np.abs(got - want) / bound).max())
                print("k=%d %s %s: largest error / bound %.3g (largest |sum| %.6g)" % (k, kind, name, r, np.abs(want).max()))
                assert r <= 1.0, (k, kind, name, r)
                assert (got < 0).all()
                ratios[name] = max(ratios.get(name, 0.0), r)
            g, l = eng.get_factors()
            same_bits(g, gamma0, "lda_prior_stats moved gamma")
            same_bits(l, lam0, "lda_prior_stats moved lambda")


@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_the_sums_do_not_depend_on_the_launch_geometry(amd, k):
    X, _, _ = em.corpus(k)
    got = {}
    for capped in (True, False):
        with cap_knobs(CAP if capped else {}):
            eng = amd.Engine()
        with eng:
            eng.upload_csr(X)
            got[capped] = []
            for kind in VECTORS[1:]:
                eng.set_factors(*start(k, kind))
                got[capped].extend(eng.lda_prior_stats())
    for a, b in zip(got[True], got[False]):
        same_bits(a, b, "capped: the sums")


# ------------------------------------------------------------------------------------------------
# 2. a uniform vector is the scalar
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [6, 130])
def test_a_uniform_vector_is_the_scalar(amd, k):
    X, _, _ = em.corpus(k)
    a, eta = 0.1, 0.05
    gamma0, lam0 = em.start(k, a, eta)
    loop = dict(n_iter=3, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED, trace=True)
    with make_engine(amd, {}, X) as eng:
        eng.timing(True)
        eng.set_factors(gamma0, lam0)
        iters, trace = eng.lda_fit(a, eta, **loop)
        g_s, l_s = eng.get_factors()
        bound_s = eng.lda_bound(a, eta)
        eng.set_factors(gamma0, lam0)
        eng.timing_reset()
        iters_v, trace_v, alpha, eta_v = eng.lda_prior_fit(np.full(k, a), eta, learn=0, **loop)
        names = eng.timing_report()
        g_v, l_v = eng.get_factors()
        assert iters == iters_v == 3 and len(trace_v) == 4 and eta_v == eta and (alpha == a).all()
        assert names["k_lda_rows_v"][0] == 3 and "k_lda_rows" not in names and "k_lda_logmean" not in names, sorted(names)
        same_bits(g_v, g_s, "uniform vector: gamma")
        same_bits(l_v, l_s, "uniform vector: lambda")
        _, _, scale = lm.bound64(X, g_s, l_s, a, eta)
        bound_v = eng.lda_prior_bound(np.full(k, a), eta)
        print("k=%d: bound %.9f (vector) %.9f (scalar), difference / (2^-50 sum |terms|) %.3g"
              % (k, bound_v, bound_s, abs(bound_v - bound_s) / (2.0 ** -50 * scale)))
        assert abs(bound_v - bound_s) <= 2.0 ** -50 * scale
        np.testing.assert_allclose(trace_v, trace, rtol=2 * U32)
        # the refit
        eng.set_factors(gamma0, lam0)
        eng.lda_refit(a, **loop)
        g_s = eng.get_factors()[0]
        eng.set_factors(gamma0, lam0)
        iters_v, _ = eng.lda_prior_refit(np.full(k, a), **loop)
        g_v, l_v = eng.get_factors()
        assert iters_v == 3
        same_bits(g_v, g_s, "uniform vector, refit: gamma")
        same_bits(l_v, lam0, "the refit wrote lambda")


# ------------------------------------------------------------------------------------------------
# 3. one step and the bound under a vector prior
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_one_step_with_a_vector_prior_against_the_model(amd, worst, k):
    X, _, _ = em.corpus(k)
    ratios = worst.setdefault(k, {})
    with make_engine(amd, {}, X) as eng:
        for kind in VECTORS[1:]:
            alpha = vector(kind, k)
            gamma0, lam0 = start(k, kind)
            want = pm.step64_v(X, gamma0, lam0, alpha, ETA, THRESH)
            eng.set_factors(gamma0, lam0)
            iters, trace, alpha_out, eta_out = eng.lda_prior_fit(alpha, ETA, learn=0, trace=True, **ONE)
            gamma, lam = eng.get_factors()
            assert iters == 1 and len(trace) == 2 and (alpha_out == alpha).all() and eta_out == ETA
            b_u, b_v = em.step_bounds(want, k)
            check("gamma " + kind, gamma, want["gamma"], b_u, ratios)
            check("lambda " + kind, lam, want["lam"], b_v, ratios)
            assert (gamma > 0).all() and (lam > 0).all()
            for d in EMPTY_DOCS:
                check("empty document " + kind, gamma[d], alpha, U32, ratios)
            check("word without entries " + kind, lam[:, em.UNUSED_WORD], np.full(k, ETA), U32, ratios)
            check_vector_bound(kind + " before", trace[0], X, gamma0, lam0, k, alpha, ETA, ratios)
            check_vector_bound(kind + " after", trace[1], X, gamma, lam, k, alpha, ETA, ratios)
            # the fold-in step
            want = pm.step64_v(X, gamma0, lam0, alpha, ETA, THRESH, update_v=False)
            eng.set_factors(gamma0, lam0)
            eng.lda_prior_refit(alpha, **ONE)
            gamma, lam = eng.get_factors()
            check("gamma, refit " + kind, gamma, want["gamma"], b_u, ratios)
            same_bits(lam, lam0, "the refit wrote lambda")


@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_bound_with_a_vector_prior_against_the_model(amd, worst, k):
    X, _, _ = em.corpus(k)
    ratios = worst.setdefault(k, {})
    with make_engine(amd, {}, X) as eng:
        for kind in VECTORS[1:]:
            alpha = vector(kind, k)
            gamma0, lam0 = start(k, kind)
            eng.set_factors(gamma0, lam0)
            tag = "k=%d %s" % (k, kind)
            check_vector_bound(tag, eng.lda_prior_bound(alpha, ETA), X, gamma0, lam0, k, alpha, ETA, ratios, float32=False)
            check_vector_bound(tag + " without topics", eng.lda_prior_bound(alpha), X, gamma0, lam0, k, alpha, None, ratios,
                               float32=False)


# ------------------------------------------------------------------------------------------------
# 4. the prior step
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [6, 64, 130])
def test_the_prior_step_maximises_the_bound_over_the_priors(amd, k):
    """One iteration with learn = 3 and prior_start = 1.  From the gamma and lambda read back the model forms T in float64; the
    returned alpha must have |g_z| <= 1e-8 (n |psi(sum alpha)| + n |psi(alpha_z)| + |T_z|) wherever it is above the floor, ten
    times the routine's own rule (the device's T differs from SciPy's by about 2^-39 of that scale), eta likewise, and the
    bound of the same state is no lower under the new priors than under the old."""
    X, _, _ = em.corpus(k)
    n, m = X.shape
    alpha0 = vector("decreasing", k)
    gamma0, lam0 = start(k, "decreasing")
    with make_engine(amd, {}, X) as eng:
        eng.timing(True)
        eng.set_factors(gamma0, lam0)
        eng.timing_reset()
        iters, trace, alpha, eta = eng.lda_prior_fit(alpha0, ETA, learn=3, prior_start=1, trace=True, **ONE)
        names = eng.timing_report()
        gamma, lam = eng.get_factors()
        assert iters == 1 and len(trace) == 2
        assert names["k_lda_logmean"][0] == 2 and names["k_lda_rows_v"][0] == 1, names
        # the tables of the new state are formed once: by the update, for the bound behind it
        assert names["k_lda_rowsum"][0] == 2, names
        T, Tt, _, _ = pm.sums64(gamma, lam)
        g, scale = pm.alpha_gradient(alpha, T, n)
        free = alpha > FLOOR
        g_eta, scale_eta = pm.eta_gradient(eta, Tt.sum(), k, m)
        print("\nk=%d: alpha %.4g .. %.4g (%d on the floor), |g| / scale %.3g; eta %.5g, |g| / scale %.3g"
              % (k, alpha.min(), alpha.max(), (~free).sum(), (np.abs(g) / scale)[free].max(), eta, abs(g_eta) / scale_eta))
        assert (alpha >= FLOOR).all() and free.any() and not (alpha == alpha0).all() and eta != ETA
        assert ((np.abs(g) / scale)[free] <= 1e-8).all()
        assert (g[~free] <= 0).all()
        assert eta > FLOOR and abs(g_eta) <= 1e-8 * scale_eta
        assert pm.alpha_objective(alpha, T, n) >= pm.alpha_objective(alpha0, T, n)
        new, old = eng.lda_prior_bound(alpha, eta), eng.lda_prior_bound(alpha0, ETA)
        print("bound %.6f under the new priors, %.6f under the old" % (new, old))
        assert new >= old
        assert abs(np.float32(new) - trace[1]) <= abs(new) * U32        # the trace's last value is the bound under the new priors
        # learn = 1 and learn = 2 move one prior each
        eng.set_factors(gamma0, lam0)
        _, _, a1, e1 = eng.lda_prior_fit(alpha0, ETA, learn=1, prior_start=1, **ONE)
        eng.set_factors(gamma0, lam0)
        _, _, a2, e2 = eng.lda_prior_fit(alpha0, ETA, learn=2, prior_start=1, **ONE)
        same_bits(a1, alpha, "learn = 1: alpha")
        assert e1 == ETA and (a2 == alpha0).all() and e2 == eta


# ------------------------------------------------------------------------------------------------
# 5. the loop
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_the_loop_is_the_step_iterated(amd, k):
    X, _, _ = em.corpus(k)
    alpha0 = vector("decreasing", k)
    gamma0, lam0 = start(k, "decreasing")
    loop = dict(n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED, trace=True)
    with make_engine(amd, {}, X) as eng:
        eng.set_factors(gamma0, lam0)
        alpha, eta, stages = alpha0, ETA, []
        for step in range(5):
            iters, trace, alpha, eta = eng.lda_prior_fit(alpha, eta, learn=3, prior_start=1, n_iter=1, **loop)
            assert iters == 1 and len(trace) == 2
            stages.append(trace)
        gamma, lam = eng.get_factors()
        eng.set_factors(gamma0, lam0)
        iters, trace, alpha5, eta5 = eng.lda_prior_fit(alpha0, ETA, learn=3, prior_start=1, n_iter=5, **loop)
        g5, l5 = eng.get_factors()
        assert iters == 5 and len(trace) == 6
        same_bits(g5, gamma, "five iterations: gamma")
        same_bits(l5, lam, "five iterations: lambda")
        same_bits(alpha5, alpha, "five iterations: alpha")
        assert eta5 == eta
        same_bits(trace, np.array([stages[0][0]] + [s[1] for s in stages], np.float32), "five iterations: trace")
        # prior_start = 3, prior_every = 2: the priors change behind the iterations 3 and 5 only
        seen = {}
        for n_iter in (2, 3, 4, 5):
            eng.set_factors(gamma0, lam0)
            iters, _, a, e = eng.lda_prior_fit(alpha0, ETA, learn=3, prior_start=3, prior_every=2, n_iter=n_iter, **loop)
            assert iters == n_iter
            seen[n_iter] = (a, e)
        assert (seen[2][0] == alpha0).all() and seen[2][1] == ETA
        assert not (seen[3][0] == alpha0).all() and seen[3][1] != ETA
        same_bits(seen[4][0], seen[3][0], "no update behind iteration 4: alpha")
        assert seen[4][1] == seen[3][1]
        assert not (seen[5][0] == seen[3][0]).all() and seen[5][1] != seen[3][1]


@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_no_stop_before_the_first_update(amd, k):
    """A tolerance of 10^6 (the relative change of the bound is far below it) stops the fixed-prior loop at its first test, behind
    iteration 1; with a learned prior and prior_start = 4
    the tests behind the iterations 1 .. 3 are recorded and set aside, and the test behind iteration 4 stops the loop"""
    X, _, _ = em.corpus(k)
    alpha0 = vector("decreasing", k)
    gamma0, lam0 = start(k, "decreasing")
    loop = dict(n_iter=10, n_iter_per_test=1, tolerance=1e6, e_step_thresh=THRESH, flags=PLSA_FUSED, trace=True)
    with make_engine(amd, {}, X) as eng:
        eng.set_factors(gamma0, lam0)
        iters, trace, alpha, eta = eng.lda_prior_fit(alpha0, ETA, learn=0, prior_start=4, **loop)
        assert iters == 1 and len(trace) == 2 and (alpha == alpha0).all()
        eng.set_factors(gamma0, lam0)
        iters, trace, alpha, eta = eng.lda_prior_fit(alpha0, ETA, learn=3, prior_start=4, **loop)
        assert iters == 4 and len(trace) == 5, (iters, trace)
        assert not (alpha == alpha0).all() and eta != ETA


# ------------------------------------------------------------------------------------------------
# 6. what it is for
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_learned_priors_on_the_planted_corpus(amd):
    """lda_prior_model.planted(): 640 + 640 documents of 100 tokens over 480 words, 8 topics, two of them heavy.  60 iterations,
    prior_start = 20, "auto" for both priors (alpha and eta start at 1 / k and hold it through the burn-in), tolerance 0, a test
    behind every iteration, against the fixed 1 / k, 0.01 fit from the same start.  The float64 model in the same configuration
    (lda_prior_model.planted_run; python tests/lda_prior_model.py), corpus seed 2, start seeds 0 .. 4:
        smallest alpha of a heavy-matched topic / largest of the others 6.29, 1.34, 1.35, 0.83, 0.97 (seed 0: 0.779 / 0.124);
        held-out perplexity 95.6 against 105.7, 102.7 / 111.4, 99.2 / 108.7, 100.7 / 110.1, 98.9 / 109.3: 7.8 to 9.5 % lower;
        eta from 1 / k to 0.053 .. 0.066; the bound never decreases, its smallest increase is 21.7 .. 60.2;
        with prior_start = 1 alpha runs off to 645 .. 694 per topic and the perplexity is 147.5.
    The split of alpha is not a property of every run (lda_prior_model.FIGURES has all twenty that were tried); the start seed
    is the one with the widest gap, 0, and the model is run first.  On an MI355X: alpha 0.78 and 0.83 for the heavy-matched
    topics against at most 0.124, eta 0.058, smallest increase of the float32 trace 38.2 against an allowed decrease of 1.05,
    perplexity 95.6 against 105.7; with prior_start = 1 alpha ends at 645 .. 694."""
    X, X_test, topics = pm.planted()
    seed = pm.START_SEED
    k = pm.PLANTED["topics"]
    model = pm.planted_run(seed)
    lo, hi = pm.heavy_split(model["alpha"], model["lam"], topics)
    fixed_model = pm.planted_run(seed, learn=False)
    assert lo > 3 * hi and model["perplexity"] < 0.95 * fixed_model["perplexity"] and np.diff(model["L"]).min() > 10
    kw = dict(n_components=k, n_iter=60, n_iter_per_test=1, tolerance=0.0, random_state=seed)
    learned = amd.LDA(doc_topic_prior="auto", topic_word_prior="auto", **kw).fit(X)
    fixed = amd.LDA(doc_topic_prior=None, topic_word_prior=0.01, **kw).fit(X)
    assert learned.n_iter_ == 60 and len(learned.bound_trace_) == 61
    assert learned.doc_topic_prior_.shape == (k,) and (fixed.doc_topic_prior_ == 1.0 / k).all() and fixed.topic_word_prior_ == 0.01
    trace = learned.bound_trace_.astype(np.float64)
    allowed = max(lm.monotone_bound(k, X.sum(), a, b, f) for a, b, f in zip(model["ll_scales"], model["scales"], model["L"]))
    lo_d, hi_d = pm.heavy_split(learned.doc_topic_prior_, learned.components_, topics)
    p_learned, p_fixed = learned.perplexity(X_test), fixed.perplexity(X_test)
    print("\nplanted corpus on the device: alpha %s, heavy-matched >= %.3f, others <= %.3f (model %.3f / %.3f); eta %.4f (model "
          "%.4f); L %.1f -> %.1f, smallest increase %.3f (allowed decrease %.3f); perplexity %.2f against %.2f (model %.1f / %.1f)"
          % (np.round(learned.doc_topic_prior_, 3), lo_d, hi_d, lo, hi, learned.topic_word_prior_, model["eta"], trace[0],
             trace[-1], np.diff(trace).min(), allowed, p_learned, p_fixed, model["perplexity"], fixed_model["perplexity"]))
    assert (np.diff(trace) >= -allowed).all(), np.diff(trace).min()
    # the first 20 iterations are the fixed-prior fit's
    same_bits(learned.bound_trace_[:20], fixed_trace_head(amd, X, k, seed), "the burn-in is the fixed 1 / k, 1 / k fit")
    assert lo_d > hi_d
    assert p_learned < p_fixed
    T = learned.transform(X_test)
    assert T.shape == (X_test.shape[0], k) and (T > 0).all() and np.abs(T.astype(np.float64).sum(1) - 1).max() <= (k + 5) * U32
    # the reason for the default: updates from the first iteration on run away
    early = amd.LDA(doc_topic_prior="auto", topic_word_prior="auto", **kw)
    early.prior_start = 1
    early.fit(X)
    print("prior_start = 1: alpha %.0f .. %.0f" % (early.doc_topic_prior_.min(), early.doc_topic_prior_.max()))
    assert early.doc_topic_prior_.max() > 100


def fixed_trace_head(amd, X, k, seed):
    """the first 20 values of the trace of the fixed 1 / k, 1 / k fit from the same start: the start of an "auto" fit"""
    _, _, info = amd.lda_fit(X, k, None, None, n_iter=19, n_iter_per_test=1, tolerance=0.0, random_state=seed, return_info=True)
    return info["bound_trace"]


@pytest.mark.gpu
def test_the_python_layer_takes_vectors_and_names(amd):
    X, X_test, _ = pm.planted()
    k = 8
    asym = 1.0 / (np.arange(1, k + 1) + np.sqrt(k))
    asym /= asym.sum()
    gamma, lam, info = amd.lda_fit(X, k, "asymmetric", 0.05, n_iter=5, random_state=1, return_info=True)
    same_bits(info["doc_topic_prior_"], asym, "asymmetric")
    assert info["topic_word_prior_"] == 0.05 and info["n_iter"] == 5
    gamma_v, lam_v = amd.lda_fit(X, k, list(asym), 0.05, n_iter=5, random_state=1)
    same_bits(gamma_v, gamma, "the same vector as a list: gamma")
    same_bits(lam_v, lam, "the same vector as a list: lambda")
    folded = amd.lda_transform(X_test, lam, asym, random_state=1)
    assert folded.shape == (X_test.shape[0], k) and (folded > 0).all()
    # a uniform vector folds in to the scalar's bits
    same_bits(amd.lda_transform(X_test, lam, np.full(k, 0.1), random_state=1), amd.lda_transform(X_test, lam, 0.1, random_state=1),
              "uniform vector: fold-in")
    model = amd.LDA(n_components=k, doc_topic_prior="asymmetric", n_iter=5, random_state=1).fit(X)
    same_bits(model.doc_topic_prior_, asym, "LDA: asymmetric")
    assert model.topic_word_prior_ == 1.0 / k and np.isfinite(model.score(X_test)) and model.perplexity(X_test) > 1


# ------------------------------------------------------------------------------------------------
# 7. refusals
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_launch_nothing_and_leave_the_state(amd):
    k = 21
    X, _, _ = em.corpus(k)
    alpha0 = vector("decreasing", k)
    gamma0, lam0 = start(k, "decreasing")
    kw = dict(n_iter=2, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH)
    nan, inf = float("nan"), float("inf")

    def spoiled(value):
        alpha = alpha0.copy()
        alpha[k - 1] = value
        return alpha
    with make_engine(amd, {}, X) as eng:
        eng.set_factors(gamma0, lam0)
        eng.timing(True)
        eng.timing_reset()
        bad = [(alpha0, ETA, 1, 0, "PLSA_FUSED"), (alpha0, ETA, 1, PLSA_FUSED | PLSA_SHARDED, "PLSA_SHARDED"),
               (alpha0, ETA, 1, PLSA_FUSED | PLSA_GRAPH, "PLSA_GRAPH"), (alpha0, ETA, 1, PLSA_FUSED | em.PLSA_REFERENCE_SUMS, "PLSA_REFERENCE_SUMS"),
               (alpha0, ETA, 1, PLSA_FUSED | em.PLSA_REFERENCE_LL, "PLSA_REFERENCE_LL"),
               (spoiled(0.0), ETA, 1, PLSA_FUSED, "alpha="), (spoiled(-0.1), ETA, 1, PLSA_FUSED, "alpha="),
               (spoiled(nan), ETA, 1, PLSA_FUSED, "alpha="), (spoiled(inf), ETA, 1, PLSA_FUSED, "alpha="),
               (alpha0, 0.0, 1, PLSA_FUSED, "eta="), (alpha0, nan, 1, PLSA_FUSED, "eta="), (alpha0, inf, 1, PLSA_FUSED, "eta="),
               (alpha0, ETA, 0, PLSA_FUSED, "doc_iter")]
        for alpha, eta, doc_iter, flags, word in bad:
            with pytest.raises(amd.DeviceError, match=word):
                eng.lda_prior_fit(alpha, eta, doc_iter=doc_iter, flags=flags, **kw)
            if word != "eta=":
                with pytest.raises(amd.DeviceError, match=word):
                    eng.lda_prior_refit(alpha, doc_iter=doc_iter, flags=flags, **kw)
            if word in ("alpha=", "eta="):
                with pytest.raises(amd.DeviceError, match=word):
                    eng.lda_prior_bound(alpha, eta)
        for extra, word in ((dict(prior_start=0), "prior_start"), (dict(prior_every=0), "prior_every"), (dict(learn=4), "learn"),
                            (dict(learn=-1), "learn")):
            with pytest.raises(amd.DeviceError, match=word):
                eng.lda_prior_fit(alpha0, ETA, flags=PLSA_FUSED, **dict(kw, **extra))
        with pytest.raises(ValueError):
            eng.lda_prior_fit(alpha0[:-1], ETA, **kw)
        for arithmetic in ("reference", "reference_source"):
            eng.set_arithmetic(arithmetic)
            for call in (lambda: eng.lda_prior_fit(alpha0, ETA, flags=PLSA_FUSED, **kw), lambda: eng.lda_prior_refit(alpha0, flags=PLSA_FUSED, **kw),
                         lambda: eng.lda_prior_bound(alpha0, ETA), eng.lda_prior_stats):
                with pytest.raises(amd.DeviceError, match="reference arithmetic"):
                    call()
        eng.set_arithmetic(None)
        assert eng.timing_report() == {}, eng.timing_report()        # nothing was launched
        g, l = eng.get_factors()
        same_bits(g, gamma0, "a refusal moved gamma")
        same_bits(l, lam0, "a refusal moved lambda")
        iters, _, a_first, e_first = eng.lda_prior_fit(alpha0, ETA, learn=3, prior_start=1, flags=PLSA_FUSED, **kw)
        names = eng.timing_report()
        assert iters == 2 and names["k_lda_rows_v"][0] == 2 and names["k_lda_topics"][0] == 2 and names["k_lda_logmean"][0] == 4
        first = eng.get_factors()
        stats = eng.lda_prior_stats()
        # the scratch goes with release_scratch and comes back with the next call
        eng.release_scratch()
        same_bits(np.concatenate(eng.lda_prior_stats()), np.concatenate(stats), "after release_scratch: the sums")
        eng.release_scratch()
        eng.set_factors(gamma0, lam0)
        iters, _, a_again, e_again = eng.lda_prior_fit(alpha0, ETA, learn=3, prior_start=1, flags=PLSA_FUSED, **kw)
        assert iters == 2 and e_again == e_first
        same_bits(a_again, a_first, "after release_scratch: alpha")
        same_bits(eng.get_factors()[0], first[0], "after release_scratch: gamma")
        same_bits(eng.get_factors()[1], first[1], "after release_scratch: lambda")


@pytest.mark.gpu
def test_a_shard_of_a_communicator_is_refused(amd, tmp_path):
    from enstop_amd import comm
    k = 21
    X, _, _ = em.corpus(k)
    alpha0 = vector("decreasing", k)
    gamma0, lam0 = start(k, "decreasing")
    kw = dict(n_iter=2, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED)
    with make_engine(amd, {}, X) as eng:
        eng.set_factors(gamma0, lam0)
        c = comm.RcclComm(eng, 0, 1, comm.rendezvous_id(0, str(tmp_path / "rccl.id")))
        try:
            eng.timing(True)
            eng.timing_reset()
            for call in (lambda: eng.lda_prior_fit(alpha0, ETA, **kw), lambda: eng.lda_prior_refit(alpha0, **kw),
                         lambda: eng.lda_prior_bound(alpha0, ETA), eng.lda_prior_stats):
                with pytest.raises(amd.DeviceError, match="communicator"):
                    call()
            assert eng.timing_report() == {}, eng.timing_report()
            same_bits(eng.get_factors()[0], gamma0, "a refusal moved gamma")
        finally:
            c.close()
        iters, _, _, _ = eng.lda_prior_fit(alpha0, ETA, **kw)
        assert iters == 2


# ------------------------------------------------------------------------------------------------
# 8. the Python refusals (no GPU)
# ------------------------------------------------------------------------------------------------
def test_the_python_refusals_come_before_any_engine(monkeypatch):
    import scipy.sparse as sp
    import enstop_amd
    from enstop_amd import engine, lda, plsa

    def no_engine(*args, **kwargs):
        raise AssertionError("an engine was asked for")
    for module in (engine, lda, plsa):
        monkeypatch.setattr(module, "get_engine", no_engine)
    X = sp.random(12, 9, density=0.5, format="csr", random_state=0, dtype=np.float32)
    nan = float("nan")
    for kw in (dict(doc_topic_prior=[0.1, 0.2]), dict(doc_topic_prior=[0.1, 0.2, 0.3, 0.4]), dict(doc_topic_prior=[0.1, 0.0, 0.3]),
               dict(doc_topic_prior=[0.1, nan, 0.3]), dict(doc_topic_prior=[0.1, float("inf"), 0.3]), dict(doc_topic_prior=[0.1, -0.2, 0.3]),
               dict(doc_topic_prior=np.ones((3, 1))), dict(doc_topic_prior=["a", "b", "c"]), dict(doc_topic_prior="symmetric"),
               dict(topic_word_prior=[0.1, 0.2, 0.3]), dict(topic_word_prior=np.full(9, 0.1)), dict(topic_word_prior="asymmetric")):
        with pytest.raises(ValueError):
            enstop_amd.lda_fit(X, 3, **kw)
        with pytest.raises(ValueError):
            enstop_amd.LDA(n_components=3, **kw).fit(X)
    for kw in (dict(prior_every=0), dict(prior_start=0), dict(prior_every=1.5), dict(prior_start=True)):
        with pytest.raises(ValueError):
            enstop_amd.lda_fit(X, 3, doc_topic_prior="auto", **kw)
        model = enstop_amd.LDA(n_components=3, doc_topic_prior="auto")
        for name, value in kw.items():
            setattr(model, name, value)
        with pytest.raises(ValueError):
            model.fit(X)
    lam = np.ones((3, 9), np.float32)
    for alpha in ([0.1, 0.2], [0.1, 0.0, 0.2], [0.1, nan, 0.2], "auto", "asymmetric"):
        with pytest.raises(ValueError):
            enstop_amd.lda_transform(X, lam, alpha)


def test_the_named_priors():
    from enstop_amd.lda import LDA, resolve_doc_topic_prior, resolve_topic_word_prior
    for k in (1, 2, 8, 100):
        alpha, learn = resolve_doc_topic_prior("asymmetric", k)
        assert not learn and alpha.shape == (k,) and abs(alpha.sum() - 1.0) <= 4 * 2.0 ** -53 * k and (np.diff(alpha) < 0).all()
        np.testing.assert_allclose(alpha * (1.0 / (np.arange(1, k + 1) + np.sqrt(k))).sum(), 1.0 / (np.arange(1, k + 1) + np.sqrt(k)),
                                   rtol=1e-15)
        alpha, learn = resolve_doc_topic_prior("auto", k)
        assert learn and (alpha == 1.0 / k).all() and alpha.shape == (k,)
        assert resolve_topic_word_prior("auto", k) == (1.0 / k, True)
        assert resolve_doc_topic_prior(None, k) == (1.0 / k, False) and resolve_doc_topic_prior(0.3, k) == (0.3, False)
        assert resolve_topic_word_prior(0.2, k) == (0.2, False)
    # a 0-d value takes the scalar path, as it always did: a NumPy scalar is a number, a 0-d array is refused as not one
    assert resolve_doc_topic_prior(np.float32(0.25), 4) == (0.25, False)
    with pytest.raises(ValueError, match="finite number"):
        resolve_doc_topic_prior(np.array(0.3), 4)
    alpha, learn = resolve_doc_topic_prior((0.5, 0.25), 2)
    assert not learn and alpha.dtype == np.float64 and (alpha == [0.5, 0.25]).all()
    assert LDA.prior_start == 20 and LDA.prior_every == 1 and "prior_start" not in LDA().get_params()
    import inspect
    import enstop_amd
    signature = inspect.signature(enstop_amd.lda_fit)
    assert signature.parameters["prior_start"].default == 20 and signature.parameters["prior_every"].default == 1
