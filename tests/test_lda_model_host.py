"""The float64 model of variational Bayes LDA (tests/lda_model.py) on a CPU: the scheme the device runs is monotone, its bound
is scikit-learn's, it ends where scikit-learn's batch fit ends, and the planted corpus of the GPU monotonicity test leaves the
device's float32 arithmetic a margin of 10.

The small corpus (96 x 80, 2 880 tokens, 4 topics) is for the checks that run scikit-learn or many iterations; its smallest
increase over 60 iterations is far below what float32 resolves, which is why the GPU test runs on the planted corpus of
smoothed_model.py (640 x 480, 25 600 tokens, 8 topics) instead.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import lda_model as lm
import smoothed_model as sm

PRIOR_PAIRS = [(0.25, 0.25), (0.05, 0.01), (0.01, 0.01)]


def start(n, m, k, seed=0):
    rs = np.random.RandomState(seed)
    lam = rs.gamma(100.0, 0.01, (k, m))
    return rs.gamma(100.0, 0.01, (n, k)), lam


@pytest.mark.parametrize("alpha,eta", PRIOR_PAIRS)
def test_the_bound_never_decreases(alpha, eta):
    """Both updates come from one set of responsibilities: exact coordinate ascent.  In float64 a step may lose what the
    summation of the bound loses: 2^-45 of the sum of |terms| is 256 units of 2^-53 for about 10^4 terms."""
    Xd = lm.small_planted()
    gamma, lam = start(*Xd.shape, 4)
    L, scales = [], []
    for _ in range(31):
        f, scale = lm.exact_bound(Xd, gamma, lam, alpha, eta)
        L.append(f)
        scales.append(scale)
        gamma, lam = lm.exact_step(Xd, gamma, lam, alpha, eta)
    steps = np.diff(L)
    print("\nalpha=%g eta=%g: L %.3f -> %.3f over 30 iterations, smallest step %.3g (allowed %.3g)"
          % (alpha, eta, L[0], L[-1], steps.min(), -2.0 ** -45 * max(scales)))
    assert (steps >= -2.0 ** -45 * max(scales)).all()
    assert L[-1] > L[0]


def test_the_bound_is_scikit_learns():
    from sklearn.decomposition import LatentDirichletAllocation
    if not hasattr(LatentDirichletAllocation, "_approx_bound"):
        pytest.skip("this scikit-learn has no LatentDirichletAllocation._approx_bound")
    Xd = lm.small_planted()
    X = sp.csr_matrix(Xd.astype(np.float32))
    n, m = Xd.shape
    worst = 0.0
    for seed, (alpha, eta) in enumerate(PRIOR_PAIRS):
        k = 4 + seed
        rs = np.random.RandomState(seed)
        gamma = (alpha + rs.gamma(1.0, 3.0, (n, k))).astype(np.float32)
        lam = (eta + rs.gamma(1.0, 5.0, (k, m))).astype(np.float32)
        model = LatentDirichletAllocation(n_components=k, doc_topic_prior=alpha, topic_word_prior=eta)
        model._init_latent_vars(m)
        model.components_ = lam.astype(np.float64)
        want = model._approx_bound(X.astype(np.float64), gamma.astype(np.float64), sub_sampling=False)
        got, _, _ = lm.bound64(X, gamma, lam, alpha, eta, round_tables=False)
        worst = max(worst, abs(got - want) / abs(want))
        exact, _ = lm.exact_bound(Xd, gamma.astype(np.float64), lam.astype(np.float64), alpha, eta)
        assert abs(exact - want) <= 1e-8 * abs(want)
    print("\nbound against scikit-learn's _approx_bound: worst relative difference %.3g" % worst)
    assert worst <= 1e-8


def test_the_model_ends_where_scikit_learns_batch_fit_ends():
    """a sanity check between two local optima, not a precision claim: scikit-learn runs up to 100 gamma rounds per sweep, the
    model one"""
    from sklearn.decomposition import LatentDirichletAllocation
    Xd = lm.small_planted()
    alpha, eta, k = 0.25, 0.25, 4
    tokens = Xd.sum()
    gamma, lam = start(*Xd.shape, k)
    for _ in range(300):
        gamma, lam = lm.exact_step(Xd, gamma, lam, alpha, eta)
    ours = lm.exact_bound(Xd, gamma, lam, alpha, eta)[0] / tokens
    model = LatentDirichletAllocation(n_components=k, doc_topic_prior=alpha, topic_word_prior=eta, max_iter=300,
                                      max_doc_update_iter=100, learning_method="batch", random_state=0).fit(Xd)
    theirs = model.score(Xd) / tokens
    print("\nper-token bound after 300 iterations: model %.6f, scikit-learn %.6f" % (ours, theirs))
    assert abs(ours - theirs) <= 0.01


def test_the_planted_corpus_leaves_float32_a_margin_of_ten():
    """What tests/test_lda_em.py's monotonicity test relies on: the model's smallest increase over 30 iterations at
    (alpha, eta) = (0.1, 0.01) is at least 10 times what a float32 trace value may be off by (lda_model.monotone_bound)."""
    X, _, gamma0, lam0 = lm.planted()
    L, ll_scales, scales = lm.planted_trace()
    k = sm.PLANTED["topics"]
    bound = max(lm.monotone_bound(k, X.sum(), a, b, f) for a, b, f in zip(ll_scales, scales, L))
    steps = np.diff(L)
    print("\nplanted corpus: L %.1f -> %.1f, smallest increase %.3f, float32 bound %.3f: margin %.1f"
          % (L[0], L[-1], steps.min(), bound, steps.min() / bound))
    assert steps.min() >= 10 * bound
