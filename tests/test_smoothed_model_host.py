"""CPU-only checks of the float64 model of smoothed (MAP) EM (tests/smoothed_model.py), the reference of tests/test_smoothed_em.py:
without pseudo-counts it is step64, a case of two documents and three words is worked by hand, and its objective never decreases
on the planted corpus -- by a margin that makes the device's monotonicity test meaningful."""
import numpy as np
import scipy.sparse as sp

from smoothed_model import PLANTED, log_prior64, objective64, planted, planted_trace, smoothed_step64
from test_pass_matrix import C_FACTOR, U32, matrix_corpus, step64


def test_without_pseudo_counts_the_model_is_step64():
    X, U, V, sw = matrix_corpus(6)
    for weights in (None, sw):
        plain = step64(X, U, V, 1e-32, weights)
        s = smoothed_step64(X, U, V, 1e-32, 0.0, 0.0, weights)
        for key in ("U", "V", "norm_pwz", "norm_pdz"):
            np.testing.assert_array_equal(s[key], plain[key])
        assert s["ll"] == plain["ll"]
        f, _, scale = objective64(X, U, V, 0.0, 0.0, weights)
        assert f == plain["ll"] and scale == 0.0
        # one side at a time: the other side is the plain update, bit for bit
        np.testing.assert_array_equal(smoothed_step64(X, U, V, 1e-32, 0.5, 0.0, weights)["V"], plain["V"])
        np.testing.assert_array_equal(smoothed_step64(X, U, V, 1e-32, 0.0, 0.05, weights)["U"], plain["U"])
        refit = smoothed_step64(X, U, V, 1e-32, 0.5, 0.05, weights, update_v=False)
        np.testing.assert_array_equal(refit["V"], np.asarray(V, np.float64))


def test_two_documents_three_words_by_hand():
    """U = 1/2 everywhere, V = [[1/2, 1/4, 1/4], [1/4, 1/4, 1/2]], X = [[2, 0, 1], [0, 4, 0]], sw = (1, 1/2), a = 1/2, b = 1/4.
    Responsibilities: word 0 (2/3, 1/3), word 1 (1/2, 1/2), word 2 (1/3, 2/3).
    n_dz = [[5/3, 4/3], [2, 2]], N_d = (3, 4): P(z|d) = [[13/6, 11/6] / 4, [5/2, 5/2] / 5] = [[13/24, 11/24], [1/2, 1/2]].
    n_wz (weighted) = z0: (4/3, 1, 1/3), z1: (2/3, 1, 2/3); N_z = (8/3, 7/3); N_z + 3 b = (41/12, 37/12):
    P(w|z) = [[19, 15, 7] / 41, [11, 15, 11] / 37]."""
    X = sp.csr_matrix(np.array([[2, 0, 1], [0, 4, 0]], np.float32))
    U = np.full((2, 2), 0.5, np.float32)
    V = np.array([[0.5, 0.25, 0.25], [0.25, 0.25, 0.5]], np.float32)
    sw = np.array([1.0, 0.5], np.float32)
    s = smoothed_step64(X, U, V, 1e-32, 0.5, 0.25, sw)
    np.testing.assert_allclose(s["norm_pdz"], [3, 4], rtol=1e-14)
    np.testing.assert_allclose(s["norm_pwz"], [8 / 3, 7 / 3], rtol=1e-14)
    np.testing.assert_allclose(s["U"], [[13 / 24, 11 / 24], [0.5, 0.5]], rtol=1e-14)
    np.testing.assert_allclose(s["V"], [[19 / 41, 15 / 41, 7 / 41], [11 / 37, 15 / 37, 11 / 37]], rtol=1e-14)
    np.testing.assert_allclose(s["U"].sum(1), 1.0, rtol=1e-14)
    np.testing.assert_allclose(s["V"].sum(1), 1.0, rtol=1e-14)
    # F of the starting factors: likelihood 2 log(3/8) + 4 (1/2) log(1/4) + log(3/8), priors a sw_d 2 log(1/2) and b (...)
    f, _, scale = objective64(X, U, V, 0.5, 0.25, sw)
    ll = 3 * np.log(3 / 8) + 2 * np.log(1 / 4)
    prior = 0.5 * (1 + 0.5) * 2 * np.log(0.5) + 0.25 * 2 * (np.log(0.5) + 2 * np.log(0.25))
    np.testing.assert_allclose(f, ll + prior, rtol=1e-14)
    np.testing.assert_allclose(scale, -prior, rtol=1e-14)
    # an empty document gets the prior mean, a zero entry adds nothing to the prior
    X0 = sp.csr_matrix(np.array([[2, 0, 1], [0, 0, 0]], np.float32))
    np.testing.assert_allclose(smoothed_step64(X0, U, V, 1e-32, 0.5, 0.25, sw)["U"][1], [0.5, 0.5], rtol=1e-14)
    Uz = np.array([[1.0, 0.0], [0.5, 0.5]], np.float32)
    np.testing.assert_allclose(log_prior64(Uz, V, 0.5, 0.0)[0], 0.5 * 2 * np.log(0.5), rtol=1e-14)


def test_the_objective_never_decreases_on_the_planted_corpus():
    """30 iterations at a = 0.1, b = 0.01 from the positive random start, weighted: F rises at every one.  The figures the
    device test (test_smoothed_em.py::test_monotone_objective) relies on: the smallest increase against check_ll's bound,
    4 (k + 1) 2^-24 sum x sw max(1, |log dot|), at least tenfold."""
    F, scales = planted_trace()
    steps = np.diff(F)
    bound = C_FACTOR * (PLANTED["topics"] + 1) * U32 * scales.max()
    print("\nplanted corpus: F %.1f -> %.1f, smallest increase %.3f, check_ll bound %.3f" % (F[0], F[-1], steps.min(), bound))
    assert steps.min() > 0
    assert steps.min() >= 10 * bound
    X, X_test, _, _, _ = planted()
    unseen = np.setdiff1d(np.unique(X_test.indices), np.unique(X.indices))
    assert unseen.size > 0                      # what the end-to-end test is for: words the training half never saw
