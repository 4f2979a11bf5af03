"""The topic metrics of the LDA estimator on a CPU.  `LDA.components_` is lambda, whose rows do not sum to 1, and
utils.mean_log_lift scores the topics as given: the estimator's coherence() and log_lift() therefore read `topic_word_`, the
normalised rows.  Hand-set fitted attributes, no device."""
import numpy as np
import pytest
import scipy.sparse as sp

from enstop_amd import LDA, PLSA, utils


@pytest.fixture(scope="module")
def fitted():
    rs = np.random.RandomState(4)
    X = sp.csr_matrix(rs.poisson(0.3, (60, 40)).astype(np.float32))
    lam = (0.01 + rs.gamma(1.0, 7.0, (5, 40))).astype(np.float32)          # row sums of a few hundred, not 1
    model = LDA(n_components=5)
    model.components_ = lam
    model.topic_word_ = lam / lam.sum(axis=1, keepdims=True)
    model.training_data_ = X
    return model, X


@pytest.mark.parametrize("n_words", [10, 20])
def test_log_lift_scores_the_normalised_topics(fitted, n_words):
    model, X = fitted
    assert np.abs(model.components_.sum(1) - 1).min() > 10
    each = [model.log_lift(z, n_words=n_words) for z in range(5)]
    mean = model.log_lift(n_words=n_words)
    np.testing.assert_allclose(mean, np.mean(each), rtol=1e-6)
    np.testing.assert_allclose(mean, utils.mean_log_lift(model.topic_word_, X, n_words), rtol=1e-12)
    for z in range(5):
        np.testing.assert_allclose(each[z], utils.log_lift(model.topic_word_, z, X, n_words), rtol=1e-12)
    # what the unnormalised table would have given is off by the mean log row sum, far outside that tolerance
    assert abs(utils.mean_log_lift(model.components_, X, n_words) - mean) > 1.0


def test_coherence_scores_the_normalised_topics(fitted):
    model, X = fitted
    each = [model.coherence(z, n_words=10) for z in range(5)]
    np.testing.assert_allclose(model.coherence(n_words=10), np.mean(each), rtol=1e-12)
    np.testing.assert_allclose(model.coherence(n_words=10), utils.mean_coherence(model.topic_word_, X, n_words=10), rtol=1e-12)
    with pytest.raises(ValueError):
        model.coherence(topic_num=5)
    with pytest.raises(ValueError):
        model.log_lift(topic_num="a")


def test_the_plsa_estimators_still_score_components(fitted):
    _, X = fitted
    rs = np.random.RandomState(5)
    T = rs.rand(3, 40) + 0.05
    T /= T.sum(1, keepdims=True)
    model = PLSA(n_components=3)
    model.components_, model.training_data_ = T, X
    np.testing.assert_allclose(model.log_lift(n_words=10), utils.mean_log_lift(T, X, 10), rtol=1e-12)
    np.testing.assert_allclose(model.coherence(1, n_words=10), utils.coherence(T, 1, X, n_words=10), rtol=1e-12)
