"""EnsembleTopics with every default -- topic_combination="hellinger_umap", the reference's own default (enstop_.py:427,
719) -- on the planted corpus of test_planted_topics.py, held to that file's bounds for the other two combiners.  The
embedding is the native one (Engine.hellinger_embedding); umap-learn is not involved.  Needs a real MI355X (-m gpu)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K0 = 8


@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


@pytest.fixture(scope="module")
def planted(amd):
    with amd.Engine() as eng:
        eng.generate_synthetic(6000, 3000, 330_000, seed=3, topics=K0, alpha=0.05, background=0.1)
        X = eng.download_active_csr()
        labels = eng.synthetic_dominant_topics()
    X = X.astype(np.int64)
    assert labels.shape == (X.shape[0],) and set(np.unique(labels)) == set(range(K0))
    return X, labels


def matched_accuracy(assign, labels, n_found):
    from scipy.optimize import linear_sum_assignment
    C = np.zeros((n_found, K0), np.int64)
    np.add.at(C, (assign, labels), 1)
    r, c = linear_sum_assignment(-C)
    return C[r, c].sum() / float(len(labels)), dict(zip(r.tolist(), c.tolist()))


def estimator(amd):
    return amd.EnsembleTopics(n_components=12, n_starts=12, n_iter=60, min_samples=3, min_cluster_size=5, n_jobs=4,
                              random_state=1)


@pytest.fixture(scope="module")
def fitted(amd, planted):
    et = estimator(amd)
    assert et.topic_combination == "hellinger_umap"
    return et, et.fit_transform(planted[0])


def test_the_default_combination_finds_the_planted_topics(amd, planted, fitted):
    X, labels = planted
    et, emb = fitted
    m_found = et.n_components_
    info = amd.engine.get_engine(None).last_embedding_info
    print("stable topics %d, embedding %s" % (m_found, info))
    assert info is not None and info["t"] == 12 * 12 and info["n_epochs"] == 500
    assert et.components_.shape == (m_found, X.shape[1]) and emb.shape == (X.shape[0], m_found)
    np.testing.assert_allclose(et.components_.sum(axis=1), 1.0, atol=1e-3)
    acc, match = matched_accuracy(emb.argmax(axis=1), labels, m_found)
    print("accuracy %.4f, match %s" % (acc, match))
    assert K0 <= m_found <= K0 + 3, m_found
    assert len(set(match.values())) == K0 and acc > 0.8, (acc, match)


def test_two_fits_give_identical_components(amd, planted, fitted):
    again = estimator(amd).fit(planted[0])
    np.testing.assert_array_equal(again.components_, fitted[0].components_)
