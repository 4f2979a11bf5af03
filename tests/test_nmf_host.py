"""CPU-only checks of the NMF boundary: the float64 restatement the device tests use (tests/nmf_reference.py) and the two
restated initialisations equal scikit-learn's public estimator exactly; the stop rule of the restated loop; backend
selection (`backend=`, ENSTOP_AMD_NMF, `last_nmf_path`) with the default unchanged.  No device computation here."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
from sklearn.decomposition import NMF

import nmf_reference as R


def _fixture(k, dtype=np.float64):
    X, _ = R.planted_corpus()
    W0, H0 = R.planted_start(X.shape[0], X.shape[1], k)
    return X.astype(dtype), W0.astype(dtype), H0.astype(dtype)


@pytest.mark.parametrize("k", [6, 20, 33, 64])
def test_step64_equals_one_iteration_of_scikit_learn(k):
    X, W0, H0 = _fixture(k)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est = NMF(n_components=k, init="custom", solver="mu", beta_loss=1, max_iter=1, tol=0)
        W = est.fit_transform(X, W=W0.copy(), H=H0.copy())
    Wr, Hr = R.step64(X, W0, H0)
    assert np.abs(W - Wr).max() == 0.0 and np.abs(est.components_ - Hr).max() == 0.0
    assert est.reconstruction_err_ == R.divergence64(X, Wr, Hr)


def test_step64_with_fixed_h_equals_transform():
    from sklearn.decomposition import non_negative_factorization
    from enstop_amd import nmf
    X, _, H0 = _fixture(6)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        W, _, _ = non_negative_factorization(X, H=H0.copy(), n_components=6, update_H=False, beta_loss=1, solver="mu",
                                             max_iter=3, tol=0)
    Wr = nmf.refit_start(X, 6).astype(np.float64)
    assert np.all(Wr == np.sqrt(X.mean() / 6).astype(np.float32))
    Wr = np.full(Wr.shape, np.sqrt(X.mean() / 6))
    for _ in range(3):
        Wr, _ = R.step64(X, Wr, H0, update_H=False)
    assert np.abs(W - Wr).max() == 0.0


@pytest.mark.parametrize("init", ["nndsvd", "random"])
@pytest.mark.parametrize("k", [6, 20])
def test_restated_inits_equal_scikit_learn(init, k):
    from enstop_amd import nmf
    X, _, _ = _fixture(k)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est = NMF(n_components=k, init=init, solver="mu", beta_loss=1, max_iter=1, tol=0, random_state=5)
        W = est.fit_transform(X)
    W0, H0 = nmf.nmf_init(X, k, init, random_state=5)
    assert W0.shape == (X.shape[0], k) and H0.shape == (k, X.shape[1]) and W0.min() >= 0 and H0.min() >= 0
    Wr, Hr = R.step64(X, W0, H0)
    assert np.abs(W - Wr).max() == 0.0 and np.abs(est.components_ - Hr).max() == 0.0


def test_init_tuple_and_bad_inits():
    from enstop_amd import nmf
    X, W0, H0 = _fixture(6)
    a, b = nmf.nmf_init(X, 6, (W0, H0))
    assert a is not None and np.array_equal(a, W0) and np.array_equal(b, H0)
    with pytest.raises(ValueError, match="shapes"):
        nmf.nmf_init(X, 5, (W0, H0))
    with pytest.raises(ValueError, match="init"):
        nmf.nmf_init(X, 6, "nndsvda")


def test_stop_rule_of_the_restated_loop():
    """300 x 120 planted corpus, k = 6, W0, H0 = rand + 0.01 in float32: the restated loop stops at iteration 60, like
    scikit-learn fed float32 and fed float64.  Tested ratios (previous - error) / error_at_init:
    6.2e-1, 2.5e-2, 2.4e-2, 2.0e-3, 2.5e-4, 5.4e-5 -- every one at least 20 % away from tol = 1e-4, so a float32
    implementation whose objective is good to 1e-6 must stop at the same test."""
    X, W0, H0 = _fixture(6, np.float32)
    W, H, n_iter, errors, ratios = R.fit64(X, W0, H0, max_iter=200, tol=1e-4)
    assert n_iter == 60 and len(errors) == 7
    assert np.all(np.abs(ratios - 1e-4) >= 0.2 * 1e-4), ratios
    for dtype in (np.float32, np.float64):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            est = NMF(n_components=6, init="custom", solver="mu", beta_loss=1, max_iter=200, tol=1e-4)
            est.fit_transform(X.astype(dtype), W=W0.astype(dtype), H=H0.astype(dtype))
        assert est.n_iter_ == 60
    assert abs(est.reconstruction_err_ - errors[-1]) <= 1e-12 * errors[-1]


def test_divergence64_edge_cases():
    """stored zeros and x <= EPS32 are left out of both sums; WH below EPS32 is read as EPS32; a negative D gives 0"""
    X = sp.csr_matrix((np.array([2.0, 0.0, 1e-9, 3.0]), np.array([0, 1, 2, 1]), np.array([0, 3, 4])), shape=(2, 3))
    W = np.array([[1.0], [0.0]])
    H = np.array([[2.0, 1.0, 1.0]])
    D, _ = R.divergence64(X, W, H, want_d=True)
    want = 2.0 * np.log(2.0 / 2.0) + 3.0 * np.log(3.0 / R.EPS32) + 4.0 - 5.0
    assert abs(D - want) <= 1e-12 * abs(want)
    assert R.divergence64(sp.csr_matrix(np.array([[1.0]])), np.array([[1.0]]), np.array([[1.0]])) == 0.0


# ---- backend selection ----------------------------------------------------------------------------------------------
def _small():
    X, _ = R.planted_corpus(n=40, m=30, k0=3, length=30)
    return X


def test_default_backend_is_the_host_and_is_reported(monkeypatch):
    from enstop_amd import enstop_
    X = _small()
    monkeypatch.delenv("ENSTOP_AMD_NMF", raising=False)
    enstop_.last_nmf_path = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        T = enstop_.nmf_topics(X, 3, random_state=0)
        assert enstop_.last_nmf_path == "host"
        # exactly what the call computed before the backends existed: scikit-learn on the resampled rows
        rng = np.random.RandomState(0)
        A = X[rng.randint(0, X.shape[0], size=X.shape[0])]
        want = NMF(n_components=3, init="nndsvd", beta_loss=1, alpha_W=0.0, solver="mu", random_state=0).fit(A).components_
        want = np.array(want, dtype=np.float64)
        want /= np.abs(want).sum(axis=1, keepdims=True)
        assert np.array_equal(T, want)
        enstop_.last_nmf_path = None
        S = enstop_.ensemble_of_topics(X, 3, model="nmf", n_runs=2, random_state=0)
        assert enstop_.last_nmf_path == "host" and S.shape == (6, 30) and np.array_equal(S[:3], T)
        monkeypatch.setenv("ENSTOP_AMD_NMF", "host")
        assert np.array_equal(enstop_.nmf_topics(X, 3, random_state=0), T)
        assert np.array_equal(enstop_.nmf_topics(X, 3, random_state=0, backend="host"), T)


def test_bad_backend_values_raise(monkeypatch):
    from enstop_amd import enstop_
    X = _small()
    monkeypatch.setenv("ENSTOP_AMD_NMF", "sometimes")
    with pytest.raises(ValueError, match="ENSTOP_AMD_NMF"):
        enstop_.nmf_topics(X, 3)
    with pytest.raises(ValueError, match="ENSTOP_AMD_NMF"):
        enstop_.ensemble_of_topics(X, 3, model="nmf", n_runs=1)
    with pytest.raises(ValueError, match="backend"):
        enstop_.nmf_topics(X, 3, backend="gpu")


@pytest.mark.parametrize("config", [dict(beta_loss=2), dict(beta_loss="frobenius"), dict(solver="cd", beta_loss=2),
                                    dict(alpha=0.1), dict(init="nndsvda")])
def test_calls_the_device_cannot_carry(monkeypatch, config):
    """host under backend=None whatever the environment selects; ValueError under backend="device", raised before any
    device is looked for (get_engine is made to fail loudly)"""
    from enstop_amd import enstop_, nmf
    from enstop_amd.ensemble import EnsembleTopics

    def no_device(*a, **k):
        raise AssertionError("a device was looked for")
    monkeypatch.setattr(nmf, "get_engine", no_device)
    monkeypatch.setattr(enstop_, "get_engine", no_device)
    X = _small()
    for env in ("auto", "device"):
        monkeypatch.setenv("ENSTOP_AMD_NMF", env)
        enstop_.last_nmf_path = None
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            enstop_.nmf_topics(X, 3, random_state=0, **config)
        assert enstop_.last_nmf_path == "host"
    with pytest.raises(ValueError, match="device"):
        enstop_.nmf_topics(X, 3, backend="device", **config)
    with pytest.raises(ValueError, match="device"):
        enstop_.ensemble_of_topics(X, 3, model="nmf", n_runs=1, nmf_backend="device", **config)
    assert EnsembleTopics(nmf_backend="device").get_params()["nmf_backend"] == "device"
    assert EnsembleTopics().nmf_backend is None


def test_without_a_library_or_a_gpu(monkeypatch):
    """a configuration the device could carry, but no engine can be had: the host under "auto" and under "device" from the
    environment, ValueError when the device backend was passed explicitly"""
    from enstop_amd import enstop_, nmf

    def no_gpu(*a, **k):
        raise RuntimeError("no HIP device")
    monkeypatch.setattr(nmf, "get_engine", no_gpu)
    X = _small()
    for env in ("auto", "device"):
        monkeypatch.setenv("ENSTOP_AMD_NMF", env)
        enstop_.last_nmf_path = None
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            T = enstop_.nmf_topics(X, 3, random_state=0)
        assert enstop_.last_nmf_path == "host" and T.shape == (3, 30)
    with pytest.raises(ValueError, match="GPU"):
        enstop_.nmf_topics(X, 3, random_state=0, backend="device")
    with pytest.raises(ValueError, match="GPU"):
        enstop_.ensemble_of_topics(X, 3, model="nmf", n_runs=1, nmf_backend="device")


def test_device_obstacles_accept_the_reference_configuration():
    from enstop_amd import nmf
    assert nmf.device_obstacle() is None
    assert nmf.device_obstacle(init="random", beta_loss="kullback-leibler", solver="mu", alpha=0) is None
    assert nmf.device_obstacle(init=(np.ones((2, 1)), np.ones((1, 2)))) is None
    assert "beta_loss" in nmf.device_obstacle(beta_loss=0)


def test_reference_recovers_the_end_to_end_corpus():
    """the corpus of test_nmf_device.py's end-to-end test: scikit-learn's members and the host combiner find a stable
    topic within Hellinger 0.1 of every planted topic (test_kl_pipeline_recovers_planted_clusters' criterion)"""
    from enstop_amd import enstop_, ensemble
    X, topics = R.planted_corpus(length=R.E2E_LENGTH)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        S = enstop_.ensemble_of_topics(X, 6, model="nmf", n_runs=8, random_state=0, init="random", nmf_backend="host")
    stable = ensemble.generate_combined_topics_hellinger(S, 3, 5)
    planted = topics.copy()
    planted[:, 11] = 0
    D = ensemble.all_pairs_hellinger_distance(np.vstack([planted, stable]))[:6, 6:]
    assert np.all(D.min(axis=1) < 0.08) and len(set(D.argmin(axis=1))) == 6, D.min(axis=1)
