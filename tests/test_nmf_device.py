"""Kullback-Leibler NMF on the device (include/plsa_hip_nmf.h) against the float64 restatement of scikit-learn's
multiplicative updates in tests/nmf_reference.py (pinned to scikit-learn by tests/test_nmf_host.py).

Error model of the half-iterations (the one of tests/test_pass_matrix.py; u = 2^-24, L the longest row for W, the longest
column for H).  An updated entry is  f * (N / S)  with  N = sum_j q_j r_j  over at most L entries, q_j = x_j / max(dot_j, EPS32)
and dot_j a k-term float32 sum of non-negative products.  Every sum adds non-negative terms, so a float32 sum of t terms
carries a relative error of at most t u whatever its order: dot_j (1 + k u), q_j one more division, N another L + 1, S
(H_sum / W_sum) is a float64 sum rounded once, the final quotient and product two more:  (L + k + 6) u  in all, held to
    |got - want| <= 4 (L + k) u |want|,
and got == 0 exactly where want == 0 (zero factors, empty rows and columns).  The fixtures keep every (WH) a factor 2 away
from EPS32 unless it is exactly 0 and every updated H a factor 2 away from float64 eps, asserted on the reference, so
the clamps fall on the same side in both precisions.  The objective: the float64 sums add x log(x / wh) with wh good to
(k + 1) u relative, i.e. |got - want| <= 4 (k + 1) u sum x max(1, |log(x / wh)|) on D.
"""
import warnings

import numpy as np
import pytest

import nmf_reference as R
from conftest import peak_rel

pytestmark = pytest.mark.gpu
U24 = 2.0 ** -24
KS = (3, 6, 20, 33, 64, 130, 300)


@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_half(got, want, L, k, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(got == 0, want == 0), what
    err = np.abs(got - want)
    bound = 4.0 * (L + k) * U24 * np.abs(want)
    worst = float((err[want != 0] / bound[want != 0]).max())
    print("%s: worst error / bound = %.3f (bound %.2e relative)" % (what, worst, 4.0 * (L + k) * U24))
    assert np.all(err <= bound), (what, worst)


def _assert_fixture_margins(details, H_new):
    for wh in details["wh"]:
        assert np.all((wh == 0) | (wh >= 2 * R.EPS32))
    Hu = details["H_unclamped"]
    assert np.all((Hu == 0) | (Hu >= 2 * R.EPS64)) and np.array_equal(Hu, H_new)


def _halves(eng, X, W0, H0):
    """both half-iterations from (W0, H0): (W after the W half, H after the H half, kernel names, pass info)"""
    eng.upload_csr(X)
    eng.nmf_set_factors(W0, H0)
    Wg, Hg = eng.nmf_get_factors()
    assert np.array_equal(_bits(Wg), _bits(W0)) and np.array_equal(_bits(Hg), _bits(H0))      # stored and returned unchanged
    eng.timing(True)
    eng.timing_reset()
    eng.nmf_update_w()
    W1, _ = eng.nmf_get_factors(want_h=False)
    eng.nmf_update_h()
    W1b, H1 = eng.nmf_get_factors()
    names = set(eng.timing_report())
    eng.timing(False)
    assert np.array_equal(_bits(W1), _bits(W1b))
    return W1, H1, names, eng.pass_info(), eng.packed_info()


@pytest.mark.parametrize("k", KS)
def test_half_iterations_entry_for_entry(amd, k, monkeypatch):
    X, W0, H0 = R.edge_corpus(k)
    L_row, L_col = int(np.diff(X.indptr).max()), int(np.diff(X.tocsc().indptr).max())
    assert L_row > 64 and L_col > 256 and np.diff(X.indptr)[5] == 0 and (X.data == 0).sum() >= 20
    with amd.Engine() as eng:
        W1, H1, names, info, packed = _halves(eng, X, W0, H0)
        assert {"k_nmf_row_pass", "k_nmf_col_pass", "k_nmf_h_finish", "k_col_reduce"} <= names and "k_nmf_row_reduce" not in names
        assert packed == dict(csr="packed", csc="packed")
        print("k = %d: passes %s" % (k, info))
        # two runs give the same bits (same context, from the same start)
        W1r, H1r, _, _, _ = _halves(eng, X, W0, H0)
        assert np.array_equal(_bits(W1), _bits(W1r)) and np.array_equal(_bits(H1), _bits(H1r))
    details = {}
    Ww, _ = R.step64(X, W0, H0, update_H=False)
    _check_half(W1, Ww, L_row, k, "W half, k = %d" % k)
    _, Hw = R.step64(X, W0, H0, details=details)
    # the H half against step64 from the W the device returned
    d2 = {}
    _, Hw_dev = R.step64_h(X, W1, H0, details=d2)
    _assert_fixture_margins(dict(wh=details["wh"] + d2["wh"], H_unclamped=d2["H_unclamped"]), Hw_dev)
    _check_half(H1, Hw_dev, L_col, k, "H half, k = %d" % k)
    if k >= 3:
        assert not W1[:, 1].any() and not H1[1].any() and not H1[2].any() and not W1[3].any()
    # PLSA_PACKED=0: the two-array streams, the same bits
    monkeypatch.setenv("PLSA_PACKED", "0")
    with amd.Engine() as eng:
        W1a, H1a, _, _, packed = _halves(eng, X, W0, H0)
    assert packed == dict(csr="arrays", csc="arrays")
    assert np.array_equal(_bits(W1), _bits(W1a)) and np.array_equal(_bits(H1), _bits(H1a))


@pytest.mark.parametrize("k", (20, 64, 130))
def test_wide_gathers_give_the_same_bits(amd, k, monkeypatch):
    """PLSA_FORCE_WIDE=1: 64-bit gather addresses and run-time kp in both passes and in the objective (read back from
    pass_info), the same operations: the bits of the narrow instantiations"""
    X, W0, H0 = R.edge_corpus(k)

    def run():
        with amd.Engine() as eng:
            W1, H1, _, info, _ = _halves(eng, X, W0, H0)
            return W1, H1, eng.nmf_divergence(), info
    W1, H1, d1, info = run()
    assert not info["row_wide"] and not info["col_wide"]
    monkeypatch.setenv("PLSA_FORCE_WIDE", "1")
    W2, H2, d2, info = run()
    assert info["row_wide"] and info["col_wide"]
    assert np.array_equal(_bits(W1), _bits(W2)) and np.array_equal(_bits(H1), _bits(H2)) and d1 == d2


@pytest.mark.parametrize("k", (6, 64))
def test_row_item_mode(amd, k):
    """12 documents of 3000 entries: the document pass runs over row items (read back from the kernels that ran)"""
    X, W0, H0 = R.long_rows_corpus(k)
    with amd.Engine() as eng:
        W1, H1, names, info, _ = _halves(eng, X, W0, H0)
        assert "k_nmf_row_reduce" in names, names
        eng.nmf_set_factors(W0, H0)
        got = eng.nmf_divergence()              # (document-owned in this mode as well)
        # H fixed: the driver steps one iteration at a time here and equals the entry point called by hand
        eng.nmf_set_factors(W0, H0)
        n_iter, errors = eng.nmf_fit(update_h=False, max_iter=3, tol=0.0)
        Wf, _ = eng.nmf_get_factors(want_h=False)
        eng.nmf_set_factors(W0, H0)
        for _ in range(3):
            eng.nmf_update_w()
        Wm, _ = eng.nmf_get_factors(want_h=False)
    assert n_iter == 3 and len(errors) == 1 and np.array_equal(_bits(Wf), _bits(Wm))
    Ww, _ = R.step64(X, W0, H0, update_H=False)
    _check_half(W1, Ww, 3000, k, "row items, W half, k = %d" % k)
    d1, d2 = {}, {}
    R.step64(X, W0, H0, update_H=False, details=d1)
    _, Hw = R.step64_h(X, W1, H0, details=d2)
    _assert_fixture_margins(dict(wh=d1["wh"] + d2["wh"], H_unclamped=d2["H_unclamped"]), Hw)
    _check_half(H1, Hw, int(np.diff(X.tocsc().indptr).max()), k, "row items, H half, k = %d" % k)
    D, scale = R.divergence64(X, W0, H0, want_d=True)
    assert abs(got * got / 2.0 - D) <= 4.0 * (k + 1) * U24 * scale


@pytest.mark.parametrize("k", KS)
def test_divergence(amd, k):
    X, W0, H0 = R.edge_corpus(k)
    with amd.Engine() as eng:
        eng.upload_csr(X)
        eng.nmf_set_factors(W0, H0)
        got = eng.nmf_divergence()
        again = eng.nmf_divergence()
    D, scale = R.divergence64(X, W0, H0, want_d=True)
    assert D > 0 and got == again
    got_d = got * got / 2.0
    bound = 4.0 * (k + 1) * U24 * scale
    print("k = %d: D = %.6e, device %.6e, error / bound = %.3f" % (k, D, got_d, abs(got_d - D) / bound))
    assert abs(got_d - D) <= bound
    assert abs(got - R.divergence64(X, W0, H0)) <= bound / got


@pytest.mark.parametrize("update_h", (1, 0))
@pytest.mark.parametrize("k", (6, 33))
def test_driver_one_iteration_at_a_time(amd, k, update_h):
    """plsa_nmf_fit with max_iter = 1 .. 12 from the same start: every iterate equals, bit for bit, the half-iteration
    entry points called by hand; errors = error_at_init + one entry per tenth iteration.  tol = 1e-30 keeps the tests on
    (scikit-learn evaluates the objective only when tol > 0) without ever stopping a loop whose objective still falls."""
    X, W0, H0 = R.edge_corpus(k)
    with amd.Engine() as eng:
        eng.upload_csr(X)
        eng.nmf_set_factors(W0, H0)
        e0 = eng.nmf_divergence()
        by_hand, e10 = [], None
        for it in range(1, 13):
            eng.nmf_update_w()
            if update_h:
                eng.nmf_update_h()
            by_hand.append(eng.nmf_get_factors())
            if it == 10:
                e10 = eng.nmf_divergence()
        for max_iter in range(1, 13):
            eng.nmf_set_factors(W0, H0)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                n_iter, errors = eng.nmf_fit(update_h=bool(update_h), max_iter=max_iter, tol=1e-30)
            W, H = eng.nmf_get_factors()
            assert n_iter == max_iter
            assert np.array_equal(_bits(W), _bits(by_hand[max_iter - 1][0])), max_iter
            assert np.array_equal(_bits(H), _bits(by_hand[max_iter - 1][1])), max_iter
            assert list(errors) == ([e0, e10] if max_iter >= 10 else [e0]), (max_iter, errors, e0, e10)
        if not update_h:
            assert np.array_equal(_bits(by_hand[-1][1]), _bits(H0))


def test_status_codes(amd):
    X, W0, H0 = R.edge_corpus(6)
    with amd.Engine() as eng:
        with pytest.raises(amd.DeviceError, match="corpus"):
            eng.nmf_update_w()
        eng.upload_csr(X)
        with pytest.raises(amd.DeviceError, match="factors"):
            eng.nmf_divergence()
        with pytest.raises(amd.DeviceError, match="1024"):
            eng.nmf_set_factors(np.ones((X.shape[0], 1025), np.float32), np.ones((1025, X.shape[1]), np.float32))
        eng.nmf_set_factors(W0, H0)
        with pytest.raises(amd.DeviceError, match="max_iter"):
            eng.nmf_fit(max_iter=0)
        W, H = eng.nmf_get_factors()
        assert np.array_equal(W, W0) and np.array_equal(H, H0)


def _stop_fixture():
    X, _ = R.planted_corpus()
    W0, H0 = R.planted_start(X.shape[0], X.shape[1], 6)
    return X, W0, H0


def test_stop_rule(amd):
    from sklearn.exceptions import ConvergenceWarning
    X, W0, H0 = _stop_fixture()
    Ww, Hw, n_want, e_want, ratios = R.fit64(X, W0, H0)
    assert n_want == 60 and len(e_want) == 7 and np.all(np.abs(ratios - 1e-4) >= 0.2e-4)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        W, H, n_iter = amd.nmf_fit(X, 6, init=(W0, H0))
    assert not [w for w in caught if issubclass(w.category, ConvergenceWarning)]
    with amd.Engine() as eng:
        eng.upload_csr(X)
        eng.nmf_set_factors(W0, H0)
        n2, errors = eng.nmf_fit()
    print("n_iter %d, errors %s, peak_rel W %.2e H %.2e" % (n_iter, errors, peak_rel(W, Ww), peak_rel(H, Hw)))
    assert n_iter == 60 and n2 == 60 and len(errors) == 7
    np.testing.assert_allclose(errors, e_want, rtol=1e-5)
    assert peak_rel(W, Ww) <= 1e-4 and peak_rel(H, Hw) <= 1e-4
    with pytest.warns(ConvergenceWarning):
        _, _, n_iter = amd.nmf_fit(X, 6, init=(W0, H0), max_iter=20, tol=1e-12)
    assert n_iter == 20


def test_tol_zero_runs_to_max_iter(amd):
    """tol = 0: no test is ever made; the loop runs to max_iter (scikit-learn warns only when tol > 0)"""
    X, W0, H0 = _stop_fixture()
    with amd.Engine() as eng:
        eng.upload_csr(X)
        eng.nmf_set_factors(W0, H0)
        n_iter, errors = eng.nmf_fit(max_iter=70, tol=0.0)
        W, H = eng.nmf_get_factors()
    assert n_iter == 70 and len(errors) == 1
    Ww, Hw, n_want, _, _ = R.fit64(X, W0, H0, max_iter=70, tol=0)
    assert n_want == 70 and peak_rel(W, Ww) <= 1e-4 and peak_rel(H, Hw) <= 1e-4
    from sklearn.exceptions import ConvergenceWarning
    with pytest.warns(ConvergenceWarning):
        amd.nmf_refit(X, H, max_iter=10, tol=1e-12)


def test_refit_against_the_float64_loop(amd):
    """H fixed (the combined pass: ten iterations per launch).  tol = 2e-4: the float64 loop's tested ratios are 6.3e-2,
    2.7e-3, 7.0e-4, 2.5e-4, 1.1e-4 -- each at least 20 % away from it -- so it stops at 50 and so must the device."""
    X, W0, H0 = _stop_fixture()
    start = np.full((X.shape[0], 6), np.sqrt(X.mean() / 6), np.float32)
    Ww, _, n_want, _, ratios = R.fit64(X, start, H0, update_H=False, tol=2e-4)
    assert n_want == 50 and np.all(np.abs(ratios - 2e-4) >= 0.2 * 2e-4), ratios
    W, n_iter = amd.nmf_refit(X, H0, tol=2e-4)
    print("refit: n_iter %d, peak_rel %.2e" % (n_iter, peak_rel(W, Ww)))
    assert n_iter == 50 and peak_rel(W, Ww) <= 1e-4


def test_plsa_after_nmf_and_nmf_after_plsa_equal_fresh_contexts(amd):
    X, W0, H0 = R.edge_corpus(20)
    kw = dict(n_iter=12, n_iter_per_test=5, tolerance=0.0, e_step_thresh=1e-16, random_state=3)

    def plsa(eng):
        from enstop_amd.plsa import _fit_on_engine
        _fit_on_engine(eng, 20, None, "random", kw["n_iter"], kw["n_iter_per_test"], kw["tolerance"], kw["e_step_thresh"],
                       kw["random_state"], None)
        return eng.get_factors()

    def nmf(eng):
        eng.nmf_set_factors(W0, H0)
        eng.nmf_fit(max_iter=12, tol=1e-30)
        return eng.nmf_get_factors()

    with amd.Engine() as eng:
        eng.upload_csr(X)
        p_fresh = plsa(eng)
        n_after = nmf(eng)
        p_after = plsa(eng)
    with amd.Engine() as eng:
        eng.upload_csr(X)
        n_fresh = nmf(eng)
    for a, b in ((p_fresh, p_after), (n_fresh, n_after)):
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


def test_members_with_distinct_draws_share_one_context(amd):
    """_ensemble_of_nmf_topics: one upload, successive bootstrap resamples with DIFFERENT draws on one context (a
    RandomState instance continues its stream from member to member); every member equals the same member fitted on a
    context of its own, and the context is left on the corpus."""
    from enstop_amd import enstop_
    from enstop_amd.engine import get_engine
    from enstop_amd.utils import normalize
    X, _ = R.planted_corpus()
    kw = dict(init="random", bootstrap=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        S = enstop_.ensemble_of_topics(X, 6, model="nmf", n_runs=3, random_state=np.random.RandomState(3),
                                       nmf_backend="device", **kw)
        assert enstop_.last_nmf_path == "device" and S.shape == (18, X.shape[1])
        assert get_engine().shape[:2] == X.shape and get_engine().shape[2] == X.nnz       # base restored
        rs = np.random.RandomState(3)
        for r in range(3):
            with amd.Engine() as eng:
                eng.upload_csr(X)
                Hm = np.array(enstop_._nmf_topics_on_engine(eng, X, 6, dict(kw, random_state=rs)), dtype=np.float64, order="C")
            normalize(Hm, axis=1)                    # (the package's own: a sequential float64 marginal)
            assert np.array_equal(S[6 * r:6 * r + 6], Hm), r
    assert not np.array_equal(S[:6], S[6:12]) and not np.array_equal(S[6:12], S[12:])


def test_ensemble_topics_end_to_end(amd):
    from enstop_amd import enstop_, ensemble
    X, topics = R.planted_corpus(length=R.E2E_LENGTH)
    enstop_.last_nmf_path = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = amd.EnsembleTopics(n_components=6, model="nmf", n_starts=8, topic_combination="hellinger",
                                   nmf_backend="device", random_state=0).fit(X)
        assert enstop_.last_nmf_path == "device"
        W, _ = amd.nmf_refit(X, model.components_)
    assert np.abs(model.components_.sum(axis=1) - 1.0).max() < 1e-5
    planted = topics.copy()
    planted[:, 11] = 0
    D = ensemble.all_pairs_hellinger_distance(np.vstack([planted, model.components_]))[:6, 6:]
    print("Hellinger distance of every planted topic to its stable topic:", D.min(axis=1))
    assert np.all(D.min(axis=1) < 0.1) and len(set(D.argmin(axis=1))) == 6
    assert model.embedding_.shape == (X.shape[0], model.components_.shape[0])
    assert np.array_equal(_bits(model.embedding_), _bits(W))
    # the default is still scikit-learn's
    enstop_.last_nmf_path = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enstop_.nmf_topics(X, 6, random_state=0)
    assert enstop_.last_nmf_path == "host"
