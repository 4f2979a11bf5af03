"""CPU-only checks of enstop_amd/scoring.py: the document split, the composition of held_out_scores (against a fake engine
with canned per-document rows: which documents are scored, both on_zero modes, the perplexity from the sums, one hold of
the engine lock) and the estimator surface."""
import numpy as np
import pytest
import scipy.sparse as sp


def _counts(seed=0, n=60, m=40, dtype=np.float32):
    rs = np.random.RandomState(seed)
    X = sp.random(n, m, density=0.2, format="csr", random_state=rs, dtype=np.float64)
    X.data = np.ceil(X.data * 6)
    return X.astype(dtype)


# ------------------------------------------------------------------------------------------------
# split_documents
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int64])
def test_split_halves_sum_to_x_exactly_and_integer_data_stays_integer(dtype):
    from enstop_amd import split_documents
    X = _counts(1, dtype=dtype)
    a, b = split_documents(X, 0.5, random_state=3)
    assert a.shape == X.shape and b.shape == X.shape and a.dtype == X.dtype and b.dtype == X.dtype
    assert ((a + b) != X).nnz == 0
    for half in (a, b):
        assert sp.isspmatrix_csr(half)
        assert (half.data != 0).all() and (half.data > 0).all()            # no stored zeros
        assert (half.data == np.floor(half.data)).all()                     # token by token: counts stay counts
    assert 0 < a.sum() < X.sum()
    # thinned token by token, not entry by entry: some entry is divided between the halves
    assert a.multiply(b).nnz > 0


def test_split_is_one_binomial_call_in_csr_order():
    from enstop_amd import split_documents
    X = _counts(2)
    a, b = split_documents(X, 0.3, random_state=11)
    drawn = np.random.RandomState(11).binomial(X.data.astype(np.int64), 0.3)
    want = sp.csr_matrix((drawn.astype(X.dtype), X.indices, X.indptr), shape=X.shape)
    assert (a != want).nnz == 0 and (b != X - want).nnz == 0


def test_split_same_seed_same_split_other_seed_other_split():
    from enstop_amd import split_documents
    X = _counts(3)
    a1, b1 = split_documents(X, 0.5, random_state=5)
    a2, b2 = split_documents(X, 0.5, random_state=5)
    a3, _ = split_documents(X, 0.5, random_state=6)
    assert (a1 != a2).nnz == 0 and (b1 != b2).nnz == 0
    assert (a1 != a3).nnz > 0
    rng = np.random.RandomState(5)                                        # a RandomState is drawn from, not re-seeded
    a4, _ = split_documents(X, 0.5, random_state=rng)
    assert (a1 != a4).nnz == 0
    a5, _ = split_documents(X, 0.5, random_state=rng)
    assert (a1 != a5).nnz > 0


def test_split_of_fractional_data_assigns_whole_entries():
    from enstop_amd import split_documents
    X = _counts(4, dtype=np.float64)
    X.data = X.data + 0.25
    a, b = split_documents(X, 0.5, random_state=0)
    assert ((a + b) != X).nnz == 0
    assert a.multiply(b).nnz == 0 and a.nnz + b.nnz == X.nnz
    take = np.random.RandomState(0).rand(X.nnz) < 0.5
    assert a.nnz == int(take.sum())
    assert (a.data != 0).all() and (b.data != 0).all()


@pytest.mark.parametrize("integer", [True, False])
def test_split_fraction_zero_and_one_give_an_empty_half(integer):
    from enstop_amd import split_documents
    X = _counts(5, dtype=np.float64)
    if not integer:
        X.data = X.data + 0.5
    a, b = split_documents(X, 0.0, random_state=1)
    assert a.nnz == 0 and (b != X).nnz == 0
    a, b = split_documents(X, 1.0, random_state=1)
    assert b.nnz == 0 and (a != X).nnz == 0
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            split_documents(X, bad)


def test_split_eliminates_stored_zeros_of_x_and_rejects_negative_entries():
    from enstop_amd import split_documents
    X = _counts(6)
    X.data[::7] = 0
    a, b = split_documents(X, 0.5, random_state=2)
    assert (a.data != 0).all() and (b.data != 0).all() and ((a + b) != X).nnz == 0
    X.data[3] = -1
    with pytest.raises(ValueError):
        split_documents(X, 0.5)


# ------------------------------------------------------------------------------------------------
# held_out_scores against a fake engine
# ------------------------------------------------------------------------------------------------
class _CountingLock:
    def __init__(self):
        self.holds, self.depth = 0, 0

    def __enter__(self):
        self.holds += 1
        self.depth += 1

    def __exit__(self, *exc):
        self.depth -= 1


class FakeEngine:
    """records the calls; score_rows returns canned rows: ll = -2 tokens, every token of the words in `zero_words` unscored"""

    def __init__(self, zero_words=()):
        self.lock = _CountingLock()
        self.calls = []
        self.zero_words = np.asarray(zero_words, np.int64)
        self.resident = None

    def _held(self, name):
        assert self.lock.depth == 1, "%s outside the engine lock" % name
        self.calls.append(name)

    def upload_csr(self, X):
        self._held("upload_csr")
        self.resident = X.copy()
        return self

    def set_factors(self, U, V=None):
        self._held("set_factors")
        self.U = np.asarray(U)
        return self

    def init_factors_numpy_stream(self, k, rng, topics=None):
        self._held("set_factors")
        rng.rand(self.resident.shape[0], k)
        return self

    def refit(self, sw, n_iter, n_iter_per_test, tolerance, thresh, flags, trace=False):
        self._held("refit")
        self.refit_args = (sw, n_iter, n_iter_per_test, tolerance, flags)
        return 7, np.zeros(0, np.float32)

    def get_factors(self, *a, **kw):
        raise AssertionError("no factor may be downloaded between the fold-in and the scoring")

    def score_rows(self, other=None, sample_weight=None):
        self._held("score_rows")
        M = (self.resident if other is None else other).tocsr().astype(np.float64)
        self.scored_matrix = M.copy()
        zero = np.zeros(M.shape[1], bool)
        zero[self.zero_words] = True
        unscored = np.asarray(M[:, zero].sum(1)).ravel()
        tokens = np.asarray(M[:, ~zero].sum(1)).ravel()
        return -2.0 * tokens, tokens, unscored


@pytest.fixture
def fake(monkeypatch):
    from enstop_amd import scoring

    def install(**kw):
        eng = FakeEngine(**kw)
        monkeypatch.setattr(scoring, "get_engine", lambda device=None: eng)
        return eng
    return install


def _corpus_with_edge_documents():
    X = _counts(7, n=40, m=30).tolil()
    X[0, :] = 0                      # empty document
    X[1, :] = 0
    X[1, 4] = 1                      # one token: one of its halves is empty whatever the draw
    return X.tocsr()


def test_completion_composes_split_fold_in_and_scoring_under_one_hold_of_the_lock(fake):
    from enstop_amd import held_out_scores, split_documents
    eng = fake()
    X = _corpus_with_edge_documents()
    topics = np.full((3, X.shape[1]), 1.0 / X.shape[1], np.float32)
    out = held_out_scores(X, topics, method="completion", fraction=0.5, random_state=9)
    assert eng.lock.holds == 1 and eng.lock.depth == 0
    assert eng.calls == ["upload_csr", "set_factors", "refit", "score_rows"]
    observed, held = split_documents(X, 0.5, np.random.RandomState(9))
    assert (eng.resident != observed).nnz == 0                      # the fold-in ran on the observed half ...
    assert (eng.scored_matrix != held).nnz == 0                     # ... and the held-out half was scored against it
    assert eng.refit_args == (None, 50, 5, 0.001, None)             # transform's iteration defaults
    assert out["n_iter"] == 7
    # the starting P(z|d) comes from the same stream, after the split's draws
    rng = np.random.RandomState(9)
    split_documents(X, 0.5, rng)
    U0 = rng.rand(X.shape[0], 3)
    U0 /= U0.sum(1, keepdims=True)
    np.testing.assert_array_equal(eng.U, U0.astype(np.float32))
    # documents with an empty half are not scored
    want = (np.diff(observed.indptr) > 0) & (np.diff(held.indptr) > 0)
    np.testing.assert_array_equal(out["scored_documents"], want)
    assert out["scored_documents"].dtype == bool
    assert not out["scored_documents"][0] and not out["scored_documents"][1] and 5 < want.sum() < X.shape[0]
    for key in ("log_likelihood", "tokens", "unscored"):
        assert out[key].shape == (X.shape[0],) and out[key].dtype == np.float64
    sel = out["scored_documents"]
    assert out["perplexity"] == float(np.exp(-np.sum(out["log_likelihood"][sel]) / np.sum(out["tokens"][sel])))
    assert abs(out["perplexity"] - np.exp(2.0)) < 1e-12
    assert set(out) == {"log_likelihood", "tokens", "unscored", "scored_documents", "perplexity", "n_iter"}


def test_perplexity_leaves_out_the_unscored_documents_sums(fake):
    """an unscored document's rows are in the dict but not in the perplexity: give it a different canned likelihood"""
    from enstop_amd import held_out_scores
    eng = fake()
    X = _corpus_with_edge_documents()
    rows = eng.score_rows.__func__

    def skewed(self, other=None, sample_weight=None):
        ll, tokens, unscored = rows(self, other, sample_weight)
        ll[1] = -1000.0 * max(tokens[1], 1.0)
        tokens[1] = max(tokens[1], 1.0)
        return ll, tokens, unscored
    eng.score_rows = skewed.__get__(eng)
    out = held_out_scores(X, np.ones((2, X.shape[1]), np.float32), random_state=1)
    assert not out["scored_documents"][1] and out["log_likelihood"][1] <= -1000.0
    assert abs(out["perplexity"] - np.exp(2.0)) < 1e-12


def test_fold_in_scores_the_resident_matrix(fake):
    from enstop_amd import held_out_scores
    eng = fake()
    X = _corpus_with_edge_documents()
    out = held_out_scores(X, np.ones((2, X.shape[1]), np.float32), method="fold_in", random_state=1, n_iter=12,
                          n_iter_per_test=3, tolerance=0.01, flags=5)
    assert eng.lock.holds == 1
    assert eng.calls == ["upload_csr", "set_factors", "refit", "score_rows"]
    assert (eng.resident != X).nnz == 0 and (eng.scored_matrix != X).nnz == 0
    assert eng.refit_args == (None, 12, 3, 0.01, 5)
    np.testing.assert_array_equal(out["scored_documents"], np.diff(X.indptr) > 0)
    assert not out["scored_documents"][0] and out["scored_documents"][1]
    np.testing.assert_array_equal(out["tokens"], np.asarray(X.sum(1)).ravel())


def test_on_zero_modes(fake):
    from enstop_amd import held_out_scores
    X = _corpus_with_edge_documents()
    topics = np.ones((2, X.shape[1]), np.float32)
    word = int(np.argmax(np.asarray(X.sum(0)).ravel()))              # a word many documents hold
    eng = fake(zero_words=[word])
    inf = held_out_scores(X, topics, method="fold_in", random_state=1)
    skip = held_out_scores(X, topics, method="fold_in", random_state=1, on_zero="skip")
    assert inf["perplexity"] == np.inf
    assert abs(skip["perplexity"] - np.exp(2.0)) < 1e-12            # the zero-mass tokens are in neither sum
    for out in (inf, skip):                                         # the dict reports them either way
        np.testing.assert_array_equal(out["unscored"], np.asarray(X[:, [word]].sum(1)).ravel().astype(np.float64))
        assert out["unscored"].sum() > 0
    # only SCORED documents decide: zero-mass tokens in a document that is not scored leave the perplexity finite
    Y = X.tolil()
    Y[:, word] = 0
    Y[1, :] = 0
    Y[1, word] = 1                                                   # one token: never scored; held out for some seed
    Y = Y.tocsr()
    Y.eliminate_zeros()
    from enstop_amd import split_documents
    seed = next(s for s in range(50) if split_documents(Y, 0.5, s)[1][1, word] == 1)
    eng = fake(zero_words=[word])
    out = held_out_scores(Y, topics, method="completion", random_state=seed)
    assert out["unscored"][1] == 1.0 and not out["scored_documents"][1] and out["unscored"].sum() == 1.0
    assert abs(out["perplexity"] - np.exp(2.0)) < 1e-12
    with pytest.raises(ValueError):
        held_out_scores(X, topics, on_zero="ignore")
    with pytest.raises(ValueError):
        held_out_scores(X, topics, method="document_completion")


def test_document_log_likelihood_marks_zero_mass_documents(fake):
    from enstop_amd import document_log_likelihood
    X = _corpus_with_edge_documents()
    word = int(np.argmax(np.asarray(X.sum(0)).ravel()))
    eng = fake(zero_words=[word])
    got = document_log_likelihood(X, np.ones((X.shape[0], 2), np.float32) / 2, np.ones((2, X.shape[1]), np.float32))
    assert eng.lock.holds == 1 and eng.calls == ["upload_csr", "set_factors", "score_rows"]
    has = np.asarray(X[:, [word]].sum(1)).ravel() > 0
    assert has.any() and not has.all()
    assert (got[has] == -np.inf).all() and np.isfinite(got[~has]).all()
    assert got[0] == 0.0


# ------------------------------------------------------------------------------------------------
# the estimator surface
# ------------------------------------------------------------------------------------------------
def _classes():
    import enstop_amd
    return [enstop_amd.PLSA, enstop_amd.StreamedPLSA, enstop_amd.BlockParallelPLSA, enstop_amd.GPUPLSA,
            enstop_amd.DistributedPLSA, enstop_amd.EnsembleTopics]


PARAMS = {
    "PLSA": ["arithmetic", "device", "e_step_thresh", "init", "n_components", "n_iter", "n_iter_per_test", "p_budget",
             "random_state", "tolerance", "transform_random_seed"],
    "StreamedPLSA": ["arithmetic", "block_size", "device", "e_step_thresh", "init", "n_components", "n_iter",
                     "n_iter_per_test", "random_state", "tolerance", "transform_random_seed"],
    "BlockParallelPLSA": ["arithmetic", "device", "e_step_thresh", "init", "n_col_blocks", "n_components", "n_iter",
                          "n_iter_per_test", "n_row_blocks", "random_state", "tolerance", "transform_random_seed"],
    "EnsembleTopics": ["alpha", "beta_loss", "bootstrap", "device", "e_step_thresh", "init", "lift_factor", "min_cluster_size",
                       "min_samples", "model", "n_components", "n_iter", "n_iter_per_test", "n_jobs", "n_starts",
                       "nmf_backend", "parallelism", "random_state", "solver", "tolerance", "topic_combination",
                       "transform_random_seed"],
}
PARAMS["GPUPLSA"] = PARAMS["DistributedPLSA"] = PARAMS["BlockParallelPLSA"]


def test_estimators_have_the_scoring_methods_and_their_parameters_are_what_they_were():
    import inspect
    classes = _classes()
    assert len(classes) == 6
    for cls in classes:
        for name in ("score_samples", "score", "perplexity"):
            assert callable(getattr(cls, name)), (cls.__name__, name)
        sig = inspect.signature(cls.perplexity)
        assert [p for p in sig.parameters] == ["self", "X", "method", "fraction", "on_zero"]
        assert (sig.parameters["method"].default, sig.parameters["fraction"].default,
                sig.parameters["on_zero"].default) == ("completion", 0.5, "inf")
        assert sorted(cls().get_params()) == PARAMS[cls.__name__], cls.__name__
        assert "fold-in" in cls.score_samples.__doc__


def test_estimator_methods_use_components_seed_flags_and_device(fake):
    import enstop_amd
    X = _corpus_with_edge_documents()
    for cls in _classes():
        eng = fake()
        est = cls(transform_random_seed=13, device=None)
        est.components_ = np.full((2, X.shape[1]), 1.0 / X.shape[1], np.float32)
        samples = est.score_samples(X)
        assert eng.calls == ["upload_csr", "set_factors", "refit", "score_rows"] and (eng.resident != X).nnz == 0
        want_flags = est._flags() if hasattr(est, "_flags") else None
        assert eng.refit_args == (None, 50, 5, 0.001, want_flags), cls.__name__
        rng = np.random.RandomState(13)
        U0 = rng.rand(X.shape[0], 2)
        np.testing.assert_array_equal(eng.U, (U0 / U0.sum(1, keepdims=True)).astype(np.float32))
        np.testing.assert_array_equal(samples, -2.0 * np.asarray(X.sum(1)).ravel())
        assert est.score(X) == float(np.sum(samples))
        assert abs(est.perplexity(X) - np.exp(2.0)) < 1e-12
        assert abs(est.perplexity(X, method="fold_in", on_zero="skip") - np.exp(2.0)) < 1e-12
        observed, _ = enstop_amd.split_documents(X, 0.25, np.random.RandomState(13))
        est.perplexity(X, fraction=0.25)
        assert (eng.resident != observed).nnz == 0
