"""plsa_codocument_counts / Engine.codocument_counts and the device back-end of coherence, on the GPU.

The counts are integers and every combination in the kernels is an OR or an integer addition (k_metric_mark,
k_metric_count in csrc/plsa_metric_kernels.hpp), so every comparison here is np.array_equal against counts taken with
NumPy from the stored-entry pattern, `B[:, w].T @ B[:, w]` -- no tolerance anywhere.  The coherence values are compared
with the host back-end for float64 EQUALITY: both finish through utils._coherence_from_counts.

Shapes: m = 97 words; n around the wave (63, 64, 65), one document, more than one workgroup of the count pass (257, 5 000:
the count pass takes 256 documents per workgroup step, from 2 049 documents on more than one workgroup per set); lists of 2,
20, 31 and 32 words (32 uses bit 31 of the mask); 1, 3 and 33 sets that share words.  Every corpus holds a column present in
every document, an empty column, a column of stored zeros only, stored zeros and negative values among the rest, and
single-entry columns beside the dense one."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import golden_csr, load_golden

pytestmark = pytest.mark.gpu

M = 97
FULL, EMPTY, ZEROS = 0, 1, 2          # special columns; columns 90 .. 96 hold a single entry each
SPECIAL = [96, ZEROS, EMPTY, FULL]    # (a list ends with them: FULL is the last word, bit nw - 1)


@pytest.fixture(scope="module")
def eng():
    import enstop_amd as amd
    with amd.Engine() as e:
        yield e


def corpus(n, seed=0):
    rs = np.random.RandomState(seed)
    A = (rs.rand(n, M) < 0.12).astype(np.float32) * rs.randint(1, 4, (n, M))
    stored = A != 0
    A[stored & (rs.rand(n, M) < 0.1)] = -1.0                    # negative values: stored, not positive
    zero = stored & (rs.rand(n, M) < 0.1)                       # stored zeros: in the pattern, not positive
    stored[:, 90:] = False
    stored[rs.randint(0, n, 7), np.arange(90, M)] = True        # single-entry columns
    A[:, 90:] = 1.0
    stored[:, FULL], A[:, FULL] = True, 2.0
    stored[:, EMPTY] = False
    stored[:, ZEROS] = rs.rand(n) < 0.5
    stored[0, ZEROS] = True
    zero[:, ZEROS] = True
    zero[:, [FULL, EMPTY]] = False
    zero[:, 90:] = False
    A[zero] = 0.0
    rows, cols = np.nonzero(stored)
    X = sp.csr_matrix((A[rows, cols].astype(np.float32), (rows, cols)), shape=(n, M))     # keeps the stored zeros
    assert X.nnz == stored.sum() and (X.data == 0).sum() >= 1 and X.has_canonical_format
    return X


def word_lists(sets, nw, seed=0):
    """[sets, nw] distinct ids per row; the rows share the special columns (rotated) and overlap at random elsewhere"""
    rs = np.random.RandomState(1000 + seed)
    out = np.empty((sets, nw), np.int32)
    for s in range(sets):
        special = (SPECIAL[-(s % 4):] + SPECIAL[:-(s % 4)] if s % 4 else list(SPECIAL))[-min(nw, 4):]
        rest = [w for w in rs.permutation(M) if w not in special][:nw - len(special)]
        out[s] = rest + special
        assert len(set(out[s])) == nw
    return out


def expected(X, words):
    X = sp.csr_matrix(X)
    rows = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    B = np.zeros(X.shape, np.int64)
    B[rows, X.indices] = 1
    P = np.zeros(X.shape, np.int64)
    P[rows, X.indices] = X.data > 0
    co = np.stack([B[:, w].T @ B[:, w] for w in words])
    positive = np.stack([P[:, w].sum(axis=0) for w in words])
    return co, positive


def check(eng, X, words, max_sets_per_pass=0):
    co, positive = eng.codocument_counts(words, max_sets_per_pass)
    want_co, want_pos = expected(X, words)
    assert co.dtype == np.int64 and positive.dtype == np.int64
    assert np.array_equal(co, want_co)
    assert np.array_equal(positive, want_pos)
    return co, positive


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
@pytest.mark.parametrize("nw", [2, 20, 31, 32])
def test_counts_equal_numpy(eng, n, nw):
    X = corpus(n, seed=n)
    eng.upload_csr(X)
    sets = {2: 33, 20: 3, 31: 1, 32: 3}[nw]
    words = word_lists(sets, nw, seed=nw)
    co, positive = check(eng, X, words)
    if nw == 32:                                    # bit 31: a signed shift would lose or smear it
        assert words[0, 31] == FULL
        assert co[0, 31, :].any() and co[0, :, 31].any() and co[0, 31, 31] == n
    if nw >= 4:
        s0 = list(words[0])
        assert positive[0, s0.index(ZEROS)] == 0 and co[0, s0.index(ZEROS), s0.index(ZEROS)] > 0     # stored zeros only
        assert not co[0, s0.index(EMPTY)].any() and not co[0, :, s0.index(EMPTY)].any()             # the empty column
        assert co[0, s0.index(FULL), s0.index(96)] == 1                                             # dense beside single-entry


@pytest.mark.parametrize("sets", [1, 3, 33])
def test_sets_that_share_words(eng, sets):
    X = corpus(257, seed=5)
    eng.upload_csr(X)
    words = word_lists(sets, 20, seed=sets)
    if sets > 1:
        assert set(words[0]) & set(words[1])
    check(eng, X, words)


def test_corpus_without_stored_entries(eng):
    X = sp.csr_matrix((65, M), dtype=np.float32)
    eng.upload_csr(X)
    co, positive = check(eng, X, word_lists(3, 20))
    assert not co.any() and not positive.any()


def test_chunked_passes_successive_calls_and_released_scratch(eng):
    X = corpus(257, seed=9)
    eng.upload_csr(X)
    words = word_lists(5, 20, seed=3)
    whole = check(eng, X, words)
    chunked = check(eng, X, words, max_sets_per_pass=2)            # 2 + 2 + 1 sets
    again = check(eng, X, words)                                   # the masks of the call before are gone
    eng.release_scratch()
    after = check(eng, X, words)
    for other in (chunked, again, after):
        assert np.array_equal(other[0], whole[0]) and np.array_equal(other[1], whole[1])
    first_only = check(eng, X, words[:1])                          # fewer sets after more: stale rows are not read
    assert np.array_equal(first_only[0][0], whole[0][0])


def test_counts_follow_the_active_matrix(eng):
    X = corpus(257, seed=4)
    eng.upload_csr(X)
    words = word_lists(3, 20, seed=1)
    check(eng, X, words)
    idx = np.random.RandomState(2).randint(0, 257, 300)
    assert len(np.unique(idx)) < len(idx)
    eng.bootstrap(idx)
    check(eng, X[idx], words)
    eng.bootstrap(None)
    check(eng, X, words)


def test_bad_arguments_are_status_codes_and_the_context_stays_usable():
    import enstop_amd as amd
    from enstop_amd.engine import DeviceError
    X = corpus(65, seed=1)
    good = word_lists(2, 20)
    with amd.Engine() as e:
        with pytest.raises(DeviceError, match="no corpus"):
            e.codocument_counts(good)
        e.upload_csr(X)
        for bad_id in (M, -1):
            bad = good.copy()
            bad[1, 7] = bad_id
            with pytest.raises(DeviceError, match="word id"):
                e.codocument_counts(bad)
        for nw in (1, 33):
            with pytest.raises(DeviceError, match="nw="):
                e.codocument_counts(np.arange(nw, dtype=np.int32)[None, :])
        with pytest.raises(DeviceError, match="sets="):
            e.codocument_counts(np.zeros((0, 5), np.int32))
        with pytest.raises(DeviceError, match="max_sets_per_pass"):
            e.codocument_counts(good, max_sets_per_pass=-1)
        check(e, X, good)


def _no_ties(T):
    assert all(len(np.unique(row)) == T.shape[1] for row in T)       # NumPy and Numba may order ties differently
    return T


def test_golden_metrics_through_the_device_backend():
    from enstop_amd import utils
    g = load_golden("metrics")
    X, T = golden_csr(g), g["topics"]
    for z in range(T.shape[0]):
        utils.last_metric_path = None
        dev = utils.coherence(T, z, X, n_words=10, backend="device")
        assert utils.last_metric_path == "device"
        np.testing.assert_allclose(dev, g["coherence"][z], rtol=1e-10)
        assert dev == utils.coherence(T, z, X, n_words=10, backend="host")
        assert utils.last_metric_path == "host"
    dev = utils.mean_coherence(T, X, n_words=10, backend="device")
    assert utils.last_metric_path == "device"
    np.testing.assert_allclose(dev, g["mean_coherence"], rtol=1e-10)
    assert dev == utils.mean_coherence(T, X, n_words=10, backend="host")


def test_random_topics_device_equals_host(monkeypatch):
    from enstop_amd import utils
    X = corpus(5000, seed=8).astype(np.float64)
    T = _no_ties(np.random.default_rng(0).random((7, M)))
    for n_words in (2, 20, 32):
        assert utils.mean_coherence(T, X, n_words=n_words, backend="device") == utils.mean_coherence(T, X, n_words=n_words, backend="host")
        assert utils.coherence(T, 3, X.tocsc(), n_words=n_words, backend="device") == utils.coherence(T, 3, X, n_words=n_words, backend="host")
    monkeypatch.setenv("ENSTOP_AMD_METRICS", "device")
    utils.mean_coherence(T, X)
    assert utils.last_metric_path == "device"
    monkeypatch.setenv("ENSTOP_AMD_METRICS", "host")
    utils.mean_coherence(T, X)
    assert utils.last_metric_path == "host"
    monkeypatch.delenv("ENSTOP_AMD_METRICS")
    utils.mean_coherence(T, X)                        # auto, a device is present
    assert utils.last_metric_path == "device"


def test_estimator_coherence_takes_the_device_and_equals_the_host(monkeypatch):
    from enstop_amd import PLSA, utils
    monkeypatch.delenv("ENSTOP_AMD_METRICS", raising=False)
    X = abs(corpus(257, seed=6))
    X.eliminate_zeros()
    model = PLSA(n_components=3, n_iter=10, random_state=0).fit(X)
    utils.last_metric_path = None
    got = model.coherence()
    assert utils.last_metric_path == "device"
    assert got == utils.mean_coherence(model.components_, model.training_data_, backend="host")
    assert model.coherence(1, n_words=5) == utils.coherence(model.components_, 1, model.training_data_, n_words=5, backend="host")


def test_tiny_positive_float64_entries_stay_positive():
    from enstop_amd import utils
    X = corpus(65, seed=3).astype(np.float64).tocsr()
    X.data[X.indices == 7] = 1e-50                    # flushes to zero as float32
    assert (X.indices == 7).sum() > 0 and np.float32(1e-50) == 0
    words = word_lists(2, 20, seed=2)
    words[0, 0] = 7 if 7 not in words[0] else words[0, 0]
    assert 7 in words[0]
    co, positive = utils._device_counts(words, X)
    want_co, _ = expected(X, words)
    want_pos = np.stack([np.asarray((X > 0).sum(axis=0)).ravel()[w] for w in words])
    assert np.array_equal(positive, want_pos) and np.array_equal(co, want_co)
    assert positive[0, list(words[0]).index(7)] == (X.indices == 7).sum()


def test_calls_the_device_cannot_carry(monkeypatch):
    from enstop_amd import utils
    monkeypatch.delenv("ENSTOP_AMD_METRICS", raising=False)
    X = corpus(65, seed=2)
    T = _no_ties(np.random.default_rng(1).random((3, M)))

    def cases():
        dup = sp.csr_matrix((np.ones(4), np.array([1, 1, 0, 2]), np.array([0, 2, 4])), shape=(2, M))
        assert not dup.has_canonical_format
        return [(X, 40), (X.toarray(), 5), (dup, 3)]

    for data, n_words in cases():
        with pytest.raises(ValueError, match="device"):
            utils.mean_coherence(T, data, n_words=n_words, backend="device")
    for data, n_words in cases():
        utils.last_metric_path = None
        utils.mean_coherence(T, data, n_words=n_words)
        assert utils.last_metric_path == "host"
