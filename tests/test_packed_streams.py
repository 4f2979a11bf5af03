"""The packed entry streams of the fused passes (PLSA_PACKED): one 32-bit word per non-zero, id | count << 24,
with an escape to the float array for counts that are not integers in 1..255.  The kernels see the same id and the same float
count either way, so a fused fit with the packed streams must equal the fit with the (index, value) arrays BIT FOR BIT.
Needs a real MI355X: run with  pytest -m gpu."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

FUSED = 1


@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


def _counts(n, m, density, seed, empty_rows=0):
    rs = np.random.RandomState(seed)
    X = sp.random(n, m, density=density, format="csr", random_state=rs, dtype=np.float64)
    X.data = np.ceil(X.data * 7)
    if empty_rows:
        X = X.tolil()
        for r in rs.choice(n, empty_rows, replace=False):
            X[r, :] = 0
        X = X.tocsr()
    return X.astype(np.float32)


def _factors(n, m, k, seed=11):
    rs = np.random.RandomState(seed)
    U = rs.rand(n, k); U /= U.sum(1, keepdims=True)
    V = rs.rand(k, m); V /= V.sum(1, keepdims=True)
    return U.astype(np.float32), V.astype(np.float32)


def _fit(eng, k, sw=None, n_iter=9, thresh=1e-32):
    n, m, _ = eng.shape
    U0, V0 = _factors(n, m, k)
    eng.set_factors(U0, V0)
    iters, ll = eng.fit(sw, n_iter=n_iter, n_iter_per_test=3, tolerance=0.0, e_step_thresh=thresh, flags=FUSED, trace=True)
    U, V = eng.get_factors()
    return dict(U=U, V=V, iters=iters, ll=ll)


def _run(amd, monkeypatch, packed, X, k, idx=None, env=(), **kw):
    monkeypatch.setenv("PLSA_PACKED", str(packed))
    for key, value in env:
        monkeypatch.setenv(key, value)
    with amd.Engine() as eng:
        eng.upload_csr(X)
        if idx is not None:
            eng.bootstrap(idx)
        out = _fit(eng, k, **kw)
        out["info"] = eng.packed_info()
    return out


def _same(a, b):
    np.testing.assert_array_equal(a["U"].view(np.uint32), b["U"].view(np.uint32))
    np.testing.assert_array_equal(a["V"].view(np.uint32), b["V"].view(np.uint32))
    assert a["iters"] == b["iters"]
    np.testing.assert_array_equal(a["ll"].view(np.uint32), b["ll"].view(np.uint32))


def _ab(amd, monkeypatch, X, k, expect, **kw):
    old = _run(amd, monkeypatch, 0, X, k, **kw)
    new = _run(amd, monkeypatch, 1, X, k, **kw)
    assert old["info"] == dict(csr="arrays", csc="arrays")
    assert new["info"] == dict(csr=expect, csc=expect)
    _same(old, new)
    return new


@pytest.mark.parametrize("k", [20, 32, 64, 128])
def test_midsize_corpus_bit_identical(amd, monkeypatch, k):
    """k = 20 / 32 / 64 / 128 cover the lane shapes of both passes (k = 64: the 8 x 2 document pass)"""
    _ab(amd, monkeypatch, _counts(6000, 3000, 0.01, seed=1), k, "packed")


@pytest.mark.parametrize("variant", ["wide", "tiny_threshold", "row_items"])
def test_kernel_variants_bit_identical(amd, monkeypatch, variant):
    """64-bit gather addresses (PLSA_FORCE_WIDE), the denormal-norm rescue (threshold 0) and the row items of the document pass"""
    X = _counts(3000, 2000, 0.02, seed=2)
    kw = {"wide": dict(env=[("PLSA_FORCE_WIDE", "1")]), "tiny_threshold": dict(thresh=0.0),
          "row_items": dict(env=[("PLSA_ROW_ITEMS", "1"), ("PLSA_ROW_SEG", "16")])}[variant]
    _ab(amd, monkeypatch, X, 64, "packed", **kw)


def test_counts_above_255_take_the_escape(amd, monkeypatch):
    """a few counts outside 1..255 or not integers (256, 300, 4 000, 2.5, 0.75): escaped entries, the streams stay packed"""
    X = _counts(4000, 2500, 0.01, seed=3)
    rs = np.random.RandomState(4)
    pick = rs.choice(X.nnz, 40, replace=False)
    X.data[pick] = np.resize(np.array([256, 300, 4000, 2.5, 0.75, 255, 1], np.float32), 40)
    _ab(amd, monkeypatch, X, 32, "packed")


def test_all_fractional_values_fall_back_to_the_arrays(amd, monkeypatch):
    """tf-idf-like weights: every entry would escape, both streams are ineligible and the two-array kernels run"""
    X = _counts(3000, 2000, 0.02, seed=5)
    X.data = (np.random.RandomState(6).rand(X.nnz) * 3 + 0.01).astype(np.float32)
    _ab(amd, monkeypatch, X, 20, "arrays")


def test_stored_zeros_and_empty_rows(amd, monkeypatch):
    X = _counts(3000, 1500, 0.02, seed=7, empty_rows=200)
    rs = np.random.RandomState(8)
    X.data[rs.choice(X.nnz, X.nnz // 40, replace=False)] = 0.0          # stored zeros: escaped entries with x = 0
    assert (X.data == 0).sum() > 0 and (np.diff(X.indptr) == 0).sum() >= 200
    _ab(amd, monkeypatch, X, 20, "packed")


def test_sample_weights(amd, monkeypatch):
    X = _counts(3000, 1500, 0.02, seed=9)
    sw = (np.random.RandomState(10).rand(3000) + 0.5).astype(np.float32)
    _ab(amd, monkeypatch, X, 64, "packed", sw=sw)


def test_bootstrap_release_scratch_refit(amd, monkeypatch):
    """a bootstrap resample, plsa_release_scratch (frees the packed streams), a refit on the same upload: rebuilt streams, same bits"""
    X = _counts(4000, 2000, 0.015, seed=12)
    idx = np.random.RandomState(13).randint(0, 4000, size=4000)
    out = {}
    for packed in (0, 1):
        monkeypatch.setenv("PLSA_PACKED", str(packed))
        with amd.Engine() as eng:
            eng.upload_csr(X)
            eng.bootstrap(idx)
            first = _fit(eng, 32)
            eng.release_scratch()
            assert eng.packed_info() == (dict(csr=None, csc=None) if packed else dict(csr="arrays", csc="arrays"))
            second = _fit(eng, 32)
            _same(first, second)
            info = eng.packed_info()
            eng.bootstrap(None)                                  # a new active matrix invalidates the streams
            assert eng.packed_info() == (dict(csr=None, csc=None) if packed else info)
            base = _fit(eng, 32)
        out[packed] = (second, base, info)
    assert out[1][2] == dict(csr="packed", csc="packed")
    _same(out[0][0], out[1][0])
    _same(out[0][1], out[1][1])


def test_small_corpus_item_mode_config1_shape(amd, monkeypatch):
    """the 20NG-shaped corpus of BASELINE config 1 (18 846 x 173 762, 2.95 M non-zeros, k = 20): row items, short column
    items, both passes side by side on two streams"""
    out = {}
    for packed in (0, 1):
        monkeypatch.setenv("PLSA_PACKED", str(packed))
        with amd.Engine() as eng:
            eng.generate_synthetic(18_846, 173_762, 2_950_000, zipf_s=1.07, seed=3)
            out[packed] = _fit(eng, 20, n_iter=6)
            out[packed]["info"] = eng.packed_info()
    assert out[1]["info"] == dict(csr="packed", csc="packed")
    _same(out[0], out[1])
