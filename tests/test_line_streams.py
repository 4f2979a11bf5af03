"""The line layout of the packed entry streams (PLSA_PACKED=1): every document, row item and column item
starts on a block of 4 * LPN words, a lane loads one 16-byte vector per block and batch c consumes component c.  A lane handles
the entry it handled with one word per load, so a fused fit on the line streams equals the fit on the (index, value) arrays
(PLSA_PACKED=0) BIT FOR BIT: both factor matrices and the likelihood trace.  The corpora are small and built so that row and
column lengths land on the block edges of each lane shape, with escaped counts on the block's corners.
Needs a real MI355X: run with  pytest -m gpu."""
import numpy as np
import pytest
import scipy.sparse as sp

from test_pass_matrix import lane_shape

pytestmark = pytest.mark.gpu

FUSED = 1
ESCAPES = (0.5, 256.0, 1000.0, 0.0)                  # a fraction, above the code's 255 twice, a stored zero
N_DOCS = 70
N_ROW_CASES = 9
N_COL_CASES = 6


@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


def row_lengths(lpn):
    return [0, 1, lpn - 1, lpn, lpn + 1, 4 * lpn - 1, 4 * lpn, 4 * lpn + 1, 8 * lpn + 3]


def col_lengths(seg):
    return [0, 1, seg - 1, seg, seg + 1, 2 * seg + 5]


def edge_corpus(k, seg, seed=0, escapes=True):
    """70 documents x (about) 90 words.  Documents 0..8 have row_lengths(document pass LPN) entries, in the words from 6 on;
    words 0..5 have col_lengths(seg) entries, in the documents from 9 on; the other documents hold about 20 more words each.
    Escaped counts: in every special document its first entry (first word of a block), the first entry of component 3, the
    first entry of the last partial block and its last entry; in every special word its first and its last entry (an item's
    last entry: the word of `seg` entries, and entry seg - 1 of the longer ones)."""
    row_lpn = lane_shape(k)[2][0]
    rows, cols = row_lengths(row_lpn), col_lengths(seg)
    assert len(rows) == N_ROW_CASES and len(cols) == N_COL_CASES and max(cols) <= N_DOCS - N_ROW_CASES
    m = max(90, N_COL_CASES + max(rows) + 8)
    rs = np.random.RandomState(1000 * k + seed)
    A = np.zeros((N_DOCS, m), np.float32)
    for d, length in enumerate(rows):
        A[d, N_COL_CASES + rs.choice(m - N_COL_CASES, length, replace=False)] = rs.randint(1, 8, size=length)
    for w, length in enumerate(cols):
        A[N_ROW_CASES + rs.choice(N_DOCS - N_ROW_CASES, length, replace=False), w] = rs.randint(1, 8, size=length)
    for d in range(N_ROW_CASES, N_DOCS):
        A[d, N_COL_CASES + rs.choice(m - N_COL_CASES, 20, replace=False)] = rs.randint(1, 256, size=20)
    X = sp.csr_matrix(A)
    assert list(np.diff(X.indptr)[:N_ROW_CASES]) == rows and list(X.getnnz(axis=0)[:N_COL_CASES]) == cols
    if escapes:
        turn = 0
        for d, length in enumerate(rows):
            block = 4 * row_lpn
            for rel in {0, 3 * row_lpn, (length - 1) // block * block, length - 1}:
                if 0 <= rel < length:
                    X.data[X.indptr[d] + rel] = ESCAPES[turn % 4]
                    turn += 1
        csc_rows = {w: np.flatnonzero(A[:, w]) for w in range(N_COL_CASES)}        # column entries in document order
        for w, length in enumerate(cols):
            for rel in {0, seg - 1, length - 1}:
                if 0 <= rel < length:
                    d = csc_rows[w][rel]
                    j = X.indptr[d] + np.searchsorted(X.indices[X.indptr[d]:X.indptr[d + 1]], w)
                    assert X.indices[j] == w
                    X.data[j] = ESCAPES[turn % 4]
                    turn += 1
        assert turn >= 20 and turn * 16 <= X.nnz and (X.data == 0).sum() >= 4
    return X.astype(np.float32)


def factors(n, m, k, seed=11):
    rs = np.random.RandomState(seed)
    U = rs.rand(n, k); U /= U.sum(1, keepdims=True)
    V = rs.rand(k, m); V /= V.sum(1, keepdims=True)
    return U.astype(np.float32), V.astype(np.float32)


def fit(eng, k, sw=None, rows=None):
    n, m, _ = eng.shape
    U0, V0 = factors(n if rows is None else int(rows.max()) + 1, m, k)
    eng.set_factors(U0 if rows is None else U0[rows], V0)
    iters, ll = eng.fit(sw, n_iter=2, n_iter_per_test=1, tolerance=0.0, e_step_thresh=1e-32, flags=FUSED, trace=True)
    U, V = eng.get_factors()
    return dict(U=U, V=V, iters=int(iters), ll=np.asarray(ll, np.float32))


def same(a, b, what=""):
    assert sorted(a) == sorted(b)
    for key in sorted(a):
        if isinstance(a[key], np.ndarray):
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, (what, key)
            width = {4: np.uint32, 8: np.uint64}[a[key].dtype.itemsize]
            np.testing.assert_array_equal(a[key].view(width), b[key].view(width), err_msg="%s %s" % (what, key))
        else:
            assert a[key] == b[key], (what, key, a[key], b[key])


def both(amd, monkeypatch, body, env=()):
    """body(engine factory) with PLSA_PACKED=0 and with PLSA_PACKED=1 -> the two results"""
    out = []
    for key, value in env:
        monkeypatch.setenv(key, value)
    for packed in (0, 1):
        monkeypatch.setenv("PLSA_PACKED", str(packed))
        out.append(body(amd.Engine))
    return out


def ab(amd, monkeypatch, X, k, expect="packed", env=(), **kw):
    def body(engine):
        with engine() as eng:
            eng.upload_csr(X)
            out = fit(eng, k, **kw)
            out["info"] = repr(eng.packed_info())
            out["seg"] = eng.balance_info()["item_entries"]
        return out
    old, new = both(amd, monkeypatch, body, env)
    assert old.pop("info") == repr(dict(csr="arrays", csc="arrays"))
    assert new.pop("info") == repr(dict(csr=expect, csc=expect))
    same(old, new)
    return new


SEG = 16        # column items of the small corpora (plsa_launch_plan.hpp: col_item_len's floor), checked in every case


@pytest.mark.parametrize("k", [3, 6, 20, 32, 64, 128, 130])
def test_block_edges_in_every_lane_shape(amd, monkeypatch, k):
    """row lengths 0, 1, LPN - 1, LPN, LPN + 1, 4 LPN - 1, 4 LPN, 4 LPN + 1, 8 LPN + 3 in the document pass' LPN, column lengths
    0, 1, seg - 1, seg, seg + 1, 2 seg + 5, escapes on the corners: lane counts 1, 2, 8, 8, 8 x 2 / 16, 16 x 2 and 32 x 2"""
    assert [lane_shape(q)[1][0] for q in (3, 6, 20, 32, 64, 128, 130)] == [1, 2, 8, 8, 16, 16, 32]
    assert lane_shape(64)[2] == (8, 2)
    out = ab(amd, monkeypatch, edge_corpus(k, SEG), k)
    assert out["seg"] == SEG


def test_more_than_a_sixteenth_escaped_drops_the_streams(amd, monkeypatch):
    X = edge_corpus(20, SEG, seed=1)
    X.data[::8] = 0.25                                   # one entry in eight escapes: both streams are ineligible
    ab(amd, monkeypatch, X, 20, expect="arrays")


@pytest.mark.parametrize("variant", ["sample_weights", "force_wide"])
def test_sample_weights_and_wide_gathers(amd, monkeypatch, variant):
    X = edge_corpus(64, SEG, seed=2)
    if variant == "sample_weights":
        ab(amd, monkeypatch, X, 64, sw=(np.random.RandomState(3).rand(N_DOCS) + 0.5).astype(np.float32))
    else:
        ab(amd, monkeypatch, X, 64, env=[("PLSA_FORCE_WIDE", "1")])


def long_documents(seed=4):
    """three documents of 5000 entries: the document pass runs over row items (every item its own slot of the stream)"""
    rs = np.random.RandomState(seed)
    A = np.zeros((3, 6000), np.float32)
    for d in range(3):
        A[d, rs.choice(6000, 5000, replace=False)] = rs.randint(1, 200, size=5000)
    X = sp.csr_matrix(A)
    X.data[[0, 15, 16, 4999, 5000, 9999, 14999]] = [0.5, 256.0, 1000.0, 0.0, 0.5, 256.0, 1000.0]     # items' first and last entries
    return X


@pytest.mark.parametrize("k", [20, 64])
def test_row_items_have_their_own_slots(amd, monkeypatch, k):
    X = long_documents()

    def body(engine):
        with engine() as eng:
            eng.upload_csr(X)
            eng.timing(True)
            out = fit(eng, k)
            assert "k_row_reduce" in set(eng.timing_report())          # the pass did run over row items
            out["info"] = repr(eng.packed_info())
        return out
    old, new = both(amd, monkeypatch, body)
    assert new.pop("info") == repr(dict(csr="packed", csc="packed")) and old.pop("info") == repr(dict(csr="arrays", csc="arrays"))
    same(old, new)


def test_forced_heavy_columns(amd, monkeypatch):
    """column items of 8 entries in 16-lane groups (a slot is a block of 64 words), columns of 3 items or more are heavy"""
    out = ab(amd, monkeypatch, edge_corpus(64, 8, seed=5), 64, env=[("PLSA_COL_SEG", "8"), ("PLSA_HEAVY_ITEMS", "2")])
    assert out["seg"] == 8


def test_rebuilds_after_bootstrap_release_and_a_new_lane_shape(amd, monkeypatch):
    """bootstrap -> fit -> plsa_release_scratch -> refit (the streams come back, the column stream from the CSC arrays); then
    k = 64 followed by k = 32 on the same context: 8-lane blocks in the document stream stay, the column stream goes from
    16-lane to 8-lane blocks"""
    X = edge_corpus(64, SEG, seed=6)
    idx = np.random.RandomState(7).randint(0, N_DOCS, size=N_DOCS)

    def body(engine):
        out = {}
        with engine() as eng:
            eng.upload_csr(X)
            eng.bootstrap(idx)
            first = fit(eng, 64, rows=idx)
            eng.release_scratch()
            second = fit(eng, 64, rows=idx)
            same(first, second, "refit after release_scratch")
            for key, value in second.items():
                out["boot_" + key] = value
            eng.bootstrap(None)
            for k in (64, 32):
                for key, value in fit(eng, k).items():
                    out["k%d_%s" % (k, key)] = value
                out["k%d_info" % k] = repr(eng.packed_info())
        with engine() as eng:                            # k = 32 on a context of its own
            eng.upload_csr(X)
            same({key[4:]: value for key, value in out.items() if key.startswith("k32_") and key != "k32_info"}, fit(eng, 32),
                 "k = 32 after k = 64")
        return out
    old, new = both(amd, monkeypatch, body)
    for k in (64, 32):
        assert new.pop("k%d_info" % k) == repr(dict(csr="packed", csc="packed"))
        assert old.pop("k%d_info" % k) == repr(dict(csr="arrays", csc="arrays"))
    same(old, new)


def test_batched_members_nmf_and_scoring_read_the_same_streams(amd, monkeypatch):
    """one step each of the batched members (k_row_pass_members / k_col_pass_members), an NMF half-iteration pair (nmf_sweep)
    and plsa_score_rows after a fit"""
    k = 64
    X = edge_corpus(k, SEG, seed=8)
    m = X.shape[1]
    rs = np.random.RandomState(9)
    idxs = [rs.randint(0, N_DOCS, size=N_DOCS) for _ in range(2)]
    U0, V0 = factors(N_DOCS, m, k)
    W0, H0 = (rs.rand(N_DOCS, k) + 0.1).astype(np.float32), (rs.rand(k, m) + 0.1).astype(np.float32)

    def body(engine):
        out = {}
        with engine() as eng:
            eng.upload_csr(X)
            batch = eng.member_batch(2)
            for r, idx in enumerate(idxs):
                batch.prepare(r, k, idx=idx, U=U0[idx], V=V0)
            iters, traces = batch.fit(2, n_iter=1, n_iter_per_test=1, tolerance=0.0, flags=FUSED, trace=True)
            assert batch.last_batched == 2
            for r in range(2):
                out["member%d_U" % r], out["member%d_V" % r] = batch.member(r).get_factors()
                out["member%d_ll" % r] = np.asarray(traces[r], np.float32)
            out["member_iters"] = [int(i) for i in iters]
            eng.nmf_set_factors(W0, H0)
            eng.nmf_update_w()
            eng.nmf_update_h()
            out["W"], out["H"] = eng.nmf_get_factors()
            fit(eng, k)
            out["score_ll"], out["score_tokens"], out["score_unscored"] = eng.score_rows()
        return out
    old, new = both(amd, monkeypatch, body)
    same(old, new)
