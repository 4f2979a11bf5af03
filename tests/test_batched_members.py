"""Batched ensemble members (parallelism="batched", engine.MemberBatch) against the classic one-member-at-a-time path,
BIT FOR BIT: topics, iteration counts and log-likelihood traces.  Needs a real MI355X (-m gpu).

The contract (include/plsa_hip_members.h): member r of a batch is what plsa_bootstrap + the
initialisation + plsa_fit give on a context of its own, whatever the batch size and whoever else is in the batch; the
likelihood test is per member; calls a batch cannot carry take the classic path silently.  Every comparison here is
`assert_array_equal` on the float32 bit patterns -- there is no tolerance to choose.

Which instantiation ran is read back, not assumed: lane shapes and gather widths from the member's pass_info(), the
index streams from its packed_info(), row items / heavy columns / norm stages / launch group from MemberBatch.info().
"""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

KNOBS = ("PLSA_FORCE_WIDE", "PLSA_PACKED", "PLSA_ROW_ITEMS", "PLSA_ROW_SEG", "PLSA_HEAVY_ITEMS", "PLSA_COL_SEG",
         "ENSTOP_AMD_ENSEMBLE", "ENSTOP_AMD_BATCH_MEMBERS", "ENSTOP_AMD_HOST_INIT")


@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


@pytest.fixture()
def env(monkeypatch):
    """PLSA_* knobs are read when a context is created: patch the environment, start from fresh engines, and leave fresh
    engines (and the caller's environment) behind."""
    from enstop_amd.engine import reset_engines

    def apply(**settings):
        for key in KNOBS:
            monkeypatch.delenv(key, raising=False)
        for key, value in settings.items():
            monkeypatch.setenv(key, str(value))
        reset_engines()
    apply()
    yield apply
    monkeypatch.undo()
    reset_engines()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _equal(a, b, what):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


# ------------------------------------------------------------------------------------------------
# members through the batch interface, and the same members one at a time on a context of their own
# ------------------------------------------------------------------------------------------------
def seeded_member(X, k, seed):
    """what enstop_._member_on_engine does with RandomState(seed): the bootstrap draw, then the same stream into plsa_init"""
    return dict(seed=seed)


def _classic(eng, X, k, spec, fit_kw):
    """one member the classic way -> (iterations, float32 trace, P(z|d), P(w|z), pass_info, packed_info)"""
    from enstop_amd.plsa import _fit_on_engine
    eng.upload_csr(X)
    if "seed" in spec:
        rng = np.random.RandomState(spec["seed"])
        eng.bootstrap(rng.randint(0, X.shape[0], size=X.shape[0]))
        iters, ll = _fit_on_engine(eng, k, None, "random", fit_kw["n_iter"], fit_kw["n_iter_per_test"], fit_kw["tolerance"],
                                   fit_kw["e_step_thresh"], rng, fit_kw.get("flags"), trace=True)
    else:
        eng.bootstrap(spec["idx"])
        eng.set_factors(spec["U"], spec["V"])
        iters, ll = eng.fit(None, trace=True, **fit_kw)
    U, V = eng.get_factors()
    return iters, ll, U, V, eng.pass_info(), eng.packed_info()


def _batched(eng, X, k, specs, fit_kw, slots=None):
    from enstop_amd.enstop_ import _prepare_member
    eng.upload_csr(X)
    batch = eng.member_batch(slots or len(specs))
    for j, spec in enumerate(specs):
        if "seed" in spec:
            _prepare_member(batch, j, eng, k, random_state=np.random.RandomState(spec["seed"]))
        else:
            batch.prepare(j, k, idx=spec["idx"], U=spec["U"], V=spec["V"])
    iters, traces = batch.fit(len(specs), trace=True, **fit_kw)
    out = []
    for j in range(len(specs)):
        view = batch.member(j)
        U, V = view.get_factors()
        out.append((int(iters[j]), traces[j], U, V, view.pass_info(), view.packed_info(), batch.info(j), batch.last_ll(j)))
    return out, batch


def _alone_ll(eng, X, k, spec, fit_kw):
    """the float64 likelihood behind the member's last test when it is the only member: a batch of one runs the classic
    loop (plsa_fit) on the member's context, its own grid in every kernel"""
    got, batch = _batched(eng, X, k, [spec], fit_kw)
    assert batch.last_batched == 0 and got[0][6]["group"] == -1
    return got[0][7]


def compare(amd, X, k, specs, fit_kw, what, expect_batched=True):
    """batched == classic for every member, bit for bit; returns (classic results, batched results)"""
    from enstop_amd.engine import get_engine
    eng = get_engine()
    got, batch = _batched(eng, X, k, specs, fit_kw)
    assert batch.last_batched == (len(specs) if expect_batched else 0), (what, batch.last_batched)
    want = [_classic(eng, X, k, spec, fit_kw) for spec in specs]
    for j, (w, g) in enumerate(zip(want, got)):
        tag = "%s member %d" % (what, j)
        assert g[0] == w[0], (tag, "iterations", g[0], w[0])
        assert g[1].dtype == np.float32 and g[1].shape == w[1].shape, (tag, "trace length", g[1].shape, w[1].shape)
        _equal(g[1], w[1], tag + " trace")
        _equal(g[3], w[3], tag + " P(w|z)")
        _equal(g[2], w[2], tag + " P(z|d)")
        assert g[4] == w[4], (tag, "pass_info", g[4], w[4])
        assert g[5] == w[5], (tag, "packed_info", g[5], w[5])
        # the float32 traces cannot see HOW the fused log-likelihood was added up; the float64 value can: one partial per
        # workgroup of the member's own document-pass grid, added in that grid's order
        alone = _alone_ll(eng, X, k, specs[j], fit_kw)
        assert np.float32(alone) == g[1][-1], (tag, alone, g[1][-1])
        assert np.float64(g[7]).view(np.uint64) == np.float64(alone).view(np.uint64), (tag, "float64 likelihood", g[7], alone)
    return want, got


def counts_corpus(n=300, m=500, seed=0, density=0.03, fractional=0.0, empty_docs=(), unused_words=0):
    rs = np.random.RandomState(seed)
    mask = rs.rand(n, m) < density
    mask[:, 5] = True                                   # a word in every document (long column)
    mask[3, rs.choice(m, min(m, 200), replace=False)] = True     # a long document
    if unused_words:
        mask[:, m - unused_words:] = False
    mask[list(empty_docs), :] = False
    r, c = np.nonzero(mask)
    x = rs.randint(1, 8, size=r.shape[0]).astype(np.float32)
    if fractional:
        pick = rs.rand(r.shape[0]) < fractional
        x[pick] += 0.37                                 # not a small integer: escapes the packed stream
    return sp.csr_matrix((x, (r, c)), shape=(n, m))


FIT = dict(n_iter=7, n_iter_per_test=2, tolerance=0.0, e_step_thresh=1e-16)


# ------------------------------------------------------------------------------------------------
# 1. the BASELINE shape through the public interface
# ------------------------------------------------------------------------------------------------
def test_stack_equals_the_classic_stack_at_the_20ng_shape(amd, env):
    from enstop_amd import enstop_
    with amd.Engine() as e:
        e.generate_synthetic(18846, 173762, 2950000, seed=0)
        X = e.download_active_csr()
    k, kw = 20, dict(n_runs=32, random_state=7, n_iter=20, n_iter_per_test=10, tolerance=0, e_step_thresh=1e-16)
    want = amd.ensemble_of_topics(X, k, parallelism="dask", n_jobs=1, **kw)
    assert enstop_.last_ensemble_timing["path"] == "contexts"
    for cap, batches in ((None, [32]), (5, [5] * 6 + [2]), (1, [1] * 32)):
        env(**({} if cap is None else {"ENSTOP_AMD_BATCH_MEMBERS": cap}))
        got = amd.ensemble_of_topics(X, k, parallelism="batched", **kw)
        t = enstop_.last_ensemble_timing
        assert t["path"] == "batched" and t["batch"] == (cap or 32), t
        assert [sum(g) for g in t["groups"]] == batches, t["groups"]
        if cap != 1:
            assert all(g == [sum(g)] for g in t["groups"]), t["groups"]      # one launch group per batch
        _equal(got, want, "stack, batch cap %s" % cap)
    for run in (0, 13, 31):
        V = amd.plsa_topics(X, k, random_state=np.random.RandomState(7 + run), n_iter=20, n_iter_per_test=10, tolerance=0,
                            e_step_thresh=1e-16)
        _equal(want[run * k:(run + 1) * k], V, "run %d against plsa_topics" % run)
    env(ENSTOP_AMD_ENSEMBLE="batched")                       # the A/B switch: "dask" takes the batched path
    got = amd.ensemble_of_topics(X, k, parallelism="dask", n_jobs=4, **kw)
    assert enstop_.last_ensemble_timing["path"] == "batched"
    _equal(got, want, "stack through ENSTOP_AMD_ENSEMBLE=batched")


# ------------------------------------------------------------------------------------------------
# 2. per-member stopping
# ------------------------------------------------------------------------------------------------
def stopping_corpus():
    rs = np.random.RandomState(3)
    T = rs.dirichlet(np.full(400, 0.05), 6)
    D = rs.dirichlet(np.full(6, 0.3), 600)
    return sp.csr_matrix(rs.poisson(60 * D @ T).astype(np.float32))


@pytest.mark.parametrize("per_test,n_iter,one_runs_out", [(1, 60, False), (1, 30, True), (2, 60, False), (10, 60, True)])
def test_members_stop_on_their_own_tests(amd, env, per_test, n_iter, one_runs_out):
    """Members that stop at DIFFERENT iterations (the strict CPU oracle stops them after 18, 29, 27, 23, 34, 21, 21, 25
    iterations with a test every iteration; 21, 31, 31, 27, 39, 23, 25, 29 with every second; 41, 41, 51, 41, 60, 41, 51, 41
    with every tenth -- the fifth runs to n_iter = 60, and to n_iter = 30 with a test every iteration).  The spread is
    asserted on the CLASSIC path's counts, so the comparison cannot pass vacuously."""
    X = stopping_corpus()
    assert X.nnz == 23560
    specs = [seeded_member(X, 6, 7 + r) for r in range(8)]
    fit_kw = dict(n_iter=n_iter, n_iter_per_test=per_test, tolerance=1e-3, e_step_thresh=1e-16)
    want, got = compare(amd, X, 6, specs, fit_kw, "stopping, test every %d of %d" % (per_test, n_iter))
    counts = [w[0] for w in want]
    print("classic iteration counts:", counts)
    assert len(set(counts)) >= 3, counts
    assert min(counts) < n_iter, counts
    if one_runs_out:
        assert max(counts) == n_iter and sum(c == n_iter for c in counts) < len(counts), counts
    assert [g[0] for g in got] == counts


# ------------------------------------------------------------------------------------------------
# 3. instantiation coverage
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 8, 20, 33, 64, 128])
def test_lane_shapes(amd, env, k):
    X = counts_corpus(seed=k)
    specs = [seeded_member(X, k, 100 + r) for r in range(4)]
    want, got = compare(amd, X, k, specs, FIT, "k=%d" % k)
    for g in got:
        assert not g[4]["row_wide"] and not g[4]["col_wide"]
        assert g[5] == dict(csr="packed", csc="packed")
        assert g[6]["group"] == 0 and g[6]["group_size"] == 4
    if k == 64:
        assert got[0][4]["row"][:2] == (8, 2) and got[0][4]["col"][:2] == (16, 1)


def tiny_members(k, n_members, n=320, m=240):
    """A corpus with a block of documents x words whose products P(w|z) P(z|d) lie near 2^-140: their responsibility norms
    are subnormal (thresh 0: the TINY rescue decides the result; 1e-32: thresholded away).  Every resample keeps the block's
    documents, and each member's P(z|d) rows follow its resample."""
    tiny_docs, n_tiny_words = (11, 12, 13, 14), 4
    rs = np.random.RandomState(500 + k)
    X = counts_corpus(n, m, seed=k).tolil()
    X[np.ix_(tiny_docs, np.arange(m - n_tiny_words, m))] = 3.0
    X = X.tocsr().astype(np.float32)
    U = rs.rand(n, k) + 0.05
    U /= U.sum(1, keepdims=True)
    V = rs.rand(k, m) + 0.05
    V /= V.sum(1, keepdims=True)
    U, V = U.astype(np.float32), V.astype(np.float32)
    U[list(tiny_docs)] = (2.0 ** -69 * (0.7 + 0.3 * rs.rand(len(tiny_docs), k))).astype(np.float32)
    V[:, m - n_tiny_words:] = (2.0 ** -70 * (0.7 + 0.3 * rs.rand(k, n_tiny_words))).astype(np.float32)
    specs = []
    for r in range(n_members):
        idx = rs.randint(0, n, size=n).astype(np.int64)
        idx[:len(tiny_docs)] = tiny_docs
        specs.append(dict(idx=idx, U=U[idx] * np.float32(1.0 + 0.01 * r), V=V))
    return X, specs


@pytest.mark.parametrize("thresh", [1e-32, 0.0])
@pytest.mark.parametrize("k", [20, 64])
def test_tiny_thresholds(amd, env, k, thresh):
    X, specs = tiny_members(k, 3)
    fit_kw = dict(n_iter=2, n_iter_per_test=1, tolerance=0.0, e_step_thresh=thresh)
    want, got = compare(amd, X, k, specs, fit_kw, "tiny block, k=%d thresh=%g" % (k, thresh))
    for w in want:
        assert np.isfinite(w[2]).all() and np.isfinite(w[3]).all()


def test_unpacked_streams_by_setting(amd, env):
    env(PLSA_PACKED=0)
    X = counts_corpus(seed=41)
    want, got = compare(amd, X, 20, [seeded_member(X, 20, 200 + r) for r in range(3)], FIT, "PLSA_PACKED=0")
    for g in got:
        assert g[5]["csr"] != "packed" and g[5]["csc"] != "packed" and g[6]["group"] == 0


def test_unpacked_streams_by_escapes(amd, env):
    X = counts_corpus(seed=42, fractional=0.3)          # more than 1/16 of the entries escape
    want, got = compare(amd, X, 20, [seeded_member(X, 20, 300 + r) for r in range(3)], FIT, "fractional counts")
    for g in got:
        assert g[5] == dict(csr="arrays", csc="arrays") and g[6]["group"] == 0 and g[6]["group_size"] == 3


def test_empty_documents_and_unused_words(amd, env):
    X = counts_corpus(seed=43, empty_docs=(7, 100, 299), unused_words=9)
    assert (np.diff(X.indptr) == 0).sum() == 3 and (np.diff(X.tocsc().indptr) == 0).sum() >= 9
    compare(amd, X, 8, [seeded_member(X, 8, 400 + r) for r in range(4)], FIT, "empty documents, unused words")


@pytest.mark.parametrize("settings,items", [(dict(PLSA_ROW_ITEMS=1, PLSA_ROW_SEG=16), True), (dict(PLSA_ROW_ITEMS=0), False)])
def test_row_items_forced_on_and_off(amd, env, settings, items):
    env(**settings)
    X = counts_corpus(seed=44)
    want, got = compare(amd, X, 20, [seeded_member(X, 20, 500 + r) for r in range(4)], FIT, "row items %s" % items)
    for g in got:
        assert g[6]["row_items"] == items and g[6]["group"] == 0
        if items:
            assert g[6]["row_item_entries"] == 16


def test_members_with_different_row_item_lengths(amd, env):
    """The row-item length follows a member's OWN non-zero count (ensure_ritems: 16 entries below 32 per group slot, 32 from
    there on; 65 536 slots at k = 20): a resample that favours the long documents lands above 2^21 entries, one that favours
    the short ones below -- one launch, two item lengths."""
    n, m, k = 1000, 20000, 20
    rs = np.random.RandomState(54)
    lengths = np.where(np.arange(n) < n // 2, 2500, 1700)
    cols = np.concatenate([rs.choice(m, L, replace=False) for L in lengths])
    rows = np.repeat(np.arange(n), lengths)
    X = sp.csr_matrix((rs.randint(1, 6, size=rows.shape[0]).astype(np.float32), (rows, cols)), shape=(n, m))
    U = rs.rand(n, k).astype(np.float32) + 0.05
    V = rs.rand(k, m).astype(np.float32) + 0.05
    U /= U.sum(1, keepdims=True)
    V /= V.sum(1, keepdims=True)
    specs = []
    for share_long in (0.75, 0.25, 0.7, 0.3):
        n_long = int(share_long * n)
        idx = np.concatenate([rs.randint(0, n // 2, size=n_long), rs.randint(n // 2, n, size=n - n_long)]).astype(np.int64)
        specs.append(dict(idx=idx, U=U[idx], V=V))
    want, got = compare(amd, X, k, specs, dict(n_iter=3, n_iter_per_test=1, tolerance=0.0, e_step_thresh=1e-16), "row item lengths")
    assert [g[6]["row_item_entries"] for g in got] == [32, 16, 32, 16], [g[6] for g in got]
    assert len({g[6]["row_grid"] for g in got}) == 4, [g[6]["row_grid"] for g in got]      # four grids in one launch
    assert all(g[6]["row_items"] and g[6]["group"] == 0 and g[6]["group_size"] == 4 for g in got)


def test_likelihood_partials_follow_the_members_own_grid(amd, env):
    """The fused log-likelihood leaves one float64 partial per workgroup of the member's document-pass grid and the final
    kernel adds them in order.  Counts spanning 2^-25 .. 2^25 make float64 sums of the float32 terms round (with counts of one
    magnitude every partial sum is exact), row items are forced on, and the members' item counts -- hence their grids --
    differ by a factor: each member's float64 likelihood must be the one it gets when fitted alone (compare()).
    Measured with the launch's x-extent substituted for every member's grid: this test still passes.  A grid below the
    cap (128 workgroups per CU) gives every group exactly one trip, so a larger grid only appends workgroups without work
    whose partials are 0.0, and a capped grid IS the launch's; the substitution cannot change a bit at any size."""
    env(PLSA_ROW_ITEMS=1, PLSA_ROW_SEG=16)
    n, m, k = 300, 500, 20
    X = counts_corpus(n, m, seed=55)
    rs = np.random.RandomState(56)
    X.data = (2.0 ** rs.uniform(-25, 25, size=X.nnz)).astype(np.float32)
    U = rs.rand(n, k).astype(np.float32) + 0.05
    V = rs.rand(k, m).astype(np.float32) + 0.05
    U /= U.sum(1, keepdims=True)
    V /= V.sum(1, keepdims=True)
    specs = []
    for copies_of_the_long_document in (0, 120, 40, 200):
        idx = rs.randint(0, n, size=n).astype(np.int64)
        idx[:copies_of_the_long_document] = 3
        specs.append(dict(idx=idx, U=U[idx], V=V))
    want, got = compare(amd, X, k, specs, dict(n_iter=4, n_iter_per_test=1, tolerance=0.0, e_step_thresh=1e-16), "likelihood grid")
    grids = [g[6]["row_grid"] for g in got]
    assert len(set(grids)) == 4 and max(grids) >= 2 * min(grids), grids
    assert all(g[6]["row_items"] and g[6]["group"] == 0 and g[5] == dict(csr="arrays", csc="arrays") for g in got)


def test_heavy_columns(amd, env):
    env(PLSA_HEAVY_ITEMS=2, PLSA_COL_SEG=8)
    X = counts_corpus(seed=45)
    want, got = compare(amd, X, 20, [seeded_member(X, 20, 600 + r) for r in range(4)], FIT, "heavy columns")
    for g in got:
        assert g[6]["heavy_columns"] > 0 and g[6]["group"] == 0


def test_forced_wide_tables_take_the_classic_loop(amd, env):
    """64-bit gather tables are not carried by a batch (include/plsa_hip_members.h): every member runs through plsa_fit"""
    env(PLSA_FORCE_WIDE=1)
    X = counts_corpus(seed=46)
    want, got = compare(amd, X, 20, [seeded_member(X, 20, 700 + r) for r in range(3)], FIT, "PLSA_FORCE_WIDE", expect_batched=False)
    for g in got:
        assert g[4]["row_wide"] and g[4]["col_wide"] and g[6]["group"] == -1


def test_two_stage_norm(amd, env):
    """members with more than 2048 chunk rows of the column pass: norm_pwz in two stages, the first cut by the MEMBER's grid"""
    rs = np.random.RandomState(47)
    n, m, k, e = 1500, 60000, 64, 220000
    rows = rs.randint(0, n, size=e)
    cols = np.concatenate([np.arange(m), rs.randint(0, m, size=e - m)])
    X = sp.csr_matrix((np.ones(e, np.float32), (rows, cols)), shape=(n, m))
    X.sum_duplicates()
    want, got = compare(amd, X, k, [seeded_member(X, k, 800 + r) for r in range(3)],
                        dict(n_iter=3, n_iter_per_test=1, tolerance=0.0, e_step_thresh=1e-16), "two-stage norm")
    for g in got:
        assert g[6]["col_chunks"] > 2048 and g[6]["norm_blocks"] >= 64 and g[6]["group"] == 0
    assert len({g[6]["col_chunks"] for g in got}) > 1          # chunk counts differ between the resamples


# ------------------------------------------------------------------------------------------------
# 4. a batch whose members fall into different instantiation groups
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fractional", [2, 1])
def test_mixed_batch(amd, env, n_fractional):
    """resamples of the integer half of a corpus keep their packed streams, resamples of the half with fractional counts
    lose them (more than 1/16 escapes): two launch groups -- or, with a single such member, one group and the classic loop"""
    n, m, k = 400, 500, 20
    A = counts_corpus(n // 2, m, seed=48)
    B = counts_corpus(n // 2, m, seed=49, fractional=0.5)
    X = sp.vstack([A, B]).tocsr()
    rs = np.random.RandomState(50)
    U = rs.rand(n, k).astype(np.float32) + 0.05
    V = rs.rand(k, m).astype(np.float32) + 0.05
    U /= U.sum(1, keepdims=True)
    V /= V.sum(1, keepdims=True)
    specs = []
    for r in range(5):
        lo = n // 2 if r < n_fractional else 0
        idx = rs.randint(lo, lo + n // 2, size=n).astype(np.int64)
        specs.append(dict(idx=idx, U=U[idx], V=V))
    from enstop_amd.engine import get_engine
    eng = get_engine()
    got, batch = _batched(eng, X, k, specs, FIT)
    want = [_classic(eng, X, k, spec, FIT) for spec in specs]
    for j, (w, g) in enumerate(zip(want, got)):
        assert g[0] == w[0]
        _equal(g[1], w[1], "mixed member %d trace" % j)
        _equal(g[3], w[3], "mixed member %d P(w|z)" % j)
        _equal(g[2], w[2], "mixed member %d P(z|d)" % j)
        assert g[5] == w[5] == (dict(csr="arrays", csc="arrays") if j < n_fractional else dict(csr="packed", csc="packed"))
    sizes = [g[6]["group_size"] if g[6]["group"] >= 0 else 1 for g in got]
    assert sizes == [n_fractional] * n_fractional + [5 - n_fractional] * (5 - n_fractional), sizes
    assert batch.last_batched == (5 if n_fractional > 1 else 4)
    assert (got[0][6]["group"] == -1) == (n_fractional == 1)
    assert got[0][6]["group"] != got[-1][6]["group"]


# ------------------------------------------------------------------------------------------------
# 5. fallbacks
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["reference", "materialised", "cells"])
def test_ineligible_calls_take_the_contexts(amd, env, monkeypatch, case):
    from enstop_amd import enstop_
    X = counts_corpus(seed=51)
    kw = dict(n_runs=5, random_state=3, n_iter=6, n_iter_per_test=2, tolerance=0, e_step_thresh=1e-16)
    if case == "reference":
        kw["arithmetic"] = "reference"
    elif case == "materialised":
        kw["flags"] = 0
    else:
        monkeypatch.setenv("ENSTOP_AMD_CONCURRENT_MEMBERS_CELLS", "1000")
        monkeypatch.setattr(enstop_, "CONCURRENT_MEMBERS_CELLS", 1000.0)      # (read from the environment at import)
    got = amd.ensemble_of_topics(X, 8, parallelism="batched", **kw)
    t = dict(enstop_.last_ensemble_timing)
    assert t["path"] == "contexts" and t["batch"] == 1 and "groups" not in t, t
    want = amd.ensemble_of_topics(X, 8, parallelism="dask", n_jobs=1, **kw)
    _equal(got, want, case)
    if case == "cells":       # ... and the same call is carried once the limit allows it
        monkeypatch.setattr(enstop_, "CONCURRENT_MEMBERS_CELLS", 2e9)
        again = amd.ensemble_of_topics(X, 8, parallelism="batched", **kw)
        assert enstop_.last_ensemble_timing["path"] == "batched"
        _equal(again, want, "eligible again")


def test_unknown_parallelism_is_still_an_error(amd):
    with pytest.raises(ValueError, match="batched"):
        amd.ensemble_of_topics(counts_corpus(), 4, n_runs=2, parallelism="threads")


# ------------------------------------------------------------------------------------------------
# 6. the estimator
# ------------------------------------------------------------------------------------------------
def test_ensemble_topics_estimator(amd, env):
    from enstop_amd import enstop_
    with amd.Engine() as e:       # the planted-topics corpus of tests/test_planted_topics.py
        e.generate_synthetic(6000, 3000, 330_000, seed=3, topics=8, alpha=0.05, background=0.1)
        X = e.download_active_csr().astype(np.int64)
    out = {}
    for par in ("dask", "batched"):
        et = amd.EnsembleTopics(n_components=20, n_starts=32, parallelism=par, topic_combination="hellinger", n_iter=30,
                                random_state=1)
        et.fit(X)
        out[par] = np.array(et.components_)
        assert enstop_.last_ensemble_timing["path"] == ("batched" if par == "batched" else "contexts")
    assert out["dask"].shape == out["batched"].shape
    np.testing.assert_array_equal(out["batched"], out["dask"])


# ------------------------------------------------------------------------------------------------
# 7. lifecycle
# ------------------------------------------------------------------------------------------------
def test_two_ensembles_on_one_engine_then_a_classic_fit(amd, env):
    from enstop_amd import enstop_
    from enstop_amd.engine import get_engine
    X1, X2 = counts_corpus(300, 500, seed=52), counts_corpus(450, 350, seed=53)
    kw = dict(random_state=11, n_iter=6, n_iter_per_test=2, tolerance=0, e_step_thresh=1e-16)
    first = amd.ensemble_of_topics(X1, 20, n_runs=6, parallelism="batched", **kw)
    get_engine().release_scratch()
    second = amd.ensemble_of_topics(X2, 7, n_runs=9, parallelism="batched", **kw)
    assert enstop_.last_ensemble_timing["path"] == "batched" and enstop_.last_ensemble_timing["groups"] == [[9]]
    U, V = amd.plsa_fit(X1, 20, None, random_state=5, **{key: v for key, v in kw.items() if key != "random_state"})
    again = amd.ensemble_of_topics(X1, 20, n_runs=6, parallelism="batched", **kw)       # the batch's slots are re-used
    _equal(again, first, "the same ensemble again")
    env()                                                                              # fresh engines
    _equal(amd.ensemble_of_topics(X1, 20, n_runs=6, parallelism="dask", n_jobs=1, **kw), first, "first ensemble")
    _equal(amd.ensemble_of_topics(X2, 7, n_runs=9, parallelism="dask", n_jobs=1, **kw), second, "second ensemble")
    U2, V2 = amd.plsa_fit(X1, 20, None, random_state=5, **{key: v for key, v in kw.items() if key != "random_state"})
    _equal(U, U2, "classic fit after the batches: P(z|d)")
    _equal(V, V2, "classic fit after the batches: P(w|z)")
