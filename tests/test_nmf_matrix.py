"""Every instantiation of the Kullback-Leibler NMF passes, the combined pass, degenerate shapes and reused contexts.

tests/test_nmf_device.py holds the NMF kernels (csrc/plsa_nmf_kernels.hpp) to the float64 restatement of scikit-learn's
multiplicative updates (tests/nmf_reference.py, pinned by tests/test_nmf_host.py) at seven topic counts.  The kernels are a
family of template instantiations on the EM passes' Shape<> types: lane shape (LPN, CH), FULL or run-time kp, WIDE or
narrow gathers, Packed<S> or the two index arrays, whole documents or row items.  This file runs all of them:

  1. CPU: K_NMF = [1, 2] + K_MATRIX reaches every (lane shape, FULL) pair of both passes; edge_corpus(k) keeps its fixture
     margins at every k of it; a float32 NumPy emulation of both halves stays inside the bound; the checker rejects five
     kinds of wrong result on the float64 reference alone.
  2. GPU: the instantiation matrix.  Per k, one Engine per setting of test_pass_matrix.SETTINGS (default, wide, arrays,
     wide_arrays, row_items, heavy) plus row_items and heavy with PLSA_FORCE_WIDE=1 and with PLSA_PACKED=0: both halves and
     the objective entry for entry, the zero pattern, the instantiations read back from pass_info() / packed_info() / the
     timing names, the same bits wherever the operations are the same.
  3. GPU: the combined pass (k_nmf_row_pass with iters > 1) and the driver at one k per (document-pass shape, FULL) pair:
     25 iterates by hand against plsa_nmf_fit, launch counts from the timing table.
  4. GPU: degenerate shapes (1 x 1, one document, one word, k above both dimensions, all-zero and absent entries).
  5. GPU: one walk over ONE context (k up and down, release_scratch, bootstrap, pLSA in between, a refused call, row-item
     mode entered and left), every step against a context of its own, bit for bit.

Bounds (the error model of tests/test_nmf_device.py, u = 2^-24): half-iterations |got - want| <= 4 (L + k) u |want| with
zeros exactly where the reference has zeros, L the longest row (W) or column (H) -- the sums add non-negative terms, so the
bound holds for any order (row items, heavy columns); objective |got^2 / 2 - D| <= 4 (k + 1) u sum x max(1, |log(x / wh)|).
Where every stored entry is zero (or none is stored) that sum is 0 and D = W_sum . H_sum, float64 on both sides: two float64
sums of n and m non-negative float32 values, k products and their sum, each within (n + m + k + 2) 2^-53 of the exact
value relative to it, so the two sides differ by at most 2 (n + m + k + 2) 2^-53 D.

Needs a real MI355X except for part 1.
"""
import functools
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import nmf_reference as R
from test_nmf_device import U24, _assert_fixture_margins, _bits, _check_half, _halves
from test_pass_matrix import DEFAULT_SHAPES, K_MATRIX, KNOBS, SETTINGS, lane_shape

K_NMF = [1, 2] + K_MATRIX
U53 = 2.0 ** -53


def _is_full(kp, shape):
    return kp == 4 * shape[0] * shape[1]


def _one_k_per_row_instantiation():
    """the LAST k of K_NMF for every (document-pass shape, FULL) pair: topics 1 and 2 of edge_corpus are dead from the first
    iteration on, so k = 1, 2, 3 leave one live topic, whose W converges in a single update -- k = 4 keeps the objective
    falling through iteration 20, which the stop test at tol = 1e-30 needs"""
    last = {}
    for k in K_NMF:
        kp, _, row = lane_shape(k)
        last[row, _is_full(kp, row)] = k
    return sorted(last.values())


K_COMBINED = _one_k_per_row_instantiation()

# Engines of the matrix: the six settings, then row_items and heavy crossed with the two knobs that must not change a bit
MATRIX_ENGINES = {name: SETTINGS[name] for name in ("default", "wide", "arrays", "wide_arrays", "row_items", "heavy")}
for _base in ("row_items", "heavy"):
    MATRIX_ENGINES[_base + "+wide"] = dict(SETTINGS[_base], PLSA_FORCE_WIDE="1")
    MATRIX_ENGINES[_base + "+arrays"] = dict(SETTINGS[_base], PLSA_PACKED="0")
SAME_BITS_AS = {"wide": "default", "arrays": "default", "wide_arrays": "default",
                "row_items+wide": "row_items", "row_items+arrays": "row_items",
                "heavy+wide": "heavy", "heavy+arrays": "heavy"}


# ------------------------------------------------------------------------------------------------
# shared references (computed once, read-only) and the checks
# ------------------------------------------------------------------------------------------------
class Ref:
    """edge_corpus(k) with the float64 W half, its unclamped (WH) and the objective at the start"""

    def __init__(self, X, W0, H0):
        self.X, self.W0, self.H0 = X, W0, H0
        self.k = W0.shape[1]
        self.L_row = int(np.diff(X.indptr).max(initial=0))
        self.L_col = int(np.diff(X.tocsc().indptr).max(initial=0))
        d = {}
        self.Ww, self.Hw = R.step64(X, W0, H0, details=d)
        self.wh_w, self.wh_h, self.H_unclamped = d["wh"][0], d["wh"][1], d["H_unclamped"]
        self.D, self.scale = R.divergence64(X, W0, H0, want_d=True)
        for a in (W0, H0, self.Ww, self.Hw, self.wh_w):
            a.setflags(write=False)

    def assert_margins(self):
        """every (WH) is 0 or at least 2 EPS32, every updated H entry 0 or at least 2 EPS64, on the float64 step"""
        _assert_fixture_margins(dict(wh=[self.wh_w, self.wh_h], H_unclamped=self.H_unclamped), self.Hw)

    def h_half(self, W1):
        """the H half from the W a device returned, with the margins on THAT reference"""
        d = {}
        _, Hw = R.step64_h(self.X, W1, self.H0, details=d)
        _assert_fixture_margins(dict(wh=[self.wh_w] + d["wh"], H_unclamped=d["H_unclamped"]), Hw)
        return Hw


@functools.lru_cache(maxsize=None)
def reference(k):
    return Ref(*R.edge_corpus(k))


def _ratio(got, want, L, k):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nz = want != 0
    return float((np.abs(got - want)[nz] / (4.0 * (L + k) * U24 * np.abs(want[nz]))).max()) if nz.any() else 0.0


def _held(got, want, L, k, what, worst=None, key=None):
    """_check_half, and the worst error over bound kept for the report; an all-zero reference wants all zeros"""
    if not np.asarray(want).any():
        assert not np.asarray(got).any(), what
        return 0.0
    _check_half(got, want, L, k, what)
    r = _ratio(got, want, L, k)
    if worst is not None:
        worst[key] = max(worst.get(key, 0.0), r)
    return r


def _held_objective(got, D, scale, k, what, worst=None, key=None):
    bound = 4.0 * (k + 1) * U24 * scale
    err = abs(got * got / 2.0 - D)
    print("%s: D = %.6e, device %.6e, error / bound = %.3g" % (what, D, got * got / 2.0, err / bound))
    assert err <= bound, (what, got, D, err, bound)
    if worst is not None:
        worst[key] = max(worst.get(key, 0.0), err / bound)


def _same(a, b, what):
    for key in sorted(set(a) & set(b)):
        if isinstance(a[key], np.ndarray):
            assert a[key].shape == b[key].shape, (what, key)
            assert np.array_equal(_bits(a[key]), _bits(b[key])), (what, key)
        elif isinstance(a[key], (float, int, list)):
            assert a[key] == b[key], (what, key, a[key], b[key])


# ------------------------------------------------------------------------------------------------
# 1. CPU
# ------------------------------------------------------------------------------------------------
def test_k_nmf_reaches_every_instantiation_of_both_passes():
    """K_NMF covers every (lane shape, FULL) pair that lane_shape produces for 1 <= k <= 1024, for the column pass and
    for the document pass (the divergence and the row reduction run in the document pass' shape), k = 1 and k = 2, and
    kp == k as well as padded kp; K_COMBINED holds one k of every document-pass pair"""
    reach_col, reach_row = set(), set()
    for k in range(1, 1025):
        kp, col, row = lane_shape(k)
        reach_col.add((col, _is_full(kp, col)))
        reach_row.add((row, _is_full(kp, row)))
    cover_col, cover_row, padded = set(), set(), set()
    for k in K_NMF:
        kp, col, row = lane_shape(k)
        cover_col.add((col, _is_full(kp, col)))
        cover_row.add((row, _is_full(kp, row)))
        if kp != k:
            padded.add(col)
    assert sorted({s for s, _ in reach_col}) == sorted(DEFAULT_SHAPES)
    assert reach_col == cover_col and reach_row == cover_row
    assert ((8, 2), True) in cover_row and ((16, 1), True) in cover_col and ((16, 1), True) not in cover_row
    assert {1, 2} <= set(K_NMF) and lane_shape(1)[1:] == ((1, 1), (1, 1)) == lane_shape(2)[1:]
    assert padded == {(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 2), (64, 4)}
    combined = {(lane_shape(k)[2], _is_full(lane_shape(k)[0], lane_shape(k)[2])) for k in K_COMBINED}
    assert combined == reach_row and len(K_COMBINED) == len(reach_row) <= 17 and set(K_COMBINED) <= set(K_NMF)


def _halves32(X, W0, H0):
    """both halves in float32 NumPy (sums in NumPy's / SciPy's order, H_sum and W_sum in float64 rounded once)"""
    X = sp.csr_matrix(X)
    rows = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    x = X.data.astype(np.float32)

    def quotient(W, H):
        wh = np.multiply(W[rows, :], H.T[X.indices, :]).sum(axis=1, dtype=np.float32)
        wh[wh < np.float32(R.EPS32)] = np.float32(R.EPS32)
        return sp.csr_matrix((x / wh, X.indices, X.indptr), shape=X.shape)

    num = np.asarray(quotient(W0, H0) @ np.ascontiguousarray(H0.T))
    hs = H0.sum(axis=1, dtype=np.float64).astype(np.float32)
    hs[hs == 0] = np.float32(R.EPS32)
    W1 = W0 * (num / hs[None, :])
    num = np.asarray(quotient(W1, H0).T @ W1).T
    ws = W1.sum(axis=0, dtype=np.float64).astype(np.float32)
    ws[ws == 0] = np.float32(1.0)
    H1 = H0 * (num / ws[:, None])
    H1[H1 < np.float32(R.EPS64)] = 0
    assert W1.dtype == np.float32 and H1.dtype == np.float32
    return W1, H1


@pytest.mark.parametrize("k", K_NMF)
def test_edge_corpus_keeps_its_margins_and_float32_stays_inside_the_bound(k):
    ref = reference(k)
    assert ref.L_row > 64 and ref.L_col > 256
    assert np.diff(ref.X.indptr)[5] == 0 and np.diff(ref.X.tocsc().indptr)[9] == 0 and (ref.X.data == 0).sum() >= 20
    ref.assert_margins()
    W1, H1 = _halves32(ref.X, ref.W0, ref.H0)
    Ww, _ = R.step64(ref.X, ref.W0, ref.H0, update_H=False)
    assert np.array_equal(Ww, ref.Ww)
    _held(W1, Ww, ref.L_row, k, "float32 emulation, W half, k = %d" % k)
    _held(H1, ref.h_half(W1), ref.L_col, k, "float32 emulation, H half, k = %d" % k)


def test_the_checker_rejects_wrong_results(monkeypatch):
    """on the float64 reference alone: each of five wrong results makes _check_half raise, the right one passes"""
    k = 6
    ref = reference(k)
    X, W0, H0, Ww, Hw = ref.X, ref.W0, ref.H0, ref.Ww, ref.Hw
    _check_half(Ww, Ww, ref.L_row, k, "W, unperturbed")
    _check_half(Hw, Hw, ref.L_col, k, "H, unperturbed")
    # an H half computed from the OLD W
    _, H_old = R.step64_h(X, W0, H0)
    with pytest.raises(AssertionError):
        _check_half(H_old, Hw, ref.L_col, k, "H from the old W")
    # one column's numerator without one 16-entry item: word 0 sits in every non-empty document
    Xc = X.tocsc(copy=True)
    assert Xc.indptr[1] - Xc.indptr[0] > 256
    Xc.data[Xc.indptr[0] + 32:Xc.indptr[0] + 48] = 0
    _, H_short = R.step64_h(Xc.tocsr(), Ww, H0)
    assert np.array_equal(H_short[:, 1:], Hw[:, 1:])
    with pytest.raises(AssertionError):
        _check_half(H_short, Hw, ref.L_col, k, "H without one item of word 0")
    # a non-zero value where the reference has a zero row
    for z in (1, 2):
        W_bad = Ww.copy()
        assert not Ww[3].any()
        W_bad[3, z] = 1e-30
        with pytest.raises(AssertionError):
            _check_half(W_bad, Ww, ref.L_row, k, "W[3, %d] not zero" % z)
    # a padding-sized error: one entry off by 8 (L + k) u, twice its bound
    d, z = np.argwhere(Ww != 0)[17]
    W_bad = Ww.copy()
    W_bad[d, z] *= 1.0 + 8.0 * (ref.L_row + k) * U24
    with pytest.raises(AssertionError):
        _check_half(W_bad, Ww, ref.L_row, k, "one entry off by twice the bound")
    W_ok = Ww.copy()
    W_ok[d, z] *= 1.0 + 2.0 * (ref.L_row + k) * U24
    _check_half(W_ok, Ww, ref.L_row, k, "one entry off by half the bound")
    # a W half without the EPS32 clamp, where it matters: document 7's W row is tiny, its (WH) fall below EPS32
    Wp, Hp = R.planted_start(X.shape[0], X.shape[1], k)
    Wp[7] *= np.float32(1e-9)
    d = {}
    W_clamped, _ = R.step64(X, Wp, Hp, update_H=False, details=d)
    rows = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    assert (d["wh"][0][rows == 7] < R.EPS32 / 2).all() and (d["wh"][0][rows != 7] >= 2 * R.EPS32).all()
    monkeypatch.setattr(R, "EPS32", 0.0)
    W_free, _ = R.step64(X, Wp, Hp, update_H=False)
    monkeypatch.undo()
    assert np.array_equal(np.delete(W_free, 7, axis=0), np.delete(W_clamped, 7, axis=0))
    _check_half(W_clamped, W_clamped, ref.L_row, k, "W with the clamp")
    with pytest.raises(AssertionError):
        _check_half(W_free, W_clamped, ref.L_row, k, "W without the clamp")


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


@pytest.fixture(scope="module")
def worst():
    out = {}
    yield out
    for q in ("W", "H", "D"):
        per_k = {key[1]: v for key, v in out.items() if key[0] == q}
        if per_k:
            at = max(per_k, key=per_k.get)
            print("\nNMF matrix: worst error / bound of %s: %.3g at k = %d (%s)" % (
                q, per_k[at], at, ", ".join("k=%d %.3g" % kv for kv in sorted(per_k.items()))))


def _engine(amd, monkeypatch, env):
    """a context with exactly the knobs of `env` (PLSA_* are read when it is created)"""
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    return amd.Engine()


def _fit(eng, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        n_iter, errors = eng.nmf_fit(**kw)
    return n_iter, [float(e) for e in errors]


def _matrix_run(eng, ref, repeat):
    W1, H1, names, info, packed = _halves(eng, ref.X, ref.W0, ref.H0)
    if repeat:                                          # the same context, from the same start: the same bits
        W1r, H1r, _, _, _ = _halves(eng, ref.X, ref.W0, ref.H0)
        assert np.array_equal(_bits(W1), _bits(W1r)) and np.array_equal(_bits(H1), _bits(H1r))
    eng.nmf_set_factors(ref.W0, ref.H0)
    eng.timing(True)
    eng.timing_reset()
    d = eng.nmf_divergence()
    again = eng.nmf_divergence()
    names_d = set(eng.timing_report())
    eng.timing(False)
    assert d == again
    return dict(W1=W1, H1=H1, d=d, names=names, names_d=names_d, info=info, packed=packed)


@pytest.mark.gpu
@pytest.mark.parametrize("k", K_NMF)
def test_nmf_instantiation_matrix(amd, monkeypatch, worst, k):
    ref = reference(k)
    ref.assert_margins()
    assert ref.L_row > 64 and ref.L_col > 256
    kp, col_shape, row_shape = lane_shape(k)
    row_full, col_full = _is_full(kp, row_shape), _is_full(kp, col_shape)
    results, h_refs = {}, {}
    seen = dict(row_pass=set(), row_reduce=set(), divergence=set(), col_pass=set())
    for name, env in MATRIX_ENGINES.items():
        tag = "k = %d, %s" % (k, name)
        with _engine(amd, monkeypatch, env) as eng:
            got = results[name] = _matrix_run(eng, ref, repeat=(name == "default"))
            if "PLSA_HEAVY_ITEMS" in env:
                lens = np.diff(ref.X.tocsc().indptr)
                assert eng.balance_info()["item_entries"] == 8
                assert ((lens + 7) // 8 > 2).sum() >= 1           # columns on the one-block-per-column path of k_col_reduce
        W1, H1 = got["W1"], got["H1"]
        # -- both halves and the objective, entry for entry
        _held(W1, ref.Ww, ref.L_row, k, "W half, " + tag, worst, ("W", k))
        key = W1.tobytes()
        if key not in h_refs:
            h_refs[key] = ref.h_half(W1)
        _held(H1, h_refs[key], ref.L_col, k, "H half, " + tag, worst, ("H", k))
        _held_objective(got["d"], ref.D, ref.scale, k, "objective, " + tag, worst, ("D", k))
        assert ref.D > 0
        # -- exact zeros: empty document 5 and empty word 9, and from k = 3 on the zero W row, W column and H rows
        assert not W1[5].any() and not H1[:, 9].any(), tag
        assert not W1[3].any(), tag
        if k >= 3:
            assert not W1[:, 1].any() and not H1[2].any() and not H1[1].any(), tag
        # -- which instantiations ran
        info, names = got["info"], got["names"]
        wide = env.get("PLSA_FORCE_WIDE") == "1"
        packed = env.get("PLSA_PACKED") != "0"
        items = env.get("PLSA_ROW_ITEMS") == "1"
        assert info["row"] == (row_shape[0], row_shape[1], row_full), (tag, info)
        assert info["col"] == (col_shape[0], col_shape[1], col_full), (tag, info)
        assert info["row_wide"] == wide and info["col_wide"] == wide, (tag, info)
        assert got["packed"] == (dict(csr="packed", csc="packed") if packed else dict(csr="arrays", csc="arrays")), (tag, got["packed"])
        assert {"k_nmf_row_pass", "k_nmf_col_pass", "k_nmf_h_finish", "k_col_reduce"} <= names, (tag, names)
        assert ("k_nmf_row_reduce" in names) == items, (tag, names)
        assert {"k_nmf_divergence", "k_nmf_divergence_final"} <= got["names_d"], (tag, got["names_d"])
        row_inst = (info["row"][:2], info["row"][2] and not info["row_wide"], info["row_wide"])
        col_inst = (info["col"][:2], info["col"][2] and not info["col_wide"], info["col_wide"])
        seen["row_pass"].add(row_inst + (got["packed"]["csr"] == "packed",))
        seen["col_pass"].add(col_inst + (got["packed"]["csc"] == "packed",))
        seen["divergence"].add(row_inst)                # (the objective reads the two arrays whatever the streams are)
        if "k_nmf_row_reduce" in names:
            seen["row_reduce"].add(row_inst)
    # -- the same arithmetic, bit for bit
    for name, base in SAME_BITS_AS.items():
        _same({key: results[name][key] for key in ("W1", "H1", "d")}, results[base], "k = %d: %s against %s" % (k, name, base))
    # -- every (shape, FULL, WIDE, packed) instantiation that k reaches
    both = (False, True)
    assert seen["row_pass"] == {(row_shape, row_full and not w, w, p) for w in both for p in both}
    assert seen["col_pass"] == {(col_shape, col_full and not w, w, p) for w in both for p in both}
    assert seen["row_reduce"] == seen["divergence"] == {(row_shape, row_full and not w, w) for w in both}
    print("\nk = %d rows %s cols %s: worst error / bound W %.3g, H %.3g, objective %.3g" % (
        k, row_shape, col_shape, worst["W", k], worst["H", k], worst["D", k]))


# ------------------------------------------------------------------------------------------------
# 3. the combined pass and the driver
# ------------------------------------------------------------------------------------------------
N_HAND = 25
FIXED_H_ITERS = (1, 9, 10, 11, 20, 25)
UPDATED_H_ITERS = (1, 10, 11)


def _launches(eng, name):
    return eng.timing_get(name)[1]


def _combined_run(eng, ref, items):
    X, W0, H0 = ref.X, ref.W0, ref.H0
    eng.upload_csr(X)
    eng.nmf_set_factors(W0, H0)
    out = dict(e0=eng.nmf_divergence())
    # -- H fixed, by hand: 25 lone passes, every iterate kept
    hand, e = [], {}
    for it in range(1, N_HAND + 1):
        eng.nmf_update_w()
        hand.append(eng.nmf_get_factors(want_h=False)[0])
        if it in (10, 20):
            e[it] = eng.nmf_divergence()
    tested = [out["e0"], e[10], e[20]]
    assert tested[0] - tested[1] > 1e-6 * tested[0] and tested[1] - tested[2] > 1e-6 * tested[0], tested   # still falling
    eng.timing(True)
    for n in FIXED_H_ITERS:
        for tol in (0.0, 1e-30):
            what = "k = %d, max_iter = %d, tol = %g" % (ref.k, n, tol)
            eng.nmf_set_factors(W0, H0)
            eng.timing_reset()
            n_iter, errors = _fit(eng, update_h=False, max_iter=n, tol=tol)
            passes, reduces = _launches(eng, "k_nmf_row_pass"), _launches(eng, "k_nmf_row_reduce")
            W, H = eng.nmf_get_factors()
            assert n_iter == n, what
            assert np.array_equal(_bits(W), _bits(hand[n - 1])), what
            assert np.array_equal(_bits(H), _bits(H0)), what
            assert errors == (tested[:1 + n // 10] if tol > 0 else tested[:1]), (what, errors, tested)
            if items:                                   # row items: one launch and one reduction per iteration
                assert (passes, reduces) == (n, n), (what, passes, reduces)
            else:                                       # the combined pass: one launch up to the next test, or to the end
                assert (passes, reduces) == ((n + 9) // 10 if tol > 0 else 1, 0), (what, passes, reduces)
            assert _launches(eng, "k_nmf_col_pass") == 0 and _launches(eng, "k_nmf_h_finish") == 0, what
    eng.timing(False)
    out["hand_w"] = np.stack(hand)
    out["errors_w"] = tested
    # -- H updated: the alternating entry points by hand, then the driver
    eng.nmf_set_factors(W0, H0)
    alt, e10 = [], None
    for it in range(1, max(UPDATED_H_ITERS) + 1):
        eng.nmf_update_w()
        eng.nmf_update_h()
        alt.append(eng.nmf_get_factors())
        if it == 10:
            e10 = eng.nmf_divergence()
    assert out["e0"] - e10 > 1e-6 * out["e0"]
    eng.timing(True)
    for n in UPDATED_H_ITERS:
        what = "k = %d, H updated, max_iter = %d" % (ref.k, n)
        eng.nmf_set_factors(W0, H0)
        eng.timing_reset()
        n_iter, errors = _fit(eng, update_h=True, max_iter=n, tol=1e-30)
        counts = [_launches(eng, name) for name in ("k_nmf_row_pass", "k_nmf_row_reduce", "k_nmf_col_pass", "k_nmf_h_finish")]
        W, H = eng.nmf_get_factors()
        assert n_iter == n, what
        assert np.array_equal(_bits(W), _bits(alt[n - 1][0])) and np.array_equal(_bits(H), _bits(alt[n - 1][1])), what
        assert errors == ([out["e0"], e10] if n >= 10 else [out["e0"]]), (what, errors)
        assert counts == [n, n if items else 0, n, n], (what, counts)
    eng.timing(False)
    out["alt_w"] = np.stack([w for w, _ in alt])
    out["alt_h"] = np.stack([h for _, h in alt])
    out["e10_alt"] = e10
    out["info"], out["packed"] = eng.pass_info(), eng.packed_info()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k", K_COMBINED)
def test_combined_pass_and_driver(amd, monkeypatch, k):
    """plsa_nmf_fit with H fixed is ONE launch of k_nmf_row_pass per stretch between two stopping tests (read from the
    timing table), and its result is, bit for bit, that many lone passes; with H updated, and over row items, the driver
    equals the entry points called by hand, launch for launch"""
    ref = reference(k)
    kp, _, row_shape = lane_shape(k)
    row_full = _is_full(kp, row_shape)
    got = {}
    for name in ("default", "wide_arrays", "row_items"):
        with _engine(amd, monkeypatch, SETTINGS[name]) as eng:
            got[name] = _combined_run(eng, ref, items=(name == "row_items"))
        info, wide = got[name]["info"], name == "wide_arrays"
        assert info["row"] == (row_shape[0], row_shape[1], row_full) and info["row_wide"] == wide == info["col_wide"], (name, info)
        assert got[name]["packed"]["csr"] == ("arrays" if name == "wide_arrays" else "packed"), (name, got[name]["packed"])
    _same(got["default"], got["wide_arrays"], "k = %d: wide_arrays against default" % k)
    # row items cut the sums differently: their first iterate is held to the reference, like the matrix holds it
    for name in got:
        _held(got[name]["hand_w"][0], ref.Ww, ref.L_row, k, "first iterate, k = %d, %s" % (k, name))


# ------------------------------------------------------------------------------------------------
# 4. degenerate shapes
# ------------------------------------------------------------------------------------------------
def _dense_counts(n, m, seed):
    rs = np.random.RandomState(seed)
    X = sp.csr_matrix(rs.randint(1, 6, size=(n, m)).astype(np.float32))
    assert X.nnz == n * m
    return X


def _one_document(m=600, entries=500, seed=21):
    rs = np.random.RandomState(seed)
    cols = np.sort(rs.choice(m, entries, replace=False)).astype(np.int32)
    return sp.csr_matrix((rs.randint(1, 6, size=entries).astype(np.float32), cols, np.array([0, entries], np.int32)), shape=(1, m))


def _stored_zeros(n=40, m=30, seed=22):
    rs = np.random.RandomState(seed)
    r, c = np.nonzero(rs.rand(n, m) < 0.2)
    X = sp.csr_matrix((np.zeros(r.shape[0], np.float32), (r, c)), shape=(n, m))
    assert X.nnz == r.shape[0] > 100 and not X.data.any()
    return X


DEGENERATE = {
    # name: (corpus, k, knobs, kernels that must / must not have run)
    "1x1": (lambda: sp.csr_matrix(np.array([[3.0]], np.float32)), 1, {}, None),
    "one_document": (_one_document, 5, {"PLSA_ROW_ITEMS": "0"}, False),
    "one_document_row_items": (_one_document, 5, {"PLSA_ROW_ITEMS": "1"}, True),
    "one_word": (lambda: _dense_counts(700, 1, 23), 5, {}, None),
    "one_word_heavy": (lambda: _dense_counts(700, 1, 23), 5, SETTINGS["heavy"], None),
    "k64_above_3x2": (lambda: _dense_counts(3, 2, 24), 64, {}, None),
    "k700_above_3x2": (lambda: _dense_counts(3, 2, 24), 700, {}, None),
}


def _degenerate_check(eng, X, W0, H0, what):
    """both halves and the objective of one small case, margins on the float64 step first"""
    ref = Ref(X, W0, H0)
    ref.assert_margins()
    k = ref.k
    W1, H1, names, info, _ = _halves(eng, X, W0, H0)
    eng.nmf_set_factors(W0, H0)
    d = eng.nmf_divergence()
    assert d == eng.nmf_divergence()
    _, col_shape, row_shape = lane_shape(k)
    assert info["row"][:2] == row_shape and info["col"][:2] == col_shape, (what, info)
    _held(W1, ref.Ww, ref.L_row, k, "W half, " + what)
    _held(H1, ref.h_half(W1), ref.L_col, k, "H half, " + what)
    if ref.scale > 0:
        _held_objective(d, ref.D, ref.scale, k, "objective, " + what)
    else:       # no positive entry: D = W_sum . H_sum, float64 on both sides (module docstring)
        n, m = X.shape
        assert ref.D > 0 and not (X.data > 0).any()
        assert abs(d * d / 2.0 - ref.D) <= 2.0 * (n + m + k + 2) * U53 * ref.D, (what, d, ref.D)
        assert not W1.any() and not H1.any(), what
    return names


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(DEGENERATE))
def test_degenerate_shapes_entry_for_entry(amd, monkeypatch, case):
    make, k, env, row_items = DEGENERATE[case]
    X = make()
    W0, H0 = R.planted_start(X.shape[0], X.shape[1], k)
    with _engine(amd, monkeypatch, env) as eng:
        names = _degenerate_check(eng, X, W0, H0, case)
        if row_items is not None:
            assert ("k_nmf_row_reduce" in names) == row_items, names
        if "PLSA_HEAVY_ITEMS" in env:                   # 700 entries in items of 8: the heavy branch of k_col_reduce
            bal = eng.balance_info()
            assert bal["item_entries"] == 8 and bal["n_items"] == 88


@pytest.mark.gpu
def test_all_stored_entries_zero(amd, monkeypatch):
    """every numerator is 0: W and H become exactly 0, the objective is sqrt(2 W_sum . H_sum) of the start"""
    X = _stored_zeros()
    W0, H0 = R.planted_start(X.shape[0], X.shape[1], 6)
    with _engine(amd, monkeypatch, {}) as eng:
        _degenerate_check(eng, X, W0, H0, "stored zeros")


@pytest.mark.gpu
def test_no_stored_entry(amd, monkeypatch):
    """an accepted empty corpus behaves like the all-zero one; a refused one leaves a usable context"""
    X = sp.csr_matrix((40, 30), dtype=np.float32)
    assert X.nnz == 0
    W0, H0 = R.planted_start(40, 30, 6)
    with _engine(amd, monkeypatch, {}) as eng:
        try:
            eng.upload_csr(X)
        except amd.DeviceError:
            accepted = False
        else:
            accepted = True
        print("a corpus without stored entries is %s" % ("accepted" if accepted else "refused"))
        if accepted:
            assert eng.shape == (40, 30, 0)
            _degenerate_check(eng, X, W0, H0, "no stored entry")
        ref = reference(6)
        W1, H1, _, _, _ = _halves(eng, ref.X, ref.W0, ref.H0)
        _held(W1, ref.Ww, ref.L_row, 6, "W half after the empty corpus")
        _held(H1, ref.h_half(W1), ref.L_col, 6, "H half after the empty corpus")
        eng.nmf_set_factors(ref.W0, ref.H0)
        _held_objective(eng.nmf_divergence(), ref.D, ref.scale, 6, "objective after the empty corpus")


# ------------------------------------------------------------------------------------------------
# 5. NMF on a reused context
# ------------------------------------------------------------------------------------------------
WALK_FIT = dict(max_iter=12, tol=1e-30)


def _walk_inputs(corpus, k):
    """(X, W0, H0) of a walk step: A = edge_corpus, A' = a seeded resample of it (280 draws), B = long_rows_corpus"""
    if corpus == "B":
        return R.long_rows_corpus(k)
    X, W0, H0 = R.edge_corpus(k)
    if corpus == "A'":
        idx = _walk_draw()
        return X[idx], np.ascontiguousarray(W0[idx]), H0
    return X, W0, H0


def _walk_draw():
    idx = np.random.RandomState(78).randint(0, 301, size=280).astype(np.int64)
    assert np.unique(idx).shape[0] < 280 and 3 in idx and 5 in idx
    return idx


def _walk_step(eng, W0, H0, star, fit):
    out = {}
    if star:
        eng.nmf_set_factors(W0, H0)
        eng.nmf_update_w()
        out["W1"] = eng.nmf_get_factors(want_h=False)[0]
        eng.nmf_update_h()
        out["H1"] = eng.nmf_get_factors(want_w=False)[1]
        eng.nmf_set_factors(W0, H0)
        out["d"] = eng.nmf_divergence()
    eng.nmf_set_factors(W0, H0)
    out["n_iter"], out["errors"] = _fit(eng, **fit)
    out["W"], out["H"] = eng.nmf_get_factors()
    out["info"] = eng.pass_info()
    return out


@pytest.mark.gpu
def test_nmf_on_a_reused_context(amd, monkeypatch):
    """One walk over ONE context; after every step the result (both half-iterations and the objective at the starred steps,
    W, H and the errors of a 12-iteration fit at all of them) equals, bit for bit, what a context created for that step
    alone returns from the same inputs.  NMF's own buffers (nmf.slabs / raw / guarded / obj) are sized by kp or a grid;
    the row items, E-step items and column structure are shared with the EM passes and invalidated by set_shape."""
    from enstop_amd.plsa import _fit_on_engine
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    fresh_cache = {}

    def fresh(corpus, k, star, fit):
        key = (corpus, k, star, tuple(sorted(fit.items())))
        if key not in fresh_cache:
            X, W0, H0 = _walk_inputs(corpus, k)
            with amd.Engine() as other:
                other.upload_csr(X)
                fresh_cache[key] = _walk_step(other, W0, H0, star, fit)
        return fresh_cache[key]

    def plsa(eng):
        _fit_on_engine(eng, 20, None, "random", 12, 5, 0.0, 1e-16, 3, None)
        return dict(zip(("U", "V"), eng.get_factors()))

    results = {}
    with amd.Engine() as eng:
        eng.timing(True)

        def step(number, corpus, k, star, fit=WALK_FIT, row_reduce=None):
            X, W0, H0 = _walk_inputs(corpus, k)
            assert eng.shape == (X.shape[0], X.shape[1], X.nnz), (number, eng.shape)
            eng.timing_reset()
            got = results[number] = _walk_step(eng, W0, H0, star, fit)
            names = set(eng.timing_report())
            kp, col, row = lane_shape(k)
            assert got["info"]["col"] == (col[0], col[1], _is_full(kp, col)), (number, got["info"])
            assert got["info"]["row"] == (row[0], row[1], _is_full(kp, row)), (number, got["info"])
            assert got["n_iter"] == fit["max_iter"] and len(got["errors"]) == 1 + fit["max_iter"] // 10, (number, got["errors"])
            if row_reduce is not None:
                assert ("k_nmf_row_reduce" in names) == row_reduce, (number, names)
            _same(fresh(corpus, k, star, fit), got, "step %d (%s, k = %d)" % (number, corpus, k))
            return got

        A = R.edge_corpus(6)[0]
        eng.upload_csr(A)
        step(1, "A", 60, True)
        assert results[1]["info"]["row"][:2] == (16, 1)
        step(2, "A", 64, True, row_reduce=False)       # document pass 16 x 1 -> 8 x 2, column pass stays 16 x 1
        assert results[2]["info"]["row"][:2] == (8, 2) and results[2]["info"]["col"] == results[1]["info"]["col"][:2] + (True,)
        step(3, "A", 6, True)                           # both shapes shrink; nmf.raw / guarded larger than needed
        step(4, "A", 700, False)                        # both grow
        eng.release_scratch()
        step(5, "A", 64, False)
        eng.bootstrap(_walk_draw())
        step(6, "A'", 64, True)
        eng.bootstrap(None)
        step(7, "A", 64, False)
        with amd.Engine() as other:                     # a pLSA fit in between: equal to a fresh context's, then NMF
            other.upload_csr(A)
            p_fresh = plsa(other)
        eng.timing(False)
        _same(p_fresh, plsa(eng), "step 8: pLSA after NMF")
        eng.timing(True)
        step(8, "A", 20, True)
        with pytest.raises(amd.DeviceError, match="1024"):      # a refused call leaves the context as it was
            eng.nmf_set_factors(np.ones((A.shape[0], 1025), np.float32), np.ones((1025, A.shape[1]), np.float32))
        step(9, "A", 20, True)
        _same(results[8], results[9], "step 9 against step 8")
        eng.upload_csr(R.long_rows_corpus(6)[0])
        step(10, "B", 6, True, row_reduce=True)         # 12 documents of 3000 entries: row items by themselves
        eng.upload_csr(A)
        step(11, "A", 6, True, row_reduce=False)        # back to whole documents
        _same(results[3], results[11], "step 11 against step 3")
        got = step(12, "A", 6, False, fit=dict(update_h=False, max_iter=25, tol=1e-30), row_reduce=False)
        assert np.array_equal(_bits(got["H"]), _bits(R.edge_corpus(6)[2]))
        assert eng.timing_get("k_nmf_row_pass")[1] == 3         # the combined pass: iterations 1-10, 11-20, 21-25
    assert [results[i]["info"]["row"][:2] for i in (1, 2, 3, 4)] == [(16, 1), (8, 2), (2, 1), (64, 4)]
