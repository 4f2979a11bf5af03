"""Every instantiation of the EM passes against a float64 restatement of one EM step, entry for entry.

The hot path is a family of template instantiations (csrc/plsa_kernels.hpp): lane shape (LPN, CH), FULL or run-time kp,
WIDE (64-bit gather addresses) or narrow, Packed<S> or the two index arrays, TINY (the denormal-norm rescue) or not, with or
without the log-likelihood, with or without row items, fused or from P.  Whole fits compare them with the oracle to 1e-4 of
the largest entry, which cannot see a wrong small entry.  Here one EM step from fixed factors is compared ELEMENTWISE with
`step64` below, a vectorised float64 restatement of enstop/plsa.py:91-105 (E-step), 172-202 / 277-310 (M-step without /
with sample weights) and 372-386 (log-likelihood).  The products P(w|z) P(z|d) are formed in float32, as the reference forms
them, so that every threshold decision is the reference's own; everything after that is float64.

Error model (u = 2^-24).  Every sum of the step adds non-negative terms, so a float32 sum of L terms in any order is within
(L - 1) u of the exact sum, relative to it, entry by entry.  An updated P(z|d) entry is num / den: num sums L terms x * v / N
(N: a responsibility norm of k products, one reciprocal of at most 1 ulp, two products), den sums its row's k nums, one
correctly rounded division: (L + k + 2) u + (L + 2k + 1) u + u <= 4 (L + k) u.  P(w|z) likewise, L the longest column,
norm_pwz is accumulated in float64 from float32 partials of at most L terms: <= 4 (L + k) u.  A log-likelihood term
x * log(dot) * sw has dot a float32 sum of k products and two roundings after logf: its error is at most
(k + 4 |log dot|) u x sw <= 4 (k + 1) u x sw max(1, |log dot|); the terms are added in float64.  So

    factors, norms, P(z|w,d):  |got - want| <= 4 (L + k) 2^-24 |want|, want == 0 exactly where want is 0
    log-likelihood:             |got - want| <= 4 (k + 1) 2^-24 sum x sw max(1, |log dot|)

with L the longest row (P(z|d), norm_pdz), the longest column (P(w|z), norm_pwz), at least 2.  The constant comes from the
model; the worst observed fraction of the bound is printed per topic count.

PLSA_FORCE_WIDE and PLSA_PACKED=0 run the same arithmetic as the default and must give the same bits.  Which instantiations
ran is read back, not assumed: lane shapes and gather widths from Engine.pass_info(), the index streams from packed_info(),
the kernel variants from the timing names.  test_gather_width_and_packed_id_edges takes the 32-bit gather offsets and the
24-bit packed ids to the edges of their ranges (about 20 GB of HBM, sparse corpora).

Needs a real MI355X for everything except the CPU pin of the restatement (test_step64_reproduces_the_reference_fixtures)
and the reach of K_MATRIX.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_golden, golden_csr

U32 = 2.0 ** -24
C_FACTOR = 4.0          # the constant of the error model above
TINY_THRESH = 5e-38     # csrc/plsa_kernels.hpp: TINY_THRESH -- thresholds below it compile the rescue in

# Topic counts of the matrix: every default lane shape in its FULL and its partial form where one exists ((1,1) and (2,1)
# are always FULL), padding topics (k % 4 != 0) and the 8 x 2 document pass (kp = 64).
K_MATRIX = [3, 4, 6, 9, 16, 21, 32, 47, 62, 64, 100, 128, 130, 255, 300, 512, 700, 1021, 1024]
DEFAULT_SHAPES = [(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (16, 2), (32, 2), (64, 2), (64, 4)]


# ------------------------------------------------------------------------------------------------
# float64 restatement of one EM step
# ------------------------------------------------------------------------------------------------
def _coo(X):
    X = X.tocsr()
    rows = np.repeat(np.arange(X.shape[0], dtype=np.int64), np.diff(X.indptr))
    return rows, X.indices.astype(np.int64), X.data.astype(np.float32)


def products32(rows, cols, U, V):
    """v[j, z] = P(w|z)[z, w_j] * P(z|d)[d_j, z] as one float32 product (plsa.py:97)"""
    return np.asarray(V, np.float32)[:, cols].T * np.asarray(U, np.float32)[rows]


def _segment_sum(ids, vals, count):
    """float64 sums of the rows of vals [nnz, k] grouped by ids -> [count, k]"""
    S = sp.csr_matrix((np.ones(ids.shape[0]), (ids, np.arange(ids.shape[0]))), shape=(count, ids.shape[0]))
    return np.asarray(S @ vals)


def e_step64(rows, cols, U, V, thresh):
    """plsa.py:91-105: responsibilities P(z|w,d) [nnz, k], float64 after the float32 product and threshold"""
    v = products32(rows, cols, U, V)
    keep = np.where(v > np.float32(thresh), v, np.float32(0)).astype(np.float64)
    norm = keep.sum(1, keepdims=True)
    return np.divide(keep, norm, out=np.zeros_like(keep), where=norm > 0)


def m_step64(rows, cols, x, P, n, m, sw=None):
    """plsa.py:172-202 (sw None) / 277-310: returns P(z|d) [n, k], P(w|z) [k, m], norm_pwz [k], norm_pdz [n]"""
    s = np.asarray(x, np.float64)[:, None] * P
    A = _segment_sum(rows, s, n)
    norm_pdz = A.sum(1)
    t = s if sw is None else s * np.asarray(sw, np.float64)[rows][:, None]
    B = _segment_sum(cols, t, m)
    norm_pwz = B.sum(0)
    U1 = np.divide(A, norm_pdz[:, None], out=np.zeros_like(A), where=norm_pdz[:, None] > 0)
    V1 = np.divide(B, norm_pwz[None, :], out=np.zeros_like(B), where=norm_pwz[None, :] > 0).T
    return U1, np.ascontiguousarray(V1), norm_pwz, norm_pdz


def loglik64(rows, cols, x, U, V, sw=None):
    """plsa.py:372-386: sum x log(sum_z P(w|z) P(z|d)) sw[d]; also the scale of its error bound, sum x sw max(1, |log dot|)"""
    dot = products32(rows, cols, U, V).astype(np.float64).sum(1)
    w = np.asarray(x, np.float64) * (1.0 if sw is None else np.asarray(sw, np.float64)[rows])
    with np.errstate(divide="ignore", invalid="ignore"):
        lg = np.log(dot)
        ll = float((w * lg).sum())
        scale = float((np.abs(w) * np.maximum(1.0, np.abs(lg))).sum())
    return ll, scale


def step64(X, U, V, thresh, sw=None):
    """One EM step of the reference from (U, V) on X, in float64 after the float32 products."""
    rows, cols, x = _coo(X)
    n, m = X.shape
    P = e_step64(rows, cols, U, V, thresh)
    U1, V1, npwz, npdz = m_step64(rows, cols, x, P, n, m, sw)
    ll, ll_scale = loglik64(rows, cols, x, U, V, sw)
    X = X.tocsr()
    Xc = X.tocsc()
    return dict(P=P, U=U1, V=V1, norm_pwz=npwz, norm_pdz=npdz, ll=ll, ll_scale=ll_scale,
                L_row=max(2, int(np.diff(X.indptr).max(initial=0))), L_col=max(2, int(np.diff(Xc.indptr).max(initial=0))))


def rel_excess(got, want, bound):
    """largest |got - want| / (bound |want|) over the non-zero entries of want; zeros of want must be exact zeros of got"""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), "non-finite entries: %d" % (~np.isfinite(got)).sum()
    zero = want == 0
    assert (got[zero] == 0).all(), "%d entries should be exactly 0, largest %.3e" % ((got[zero] != 0).sum(), np.abs(got[zero]).max())
    if zero.all():
        return 0.0
    return float((np.abs(got - want)[~zero] / (bound * np.abs(want[~zero]))).max())


def check(name, got, want, bound, ratios=None):
    r = rel_excess(got, want, bound)
    assert r <= 1.0, "%s: error %.3g x its bound %.3g (relative)" % (name, r, bound)
    if ratios is not None:
        ratios[name] = max(ratios.get(name, 0.0), r)
    return r


def check_ll(name, got, want, scale, k, ratios=None):
    bound = C_FACTOR * (k + 1) * U32 * scale
    err = abs(float(got) - want)
    assert err <= bound, "%s: log-likelihood %r vs %r (error %.3g, bound %.3g)" % (name, got, want, err, bound)
    if ratios is not None:
        ratios[name] = max(ratios.get(name, 0.0), err / bound)


def lane_shape(k, chunks_per_lane=2):
    """(kp, column-pass (lpn, ch), document-pass (lpn, ch)): csrc/plsa_hip.hip set_shape restated"""
    kp = (k + 3) // 4 * 4
    lpn = 1
    while lpn < kp // 4 and lpn < 64:
        lpn *= 2
    if lpn >= 32 and lpn * 4 >= kp and chunks_per_lane == 2:
        lpn //= 2
    ch = (kp // 4 + lpn - 1) // lpn
    if ch == 3:
        ch = 4
    row = (8, 2) if (lpn, ch) == (16, 1) and kp == 64 else (lpn, ch)
    return kp, (lpn, ch), row


# ------------------------------------------------------------------------------------------------
# CPU: the restatement against the reference's own outputs, and the reach of K_MATRIX
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["kernels_k6", "kernels_k8_thresh", "kernels_k20", "kernels_k33"])
def test_step64_reproduces_the_reference_fixtures(case):
    """The checker checked: the reference (float32 arithmetic, golden fixtures) stays within the rounding of ITS sums of
    e_step64 / m_step64 / loglik64.  Its own summation lengths set the bounds: P(z|w,d) a norm of k terms; P(z|d) L_row
    terms over norm_pdz, a running sum of L_row k terms; P(w|z) L_col terms over norm_pwz, a running sum of nnz terms; the
    log-likelihood one float32 sum of nnz terms."""
    g = load_golden(case)
    X = golden_csr(g)
    rows, cols, x = _coo(X)
    n, m = X.shape
    k = int(g["k"])
    nnz = x.shape[0]
    L_row = int(np.diff(X.tocsr().indptr).max())
    L_col = int(np.diff(X.tocsc().indptr).max())

    P = e_step64(rows, cols, g["U"], g["V"], g["thresh"])
    np.testing.assert_array_equal(P == 0, g["P"] == 0)                      # the reference's threshold decisions
    check("P", g["P"], P, 2 * (k + 1) * U32)

    # the M-steps from the reference's own P(z|w,d)
    for sw, key in ((None, ""), (g["sw"], "w")):
        U1, V1, npwz, npdz = m_step64(rows, cols, x, g["P"].astype(np.float64), n, m, sw)
        sfx = "_" + key if key else ""
        check("U_m" + key, g["U_m" + key], U1, 2 * (L_row * (k + 1) + 4) * U32)
        check("V_m" + key, g["V_m" + key], V1, 2 * (L_col + nnz + 4) * U32)
        check("norm_pwz" + sfx, g["norm_pwz" + sfx], npwz, 2 * (nnz + 2) * U32)
        check("norm_pdz" + sfx, g["norm_pdz" + sfx], npdz, 2 * (L_row * k + 2) * U32)

    # the log-likelihoods (the reference: float32 dot, float32 running sum over nnz)
    ones = np.ones(n, np.float32)
    for sw, key, U, V in ((ones, "ll_ones", g["U"], g["V"]), (g["sw"], "ll_sw", g["U"], g["V"]),
                          (ones, "ll_after_m", g["U_m"], g["V_m"])):
        want, scale = loglik64(rows, cols, x, U, V, sw)
        got = float(g[key])
        if not np.isfinite(want):
            assert got == want, (key, got, want)
            continue
        err = abs(got - want)
        assert err <= 2 * U32 * (k * scale + (nnz + 4) * abs(want)), (key, got, want)


def test_step64_rejects_a_wrong_step():
    """the pin is not vacuous: a one-ulp-scale change of the inputs, a swapped topic or a dropped entry breaks it"""
    g = load_golden("kernels_k20")
    X = golden_csr(g)
    rows, cols, x = _coo(X)
    n, m = X.shape
    k = int(g["k"])
    L_row = int(np.diff(X.tocsr().indptr).max())
    bound = 2 * (L_row * (k + 1) + 4) * U32
    U1, _, _, _ = m_step64(rows, cols, x, g["P"].astype(np.float64), n, m)
    Pw = g["P"].astype(np.float64).copy()
    Pw[:, [0, 1]] = Pw[:, [1, 0]]
    U2, _, _, _ = m_step64(rows, cols, x, Pw, n, m)
    with pytest.raises(AssertionError):
        check("swapped", g["U_m"], U2, bound)
    x2 = x.copy()
    x2[5] = 0
    U3, _, _, _ = m_step64(rows, cols, x2, g["P"].astype(np.float64), n, m)
    with pytest.raises(AssertionError):
        check("dropped", g["U_m"], U3, bound)
    check("same", g["U_m"], U1, bound)


def test_matrix_topic_counts_reach_every_default_instantiation():
    """K_MATRIX covers every (lane shape, FULL) pair that set_shape produces for 1 <= k <= 1024, for both passes, with and
    without padding topics; the default shapes are the nine that DESIGN.md names."""
    reach_col, reach_row = set(), set()
    for k in range(1, 1025):
        kp, col, row = lane_shape(k)
        reach_col.add((col, kp == 4 * col[0] * col[1]))
        reach_row.add((row, kp == 4 * row[0] * row[1]))
    cover_col, cover_row, padded = set(), set(), set()
    for k in K_MATRIX:
        kp, col, row = lane_shape(k)
        cover_col.add((col, kp == 4 * col[0] * col[1]))
        cover_row.add((row, kp == 4 * row[0] * row[1]))
        if kp != k:
            padded.add(col)
    assert sorted({s for s, _ in reach_col}) == sorted(DEFAULT_SHAPES)
    assert reach_col == cover_col and reach_row == cover_row
    assert ((8, 2), True) in cover_row
    assert padded == {(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 2), (64, 4)}


# ------------------------------------------------------------------------------------------------
# GPU: the instantiation matrix
# ------------------------------------------------------------------------------------------------
EMPTY_DOCS = (7, 501)
LONG_DOC, HEAVY_WORD = 3, 5
TINY_DOCS, N_TINY_WORDS = (11, 12, 13, 14), 4


def matrix_corpus(k, n=640, m=480):
    """One seeded corpus per k: ~4 000 non-zeros, two empty documents, a 300-word document (row items), a word in every
    non-empty document (heavy columns), stored zeros, a few escaped counts (256, 300, 2.5; fewer than 1/16 of the entries,
    the packed streams stay eligible), and a block of documents x words whose products P(w|z) P(z|d) lie in
    [2^-140, 2^-139]: their responsibility norms are subnormal (thresh 0: the TINY rescue; 1e-32: all thresholded away)."""
    rs = np.random.RandomState(1000 + k)
    mask = rs.rand(n, m) < 0.011
    mask[LONG_DOC, rs.choice(m, 300, replace=False)] = True
    mask[:, HEAVY_WORD] = True
    tiny_words = np.arange(m - N_TINY_WORDS, m)
    mask[np.ix_(TINY_DOCS, tiny_words)] = True
    mask[list(EMPTY_DOCS), :] = False
    r, c = np.nonzero(mask)
    x = rs.randint(1, 8, size=r.shape[0]).astype(np.float32)
    pick = rs.choice(r.shape[0], 60, replace=False)
    x[pick[:40]] = 0.0                                            # stored zeros
    x[pick[40:]] = np.resize(np.array([256, 300, 2.5, 4000, 0.75], np.float32), 20)
    X = sp.csr_matrix((x, (r, c)), shape=(n, m))
    assert X.nnz == r.shape[0] and (X.data == 0).sum() == 40
    U = (rs.rand(n, k) + 0.05).astype(np.float64)
    U /= U.sum(1, keepdims=True)
    V = (rs.rand(k, m) + 0.05).astype(np.float64)
    V /= V.sum(1, keepdims=True)
    U, V = U.astype(np.float32), V.astype(np.float32)
    U[list(TINY_DOCS)] = (2.0 ** -69 * (0.7 + 0.3 * rs.rand(len(TINY_DOCS), k))).astype(np.float32)
    V[:, tiny_words] = (2.0 ** -70 * (0.7 + 0.3 * rs.rand(k, N_TINY_WORDS))).astype(np.float32)
    sw = (0.5 + rs.rand(n)).astype(np.float32)
    return X, U, V, sw


def _tiny_block_is_subnormal(X, U, V):
    rows, cols, _ = _coo(X)
    v = products32(rows, cols, U, V)
    tiny = np.isin(rows, TINY_DOCS) & (cols >= X.shape[1] - N_TINY_WORDS)
    assert tiny.sum() == len(TINY_DOCS) * N_TINY_WORDS
    assert (v[tiny] >= 2.0 ** -140.1).all() and (v[tiny] <= 2.0 ** -139).all()
    assert (v[tiny].astype(np.float64).sum(1) < 2.0 ** -128).all()          # 1 / norm overflows without the rescue
    assert (v[~tiny].astype(np.float64).sum(1) > 2.0 ** -100).all()         # the rest never needs it


# settings of a context (PLSA_* knobs are read when it is created).  The first four run the same arithmetic: their
# results must be bit-identical.  ROW_ITEMS and HEAVY cut the sums differently and are held to the float64 step.
SETTINGS = {
    "default": {},
    "wide": {"PLSA_FORCE_WIDE": "1"},
    "arrays": {"PLSA_PACKED": "0"},
    "wide_arrays": {"PLSA_FORCE_WIDE": "1", "PLSA_PACKED": "0"},
    "row_items": {"PLSA_ROW_ITEMS": "1", "PLSA_ROW_SEG": "16"},
    "heavy": {"PLSA_HEAVY_ITEMS": "2", "PLSA_COL_SEG": "8"},
    "e_rows": {"PLSA_E_ROWS": "1"},          # the document-owned E-step traversal (chosen by size from 1e8 cells on)
}
KNOBS = sorted({key for env in SETTINGS.values() for key in env})
SAME_ARITHMETIC = ("default", "wide", "arrays", "wide_arrays")
# (path, want_ll, weighted, thresh): every (LL, TINY) pair of the fused passes with and without weights; the materialised
# schedule and the kernel-level entry points with both thresholds
RUNS = [("fused", True, False, 1e-32), ("fused", False, True, 1e-32), ("fused", True, True, 0.0), ("fused", False, False, 0.0),
        ("materialised", True, True, 1e-32), ("materialised", False, False, 0.0),
        ("kernels", True, True, 0.0), ("kernels", True, False, 1e-32)]
FUSED_ONLY = ("wide_arrays", "row_items", "heavy")
MATERIALISED_ONLY = ("e_rows",)


def _run(eng, path, want_ll, sw, thresh, U0, V0, k):
    eng.set_factors(U0, V0)
    eng.timing_reset()
    out = {}
    if path == "kernels":
        out["ll"] = eng.log_likelihood(sw) if want_ll else None
        out["P"] = eng.e_step(thresh)
        out["norm_pwz"], out["norm_pdz"] = eng.m_step(sw)
    else:
        out["ll"] = eng.em_accumulate(sw, thresh, want_ll=want_ll, materialised=(path == "materialised"))
        _, m, _ = eng.shape
        out["acc"] = eng.accumulator_get().reshape(m, -1)        # un-normalised P(w|z) with the padding topics
        eng.em_finish()
    out["U"], out["V"] = eng.get_factors()
    out["names"] = set(eng.timing_report())
    out["pass"] = eng.pass_info()
    out["packed"] = eng.packed_info()
    return out


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b, what):
    for key in ("U", "V", "P", "acc", "norm_pwz", "norm_pdz"):
        if key in a:
            np.testing.assert_array_equal(_bits(a[key]), _bits(b[key]), err_msg="%s: %s" % (what, key))
    if a["ll"] is not None:
        assert np.float64(a["ll"]).view(np.uint64) == np.float64(b["ll"]).view(np.uint64), (what, a["ll"], b["ll"])


@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


@pytest.fixture(scope="module")
def worst():
    out = {}
    yield out
    if out:
        print("\npass matrix: worst error / bound per quantity: " +
              ", ".join("%s %.3g" % (key, v) for key, v in sorted(out.items())))


@pytest.mark.gpu
@pytest.mark.parametrize("k", K_MATRIX)
def test_instantiation_matrix(amd, monkeypatch, worst, k):
    X, U0, V0, sw_doc = matrix_corpus(k)
    _tiny_block_is_subnormal(X, U0, V0)
    n, m = X.shape
    kp, col_shape, row_shape = lane_shape(k)
    want = {}
    for weighted in (False, True):
        for thresh in (1e-32, 0.0):
            want[weighted, thresh] = step64(X, U0, V0, thresh, sw_doc if weighted else None)
    L_row, L_col = want[False, 0.0]["L_row"], want[False, 0.0]["L_col"]
    b_row, b_col = C_FACTOR * (L_row + k) * U32, C_FACTOR * (L_col + k) * U32
    ratios = {}
    results = {}
    seen_row, seen_col = set(), set()
    for name, env in SETTINGS.items():
        for key in KNOBS:
            monkeypatch.delenv(key, raising=False)
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with amd.Engine() as eng:
            eng.upload_csr(X)
            eng.timing(True)
            for path, want_ll, weighted, thresh in RUNS:
                if (name in FUSED_ONLY and path != "fused") or (name in MATERIALISED_ONLY and path == "fused"):
                    continue
                sw = sw_doc if weighted else None
                got = _run(eng, path, want_ll, sw, thresh, U0, V0, k)
                results[name, path, want_ll, weighted, thresh] = got
                ref = want[weighted, thresh]
                tag = "k=%d %s %s ll=%d sw=%d thresh=%g" % (k, name, path, want_ll, weighted, thresh)
                # -- the step, entry for entry
                check("U " + tag, got["U"], ref["U"], b_row, ratios)
                check("V " + tag, got["V"], ref["V"], b_col, ratios)
                if want_ll:
                    check_ll("LL " + tag, got["ll"], ref["ll"], ref["ll_scale"], k, ratios)
                if path == "kernels":
                    check("P " + tag, got["P"], ref["P"], C_FACTOR * (2 + k) * U32, ratios)
                    check("norm_pwz " + tag, got["norm_pwz"], ref["norm_pwz"], b_col, ratios)
                    check("norm_pdz " + tag, got["norm_pdz"], ref["norm_pdz"], b_row, ratios)
                else:   # the accumulator: P(w|z) before the division, padding topics exactly 0
                    acc = got["acc"]
                    assert acc.shape == (m, kp)
                    assert not acc[:, k:].any(), tag
                    check("acc " + tag, acc[:, :k].T, ref["V"] * ref["norm_pwz"][:, None], b_col, ratios)
                for d in EMPTY_DOCS:
                    assert not got["U"][d].any(), tag
                # -- which instantiations ran
                info, pk = got["pass"], got["packed"]
                assert info["col"] == (col_shape[0], col_shape[1], kp == 4 * col_shape[0] * col_shape[1]), (tag, info)
                assert info["row"] == (row_shape[0], row_shape[1], kp == 4 * row_shape[0] * row_shape[1]), (tag, info)
                wide_knob = env.get("PLSA_FORCE_WIDE") == "1"
                assert info["row_wide"] == wide_knob and info["col_wide"] == wide_knob, (tag, info)
                packed = env.get("PLSA_PACKED") != "0"
                names = got["names"]
                tiny = thresh < TINY_THRESH
                if path == "fused":
                    assert pk == (dict(csr="packed", csc="packed") if packed else dict(csr="arrays", csc="arrays")), (tag, pk)
                    assert ("k_row_pass<fused,LL>" if want_ll else "k_row_pass<fused>") in names, (tag, names)
                    assert {"k_col_pass<fused>", "k_col_reduce"} <= names, (tag, names)
                    assert ("k_row_reduce" in names) == (name == "row_items"), (tag, names)
                    seen_row.add((info["row"][:2], info["row"][2] and not info["row_wide"], info["row_wide"], packed, tiny, want_ll))
                    seen_col.add((info["col"][:2], info["col"][2] and not info["col_wide"], info["col_wide"], packed, tiny))
                else:
                    assert {"k_e_step", "k_row_pass<P>", "k_col_pass<P>"} <= names, (tag, names)
                    assert ("k_loglik" in names) == want_ll, (tag, names)
            if name == "heavy":
                bal = eng.balance_info()
                lens = np.diff(X.tocsc().indptr)
                assert bal["item_entries"] == 8
                assert ((lens + 7) // 8 > 2).sum() >= 1           # columns that take the heavy (one block per column) path
    # -- the same arithmetic, bit for bit
    for key, got in results.items():
        if key[0] in SAME_ARITHMETIC and key[0] != "default":
            _same_bits(results[("default",) + key[1:]], got, "k=%d %s vs default" % (k, key))
    # -- every (shape, FULL, WIDE, Packed, TINY, LL) combination of the fused passes that k reaches
    row_full = kp == 4 * row_shape[0] * row_shape[1]
    col_full = kp == 4 * col_shape[0] * col_shape[1]
    flags = [(w, p, t) for w in (False, True) for p in (False, True) for t in (False, True)]
    assert seen_row == {(row_shape, row_full and not w, w, p, t, ll) for w, p, t in flags for ll in (False, True)}
    assert seen_col == {(col_shape, col_full and not w, w, p, t) for w, p, t in flags}
    for key, v in ratios.items():
        q = key.split(" ")[0]
        worst[q] = max(worst.get(q, 0.0), v)
    print("\nk=%d rows %s cols %s: worst error / bound %.3g (%s)" % (
        k, row_shape, col_shape, max(ratios.values()), max(ratios, key=ratios.get)))


# ------------------------------------------------------------------------------------------------
# gather widths and packed-id limits at their boundaries
# ------------------------------------------------------------------------------------------------
# The fused passes gather factor rows by index with a 32-bit unsigned BYTE offset below 4 GB and with 64-bit row
# addresses from 4 GB on (csrc/plsa_hip.hip: table_is_wide); their packed streams hold ids below 2^24
# (csrc/plsa_kernels.hpp: PACK_MAX_IDS).  side "row": the document pass gathers P(w|z), `rows` = m words; side "col": the
# column pass gathers P(z|d), `rows` = n documents (almost all empty).  The touched ids sit at the bottom of the range,
# around byte offset 2^31 (the sign bit of the offset) and at the very top; the step is compared with the float64
# step of the same corpus restricted to them, untouched rows / columns must stay exactly 0, and a narrow table must give
# the same bits under PLSA_FORCE_WIDE=1.  Host factors are np.zeros with the touched rows filled in (two 4 GB arrays at most).
GATHER_EDGES = [("row", 64, (1 << 23) + 16),                       # offsets across 2^31 first, the sign bit of the offset
                ("row", 64, (1 << 24) - 1), ("row", 64, 1 << 24), ("row", 64, (1 << 24) + 1),
                ("col", 64, (1 << 24) - 1), ("col", 64, 1 << 24), ("col", 64, (1 << 24) + 1),
                ("row", 1024, (1 << 20) - 1), ("row", 1024, 1 << 20), ("col", 1024, (1 << 20) - 1), ("col", 1024, 1 << 20)]


def _edge_corpus(side, k, rows, seed=5):
    rs = np.random.RandomState(seed)
    kp = (k + 3) // 4 * 4
    sign = (1 << 31) // (4 * kp)                                  # the row at byte offset 2^31
    edges = np.unique([i for i in (0, 1, 2, 3, sign - 2, sign - 1, sign, sign + 1, rows - 4, rows - 3, rows - 2, rows - 1)
                       if 0 <= i < rows])
    if side == "row":                                             # 3 000 documents over the edge words + a few random ones
        n, m = 3000, rows
        lengths = rs.randint(3, 7, size=n)
        r = np.repeat(np.arange(n), lengths)
        c = np.where(rs.rand(r.shape[0]) < 0.8, rs.choice(edges, r.shape[0]), rs.randint(0, rows, r.shape[0]))
    else:                                                         # the edge documents + 200 random ones, 2 000 words
        n, m = rows, 2000
        docs = np.unique(np.concatenate([edges, rs.randint(0, rows, 200)]))
        r = np.repeat(docs, 30)
        c = rs.randint(0, m, r.shape[0])
    X = sp.csr_matrix((rs.randint(1, 8, r.shape[0]).astype(np.float32), (r, c)), shape=(n, m))
    X.sum_duplicates()
    Xc = X.tocsc() if side == "row" else X
    touched = np.flatnonzero(np.diff(Xc.indptr))
    assert set(edges) <= set(touched)
    return X, touched


def _edge_factors(side, X, touched, k, seed=6):
    rs = np.random.RandomState(seed)
    n, m = X.shape
    if side == "row":
        U = (rs.rand(n, k) + 0.05).astype(np.float32)
        U /= U.sum(1, keepdims=True)
        V = np.zeros((k, m), np.float32)
        V[:, touched] = (rs.rand(k, touched.shape[0]) + 0.05) / m
    else:
        U = np.zeros((n, k), np.float32)
        t = rs.rand(touched.shape[0], k) + 0.05
        U[touched] = t / t.sum(1, keepdims=True)
        V = (rs.rand(k, m) + 0.05).astype(np.float32)
        V /= V.sum(1, keepdims=True)
    return U, V


def _edge_step(amd, side, X, touched, U0, V0):
    """one fused EM step; returns the touched part of the gathered factor (the rest checked to be 0 and dropped)"""
    with amd.Engine() as eng:
        eng.upload_csr(X)
        eng.set_factors(U0, V0)
        info = eng.pass_info()
        ll = eng.em_accumulate(None, 1e-32, want_ll=True)
        eng.em_finish()
        pk = eng.packed_info()
        U, V = eng.get_factors()
    if side == "row":
        part = V[:, touched].copy()
        V[:, touched] = 0
        assert not V.any(), "untouched P(w|z) columns are not 0"
        del V
        return dict(info=info, packed=pk, ll=ll, U=U, V=part)
    part = U[touched].copy()
    U[touched] = 0
    assert not U.any(), "P(z|d) rows of empty documents are not 0"
    del U
    return dict(info=info, packed=pk, ll=ll, U=part, V=V)


@pytest.mark.gpu
@pytest.mark.parametrize("side, k, rows", GATHER_EDGES)
def test_gather_width_and_packed_id_edges(amd, monkeypatch, side, k, rows):
    from enstop_amd.engine import reset_engines
    reset_engines()                                   # engines cached by other modules may hold most of the HBM
    kp = (k + 3) // 4 * 4
    wide = rows * kp * 4 >= 1 << 32
    packed = rows <= 1 << 24
    X, touched = _edge_corpus(side, k, rows)
    U0, V0 = _edge_factors(side, X, touched, k)
    # the float64 step of the corpus restricted to the touched rows / columns (the others add exact zeros)
    if side == "row":
        want = step64(X[:, touched], U0, V0[:, touched], 1e-32)
    else:
        want = step64(X[touched], U0[touched], V0, 1e-32)
    monkeypatch.delenv("PLSA_FORCE_WIDE", raising=False)
    monkeypatch.delenv("PLSA_PACKED", raising=False)
    got = _edge_step(amd, side, X, touched, U0, V0)
    gathered, other = ("row_wide", "col_wide") if side == "row" else ("col_wide", "row_wide")
    stream, other_stream = ("csr", "csc") if side == "row" else ("csc", "csr")
    assert got["info"][gathered] == wide and not got["info"][other], got["info"]
    assert got["packed"][stream] == ("packed" if packed else "arrays") and got["packed"][other_stream] == "packed", got["packed"]
    check("U", got["U"], want["U"], C_FACTOR * (want["L_row"] + k) * U32)
    check("V", got["V"], want["V"], C_FACTOR * (want["L_col"] + k) * U32)
    check_ll("LL", got["ll"], want["ll"], want["ll_scale"], k)
    if not wide:                                      # the 64-bit form of the same gathers: the same bits
        monkeypatch.setenv("PLSA_FORCE_WIDE", "1")
        w = _edge_step(amd, side, X, touched, U0, V0)
        assert w["info"][gathered] and w["info"][other]
        for key in ("U", "V"):
            np.testing.assert_array_equal(w[key].view(np.uint32), got[key].view(np.uint32), err_msg=key)
        assert np.float64(w["ll"]).view(np.uint64) == np.float64(got["ll"]).view(np.uint64)
