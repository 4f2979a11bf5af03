"""The topic-combination kernels against float64 restatements of the reference, entry for entry.

After the bootstrapped fits everything EnsembleTopics returns goes through three kernel families of
csrc/plsa_combine_kernels.hpp: k_hell_prepare / k_hell_gram / k_hell_finish (plsa_all_pairs_hellinger), k_kl_gram / k_sum_slices
(plsa_all_pairs_kl) and k_rep_accumulate / k_rep_normalise (plsa_cluster_representatives).  Here each is compared ELEMENTWISE
with a float64 restatement written below (float64 GEMMs; none of them calls enstop_amd.ensemble's host functions):

    hellinger64        umap.distances.hellinger (umap-learn >= 0.3.8) applied pairwise as enstop_.py:258-266 does, zero-mass
                       conventions included.  NO reference run of this matrix exists (umap is not installable where the
                       goldens are made): it is pinned to the published definition, statement by statement
                       (test_hellinger64_is_the_published_definition).
    kl64               enstop_.py:234-253, pinned to the reference's own run (combine_t24.npz: kl_f64_input, kl_f32_input).
    representatives64  enstop_.py:299-308, 340-345, 385-393, pinned to the reference's rep_kl / rep_hellinger / rep_umap.

Error model (u = 2^-24; constants read from the kernels, these are the only tolerances of the GPU tests).

Hellinger.  k_hell_prepare replaces p by sqrtf(p) (correctly rounded: relative error <= u) and sums p in float64 (exact to
m 2^-53).  k_hell_gram forms float32 products of two roots (<= 3 u each with the roots' errors) and adds them in float32 for at
most 256 words (`since_flush`), then in float64; slices are added in float64.  Zero products add exactly, so with W_ij the
largest number of non-zero products of the pair inside one flush window, |g - g64| <= (W_ij + 2) u g64 to first order;
C_HELL = 3 absorbs the second order and the float64 sums.  W_ij is bounded here by min(256, common support of i and j),
which needs no knowledge of the slicing.  A product of two roots below 2^-63 is subnormal or underflows: its error is
absolute, at most 2^-149 per product.  The kernel returns D = sqrt(max(1 - x, 0)), x = g / sqrt(l_i l_j); the assertion is on
x recovered as 1 - D^2 (8 * 2^-53 for the float64 roundings of that round trip):

    |(1 - D^2) - x64| <= ((W_ij + 3) u + 2 m 2^-53) x64 + common_ij 2^-149 / sqrt(l_i l_j) + 8 * 2^-53

D itself is asserted only through x: sqrt(1 - x) amplifies near x = 1, so two IDENTICAL topics in different rows may come
back with D up to sqrt((W + 3) u) ~ 4e-3 instead of 0 (the diagonal is exactly 0 by construction, not by arithmetic).
Exact: D == D^T bit for bit, zero diagonal, 0 / 1 for pairs with two / one zero-mass rows, 1 for disjoint supports.

KL.  k_kl_gram stages p_i, log2 p_i, log2 p_j and [p_j > 0], forms (p_i [p_j > 0]) * (log2 p_i - log2 p_j) in float32 and adds
like k_hell_gram.  v_log_f32 is documented to 1 ulp (2 u); below 2^-126 the argument is scaled by 2^32 and 32 is
subtracted, one more rounding: <= 3 u |log2 p| per logarithm.  The subtraction and the product round once each: a term is
within 5 u p_i (|log2 p_i| + |log2 p_j|).  Terms have both signs, so the sum's error is relative to the sum of magnitudes:

    |D - D64| <= (W_ij + 6) u S_ij + common_ij 2^-149,     S_ij = sum_w p_i (|log2 p_i| + |log2 p_j|) over the common support

(C_KL = 6: 5 plus second order; the absolute term is the subnormal rounding of a product with p_i < 2^-126.)  Exact:
D[i, i] == 0, D[i, j] == 0 for disjoint supports and for identical rows.  The float64 side takes exact logarithms of the
float32 inputs.

Representatives.  k_rep_accumulate adds w_i * sqrtf(p_i) in float64 (<= u per root), squares, k_rep_normalise divides by the
float64 row total and rounds once to float32: mean u, square 2 u, total 2 u, rounding u -> C_REP = 6 with the float64 dust,

    |rep - rep64| <= 6 u rep64 + 2^-149        (the absolute term: a float32 result below 2^-126 is subnormal)

and zeros of the restatement are exact zeros of the output.

Observed on an MI355X, 256 CUs (worst error / bound, printed per case and at the end of the module): boundary spikes
Hellinger 0.71, KL 0.21, representatives 0.45 (two to sixteen non-zero products per pair: the worst case is nearly met);
dense families at t = 640 / 1280, m = 173 762 Hellinger 0.0027 / 0.0028, KL 0.00029 / 0.00031, representatives 0.33 / 0.28;
subnormal entries KL 0.0063, Hellinger 0.0063, representatives 0.31; degenerate rows 0.007 / 0.002 / 0.47; t * m > 2^31
0.038 / 0.013 / 0.24, > 2^32 0.073 / 0.018 / 0.24.  Before k_kl_gram scaled its subnormal arguments the four subnormal
cases came back with 1300 / 1300 / 2400 / 22 499 non-finite divergences (a bare v_log_f32 returns -inf below 2^-126).

Mutations of the kernels, each run once against this file (MI355X): upper-triangular tile list started at j = i + 1 --
15 of 22 cases red; [p_j > 0] mask removed from k_kl_gram -- 14 red; la - lb swapped -- 19 red; k_rep_accumulate ignoring
w -- 18 red; k_rep_normalise summing n_blocks - 1 partials -- 22 red; `since_flush >= 65536` -- red only in the t = 1280
families, and there through the leaf labels (two families swap their numbers), not through the W_ij term: the bound is worst
case and dense rows sit at 0.003 of it.  GREEN, both for the same reason: the staging guard `ww < w1` replaced by `ww < m`,
and `slice` not rounded to a multiple of HELL_KSTEP.  Each of the two makes the other redundant (with whole staging steps
per slice a step never crosses w1 except at m; with the guard a ragged slice is cut correctly), so either alone is the same
program; both together let the slices overlap and 17 cases are red.  Dropping `bj + r < t` from the staging was not run: the
rows it would stage feed only outputs j >= t, which the store guard discards, so its one effect is a read past the buffer.

Inputs: boundary spikes at every reachable branch of the host's slicing (restated in host_slicing, the branch asserted),
production shapes t = 640 and 1280 over m = 173 762 in 20 families of near-duplicates (the HDBSCAN* leaf labels from the device
matrix equal those from the float64 matrix), subnormal entries, degenerate rows and labels, and t * m above 2^31 and 2^32
elements.  Everything but the pins of the restatements and of the inputs needs a real MI355X.
"""
import numpy as np
import pytest

from conftest import load_golden

U32 = 2.0 ** -24
U64 = 2.0 ** -53
TINY32 = 2.0 ** -149    # spacing of the float32 subnormals
C_HELL = 3.0
C_KL = 6.0
C_REP = 6.0
FLUSH = 256             # csrc/plsa_combine_kernels.hpp: `since_flush >= 256`
TILE = 64               # HELL_TILE
KSTEP = 32              # HELL_KSTEP
MAX_TOPICS = 65536      # plsa_all_pairs_*: t > 65536 is refused


# ------------------------------------------------------------------------------------------------
# float64 restatements
# ------------------------------------------------------------------------------------------------
def _common(T):
    """number of words where both rows are positive, [t, t] (float32 GEMM of 0 / 1: exact below 2^24)"""
    pos = (np.asarray(T) > 0).astype(np.float32)
    return (pos @ pos.T).astype(np.float64)


def hellinger64(T):
    """umap.distances.hellinger for every pair of rows, as enstop_.py:258-266 applies it: result = sum sqrt(x y),
    l1 norms of x and y; both norms zero -> 0, one zero -> 1, else sqrt(1 - result / sqrt(l1_x l1_y)).  Returns D and, for the
    bound, the Bhattacharyya sums g and the norms."""
    P = np.asarray(T, np.float64)
    l1 = P.sum(axis=1)
    root = np.sqrt(P)
    del P
    g = root @ root.T
    del root
    zero = l1 == 0
    denom = np.sqrt(np.outer(l1, l1))
    x = np.divide(g, denom, out=np.zeros_like(g), where=denom > 0)
    D = np.sqrt(np.maximum(1.0 - x, 0.0))
    D[np.outer(zero, zero)] = 0.0
    D[np.logical_xor.outer(zero, zero)] = 1.0
    return D, g, l1


def kl64(T):
    """enstop_.py:234-253: D[i, j] = sum over the words with p_i > 0 and p_j > 0 of p_i (log2 p_i - log2 p_j).  Returns D and
    S[i, j] = sum p_i (|log2 p_i| + |log2 p_j|) over the same words, the scale of the error bound."""
    P = np.asarray(T, np.float64)
    posm = P > 0
    L = np.zeros_like(P)
    np.log2(P, out=L, where=posm)
    pos = posm.astype(np.float64)
    del posm
    A = (P * L) @ pos.T          # sum p_i log2 p_i over the common support
    B = P @ L.T                  # sum p_i log2 p_j (log2 p_j stored as 0 where p_j == 0, p_i == 0 adds 0)
    if (L > 0).any():            # entries above 1: the magnitudes need their own products
        np.abs(L, out=L)
        S = (P * L) @ pos.T + P @ L.T
    else:
        S = -A - B
    D = A - B
    np.fill_diagonal(D, 0.0)     # p (log2 p - log2 p) is 0 term by term; the difference of the two products is not
    return D, S


def representatives64(T, labels, weights=None):
    """enstop_.py:299-308 / 340-345 (weights None: np.mean) and 385-393 (np.average with the membership strengths):
    (mean of sqrt(p) over the cluster) ** 2, divided by its sum.  A cluster id without a member is NumPy's mean of an empty
    slice: a row of NaN."""
    labels = np.asarray(labels)
    n_clusters = int(labels.max()) + 1 if labels.size and labels.max() >= 0 else 0
    t = labels.shape[0]
    M = np.zeros((n_clusters, t))
    for c in range(n_clusters):
        mask = labels == c
        M[c, mask] = 1.0 if weights is None else np.asarray(weights, np.float64)[mask]
    used = np.flatnonzero(M.any(axis=0))
    root = np.sqrt(np.asarray(T)[used].astype(np.float64))
    den = M.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = (M[:, used] @ root) / den[:, None]
        v = mean * mean
        return v / v.sum(axis=1, keepdims=True)


def host_slicing(t, m, cus, kind):
    """csrc/plsa_combine_plan.hpp vocab_slicing, as plsa_all_pairs_hellinger / plsa_all_pairs_kl (csrc/plsa_combine.hpp) call
    it, restated: the number of vocabulary slices wanted (`branch`), the words per slice (a multiple of the staging step) and
    the slices launched.  tests/test_combine_plan_host.py holds the header to this restatement."""
    nt = (t + TILE - 1) // TILE
    tiles = nt * (nt + 1) // 2 if kind == "hellinger" else nt * nt
    wanted = max(1, min(64, (4 * cus + tiles - 1) // tiles))
    words = ((m + wanted - 1) // wanted + KSTEP - 1) // KSTEP * KSTEP
    slices = (m + words - 1) // words
    branch = "few_tiles" if wanted == 64 else "chip_full" if wanted == 1 else "intermediate"
    return dict(branch=branch, wanted=wanted, slice=words, slices=slices, tiles=tiles,
                last=m - (slices - 1) * words)


# ------------------------------------------------------------------------------------------------
# the bounds
# ------------------------------------------------------------------------------------------------
def _offdiag_max(a):
    a = a.copy()
    np.fill_diagonal(a, 0.0)
    return float(a.max()) if a.size else 0.0


def check_hellinger(name, D, T, ratios=None, ref=None):
    """D from the device against hellinger64(T) under the bound of the module docstring; returns error / bound"""
    T = np.asarray(T)
    t, m = T.shape
    want, g, l1 = ref if ref is not None else hellinger64(T)
    assert D.shape == (t, t) and D.dtype == np.float64, (name, D.shape, D.dtype)
    assert np.isfinite(D).all(), "%s: %d non-finite distances" % (name, (~np.isfinite(D)).sum())
    np.testing.assert_array_equal(D.view(np.uint64), D.T.view(np.uint64), err_msg=name + ": not symmetric bit for bit")
    assert not np.diag(D).any(), name + ": diagonal"
    zero = l1 == 0
    both, one = np.outer(zero, zero), np.logical_xor.outer(zero, zero)
    assert (D[both] == 0).all() and (D[one] == 1).all(), name + ": zero-mass rows"
    common = _common(T)
    live = ~both & ~one & ~np.eye(t, dtype=bool)
    disjoint = live & (common == 0)
    assert (D[disjoint] == 1).all(), name + ": disjoint supports must be at distance 1 exactly"
    denom = np.sqrt(np.outer(l1, l1))
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.where(live, g / denom, 0.0)
        bound = ((np.minimum(FLUSH, common) + C_HELL) * U32 + 2 * m * U64) * x + common * TINY32 / denom + 8 * U64
    err = np.abs((1.0 - D * D) - x)
    ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
    assert ratio <= 1.0, "%s: |(1 - D^2) - x64| is %.3g x its bound at %s" % (
        name, ratio, np.unravel_index(np.argmax(np.where(live, err / np.where(live, bound, 1.0), 0.0)), D.shape))
    if ratios is not None:
        ratios["hellinger"] = max(ratios.get("hellinger", 0.0), ratio)
    return ratio


def check_kl(name, D, T, ratios=None, ref=None):
    T = np.asarray(T)
    t, m = T.shape
    want, S = ref if ref is not None else kl64(T)
    assert D.shape == (t, t) and D.dtype == np.float64, (name, D.shape, D.dtype)
    assert np.isfinite(D).all(), "%s: %d non-finite divergences" % (name, (~np.isfinite(D)).sum())
    assert not np.diag(D).any(), name + ": diagonal"
    common = _common(T)
    assert (D[common == 0] == 0).all(), name + ": disjoint supports must give 0 exactly"
    bound = (np.minimum(FLUSH, common) + C_KL) * U32 * S + common * TINY32
    err = np.abs(D - want)
    live = (bound > 0) & ~np.eye(t, dtype=bool)
    ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
    assert ratio <= 1.0, "%s: |D - D64| is %.3g x its bound at %s" % (
        name, ratio, np.unravel_index(np.argmax(np.where(live, err / np.where(live, bound, 1.0), 0.0)), D.shape))
    if ratios is not None:
        ratios["kl"] = max(ratios.get("kl", 0.0), ratio)
    return ratio


def check_representatives(name, R, want, ratios=None):
    assert R.shape == want.shape and R.dtype == np.float32, (name, R.shape, R.dtype, want.shape)
    nan = np.isnan(want)
    assert (np.isnan(R) == nan).all(), name + ": NaN rows (clusters without a member) differ"
    R, want = R[~nan].astype(np.float64), want[~nan]
    assert np.isfinite(R).all(), name + ": non-finite entries"
    assert not R[want == 0].any(), name + ": zeros of the restatement must be exact zeros"
    bound = C_REP * U32 * want + TINY32
    ratio = float((np.abs(R - want) / bound).max()) if want.size else 0.0
    assert ratio <= 1.0, "%s: |rep - rep64| is %.3g x its bound" % (name, ratio)
    if ratios is not None:
        ratios["representatives"] = max(ratios.get("representatives", 0.0), ratio)
    return ratio


# ------------------------------------------------------------------------------------------------
# CPU: the restatements pinned to the reference, the slicing, the inputs
# ------------------------------------------------------------------------------------------------
def _kl_pin(got, want, S, m):
    """the reference adds m float64 terms one after the other (numba, fastmath: any order), each with two libm
    logarithms, a subtraction and a product: within (m + 6) 2^-53 of the sum of magnitudes"""
    assert (np.abs(got - want) <= (m + 6) * U64 * S).all(), float(np.abs(got - want).max())


def test_kl64_reproduces_the_reference_run():
    g = load_golden("combine_t24")
    T = g["topics"]
    t, m = T.shape
    D, S = kl64(T)
    _kl_pin(g["kl_f64_input"], D, S, m)
    assert not np.diag(D).any()
    # the reference's float32-input run: float32 logarithms, subtraction and product (3 + 1 + 1 roundings of 2^-24 at
    # most), added in float64
    assert (np.abs(g["kl_f32_input"] - D) <= 5 * U32 * S + m * U64 * S).all()
    # the pin is not vacuous: two rows swapped, one word dropped from one row
    swapped = T.copy()
    swapped[[2, 3]] = swapped[[3, 2]]
    with pytest.raises(AssertionError):
        _kl_pin(g["kl_f64_input"], *kl64(swapped), m)
    dropped = T.copy()
    dropped[5, np.argmax(dropped[5] > 0)] = 0.0
    with pytest.raises(AssertionError):
        _kl_pin(g["kl_f64_input"], *kl64(dropped), m)


def _rep_pin(got, want, n_c, m):
    """the reference: float32 roots, a float32 mean over n_c rows (n_c roundings), a float32 square, a float32 sum of m
    non-negative entries in some order (m - 1) and a float32 division: entry 2 (n_c + 1) + 1, its sum the same plus m,
    the division 1 -> (4 n_c + m + 8) 2^-24, relative, entry by entry"""
    got = got.astype(np.float64)
    assert not got[want == 0].any()
    assert (np.abs(got - want) <= (4 * n_c + m + 8) * U32 * want).all(), float((np.abs(got - want) / np.maximum(want, 1e-300)).max())


def test_representatives64_reproduces_the_reference_run():
    g = load_golden("combine_t24")
    T, labels, probs = g["topics"], g["labels"], g["probabilities"]
    m = T.shape[1]
    n_c = int(np.bincount(labels[labels >= 0]).max())
    for key, w in (("rep_kl", None), ("rep_hellinger", None), ("rep_umap", probs)):
        _rep_pin(g[key], representatives64(T, labels, w), n_c, m)
    # not vacuous: a wrong label, a dropped word, two rows swapped across clusters
    wrong = labels.copy()
    wrong[0] = 1
    with pytest.raises(AssertionError):
        _rep_pin(g["rep_kl"], representatives64(T, wrong), n_c, m)
    dropped = T.copy()
    dropped[0, np.argmax(dropped[0])] = 0.0
    with pytest.raises(AssertionError):
        _rep_pin(g["rep_kl"], representatives64(dropped, labels), n_c, m)
    swapped = T.copy()
    swapped[[0, 2]] = swapped[[2, 0]]
    with pytest.raises(AssertionError):
        _rep_pin(g["rep_umap"], representatives64(swapped, labels, probs), n_c, m)


def test_hellinger64_is_the_published_definition():
    """No reference run of the Hellinger matrix exists (umap-learn is not installable where the goldens are made).
    hellinger64 is held to umap.distances.hellinger's published statements evaluated pair by pair, coordinate by coordinate."""
    def hellinger(x, y):
        result = l1_norm_x = l1_norm_y = 0.0
        for i in range(x.shape[0]):
            result += np.sqrt(x[i] * y[i])
            l1_norm_x += x[i]
            l1_norm_y += y[i]
        if l1_norm_x == 0 and l1_norm_y == 0:
            return 0.0
        if l1_norm_x == 0 or l1_norm_y == 0:
            return 1.0
        return np.sqrt(max(1 - result / np.sqrt(l1_norm_x * l1_norm_y), 0.0))
    T = load_golden("combine_t24")["topics"][:12, :60].astype(np.float64)
    T[4] = 0.0
    T[7] = 0.0
    T[9] = T[8]
    T[10, :30] = 0.0
    T[11, 30:] = 0.0
    D, g, l1 = hellinger64(T)
    t, m = T.shape
    for i in range(t):
        for j in range(t):
            want = hellinger(T[i], T[j])
            # 1 - x carries m roundings of 2^-53 from either evaluation; the root of it is compared through its square
            assert abs(D[i, j] ** 2 - want ** 2) <= 4 * m * U64, (i, j, D[i, j], want)
    assert D[4, 7] == 0 and D[4, 0] == 1 and D[0, 7] == 1 and D[10, 11] == 1
    others = [k for k in range(t) if k not in (8, 9)]
    assert np.array_equal(D[8, others], D[9, others])            # identical rows
    # the product's host definition is a separate implementation of the same matrix
    from enstop_amd.ensemble import all_pairs_hellinger_distance, all_pairs_kl_divergence
    off = ~np.eye(t, dtype=bool)
    assert np.abs(all_pairs_hellinger_distance(T)[off] ** 2 - D[off] ** 2).max() <= 4 * m * U64
    K, S = kl64(T)
    assert (np.abs(all_pairs_kl_divergence(T) - K) <= 4 * m * U64 * S).all()


# (t, m, branch of the Hellinger slicing, branch of the KL slicing) on 256 CUs
SPIKE_CASES = [
    (1, 1, "few_tiles", "few_tiles"), (3, 1, "few_tiles", "few_tiles"), (1, 1000, "few_tiles", "few_tiles"),
    (5, 7, "few_tiles", "few_tiles"), (33, 31, "few_tiles", "few_tiles"),
    (64, 4037, "few_tiles", "few_tiles"),          # 64 slices of 64 words, the last one 5 words: shorter than a staging step
    (64, 4099, "few_tiles", "few_tiles"), (65, 4099, "few_tiles", "few_tiles"),
    (128, 10007, "few_tiles", "few_tiles"), (129, 10007, "few_tiles", "few_tiles"),
    (640, 20011, "intermediate", "intermediate"), (1280, 5003, "intermediate", "intermediate"),
    (2048, 2053, "intermediate", "chip_full"),     # KL launches nt^2 = 1024 tiles = 4 x 256 CUs, Hellinger 528
    (2817, 1031, "chip_full", "chip_full"),        # nt = 45: nt (nt + 1) / 2 = 1035 tiles
]
MI355X_CUS = 256


def test_spike_cases_reach_every_branch_of_the_slicing():
    seen = {"hellinger": set(), "kl": set()}
    for t, m, hb, kb in SPIKE_CASES:
        for kind, want in (("hellinger", hb), ("kl", kb)):
            s = host_slicing(t, m, MI355X_CUS, kind)
            assert s["branch"] == want, (t, m, kind, s)
            assert s["slice"] % KSTEP == 0 and (s["slices"] - 1) * s["slice"] < m <= s["slices"] * s["slice"], s
            seen[kind].add(s["branch"])
    assert seen["hellinger"] == seen["kl"] == {"few_tiles", "intermediate", "chip_full"}
    # where the two kernels part: t = 1985 ... 2816 is chip_full for KL only
    assert host_slicing(1984, 100, 256, "kl")["wanted"] == 2 and host_slicing(1985, 100, 256, "kl")["wanted"] == 1
    assert host_slicing(2816, 100, 256, "hellinger")["wanted"] == 2 and host_slicing(2817, 100, 256, "hellinger")["wanted"] == 1
    s = host_slicing(64, 4037, 256, "hellinger")
    assert (s["slices"], s["slice"], s["last"]) == (64, 64, 5)
    assert host_slicing(5, 7, 256, "kl")["slices"] == 1 and host_slicing(1, 1, 256, "kl")["slices"] == 1


def test_partial_buffer_never_needs_a_cap():
    """slices * tiles stays near 4 x CUs, so the [slices, t, t] float64 partial buffer with slices > 1 peaks far below the
    4e9 bytes the host code used to cap it at: the cap was a branch no input reaches and is gone."""
    peak = 0.0
    for cus in range(64, 305, 8):
        for kind in ("hellinger", "kl"):
            for nt in range(1, MAX_TOPICS // TILE + 1):
                t = nt * TILE                                    # the largest t of its tile count
                wanted = host_slicing(t, 1 << 20, cus, kind)["wanted"]
                if wanted > 1:
                    peak = max(peak, wanted * float(t) * t * 8.0)
    assert peak <= 1.6e8, peak


# ---- production-shaped families (3b): the inputs, and the condition on them
N_WORDS = 173762
N_FAMILIES = 20
MIN_SAMPLES, MIN_CLUSTER_SIZE = 5, 5


def family_topics(t, m=N_WORDS, seed=11):
    """20 families of near-duplicate topics: a Dirichlet(1) base times (1 + 5 % noise), renormalised; float32, no entry
    below FLT_MIN.  Row i belongs to family i % 20."""
    rs = np.random.RandomState(seed + t)
    base = rs.standard_exponential((N_FAMILIES, m)) + 1e-9
    base /= base.sum(axis=1, keepdims=True)
    T = np.empty((t, m), np.float32)
    for i in range(t):
        row = base[i % N_FAMILIES] * (1.0 + 0.05 * rs.standard_normal(m).clip(-4, 4))
        T[i] = row / row.sum()
    assert (T >= 2.0 ** -126).all()
    return T, np.arange(t) % N_FAMILIES


def same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or (a < 0).any() != (b < 0).any():
        return False
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def hellinger_labels(D):
    from enstop_amd.hdbscan_tree import hdbscan_precomputed_leaf
    D = D.copy()
    np.fill_diagonal(D, 0.0)            # hellinger64 leaves the rounding of 1 - x there, the device writes 0
    return hdbscan_precomputed_leaf(D, MIN_SAMPLES, MIN_CLUSTER_SIZE)[0]


def kl_labels(D):
    from enstop_amd.ensemble import mutual_reachability_from_divergences
    from enstop_amd.hdbscan_tree import labels_from_mutual_reachability
    return labels_from_mutual_reachability(mutual_reachability_from_divergences(D, MIN_SAMPLES), MIN_CLUSTER_SIZE)[0]


@pytest.mark.parametrize("t", [640, 1280])
def test_family_inputs_cluster_into_their_families_in_float64(t):
    """The condition test_production_shape_families relies on: the float64 matrices alone give the 20 families, no noise,
    and hold the small within-family entries next to the large ones."""
    T, family = family_topics(t)
    D, g, l1 = hellinger64(T)
    same = family[:, None] == family[None, :]
    off = ~np.eye(t, dtype=bool)
    assert D[same & off].max() < 0.1 * D[~same].min()
    assert same_partition(hellinger_labels(D), family)
    K, S = kl64(T)
    assert K[same & off].max() < 0.1 * K[~same].min() and K[off].min() > 0
    assert same_partition(kl_labels(K), family)


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
    if out:
        print("\ntopic combination: worst error / bound per kind: " +
              ", ".join("%s %.3g" % (key, v) for key, v in sorted(out.items())))


def spike_positions(m, s):
    """words at the staging, flush-window and slice boundaries of one slicing"""
    w, n = s["slice"], s["slices"]
    cand = [0, 31, 32, 255, 256, w - 1, w, w + 1, w + 255, w + 256, (n - 1) * w - 1, (n - 1) * w, m - 1]
    return sorted({c for c in cand if 0 <= c < m})


def spike_topics(t, m, s, seed):
    """Rows 0, 63, 64, 65 and t - 1 carry mass on every boundary word and nowhere else (a dozen words at most: one missed or
    doubled word moves an entry by several per cent, the bound is ~ 20 u).  Every other row carries 3 of those words and 2
    random ones, so no row or column of the matrix is interchangeable with another."""
    rs = np.random.RandomState(seed)
    pos = np.array(spike_positions(m, s))
    T = np.zeros((t, m), np.float64)
    special = [i for i in (0, 63, 64, 65, t - 1) if 0 <= i < t]
    for i in range(t):
        if i in special:
            T[i, pos] = rs.uniform(0.75, 1.25, pos.shape[0])
        else:
            some = rs.choice(pos, min(3, pos.shape[0]), replace=False)
            T[i, some] = rs.uniform(0.5, 1.5, some.shape[0])
            T[i, rs.randint(0, m, 2)] += rs.uniform(0.5, 1.5, 2)
    T = (T / T.sum(axis=1, keepdims=True)).astype(np.float32)
    assert _common(T).max() <= 16
    return T, pos


@pytest.mark.gpu
@pytest.mark.parametrize("t, m, hell_branch, kl_branch", SPIKE_CASES)
def test_boundary_spikes(amd, worst, t, m, hell_branch, kl_branch):
    eng = amd.engine.get_engine()
    cus = eng.device_info()["cus"]
    out = []
    for kind, branch in (("hellinger", hell_branch), ("kl", kl_branch)):
        s = host_slicing(t, m, cus, kind)
        assert s["branch"] == branch, "%s slicing at t=%d m=%d on %d CUs: %r, the case is meant to reach %s" % (
            kind, t, m, cus, s, branch)
        T, pos = spike_topics(t, m, s, seed=t * 7 + m)
        if kind == "hellinger":
            r = check_hellinger("spikes hellinger t=%d m=%d" % (t, m), eng.all_pairs_hellinger(T), T, worst)
        else:
            r = check_kl("spikes kl t=%d m=%d" % (t, m), eng.all_pairs_kl(T), T, worst)
        out.append("%s %s (%d slices of %d words, last %d; %d boundary words) error / bound %.3g" % (
            kind, s["branch"], s["slices"], s["slice"], s["last"], pos.shape[0], r))
        if kind == "kl":                    # the representatives of the same rows: three clusters and noise
            labels = (np.arange(t) % 4 - 1).astype(np.int64)
            labels[[i for i in (0, t - 1) if i < t]] = 0
            w = np.random.RandomState(t).rand(t)
            w[::5] = 0.0
            w[0] = 0.5
            for weights in (None, w):
                populated = all((weights if weights is not None else np.ones(t))[labels == c].sum() > 0
                                for c in range(labels.max() + 1))
                if populated:
                    r = check_representatives("spikes representatives t=%d m=%d" % (t, m),
                                              eng.cluster_representatives(T, labels, weights),
                                              representatives64(T, labels, weights), worst)
                    out.append("representatives error / bound %.3g" % r)
    print("\nt=%d m=%d: %s" % (t, m, "; ".join(out)))


@pytest.mark.gpu
@pytest.mark.parametrize("t", [640, 1280])
def test_production_shape_families(amd, worst, t):
    """t = 32 and 64 members x 20 topics over the 173 762 words of the flagship corpus, dense rows; one float64 evaluation
    per matrix (test_family_inputs_cluster_into_their_families_in_float64 checks the same matrices without a GPU)."""
    from enstop_amd.engine import reset_engines
    reset_engines()
    T, family = family_topics(t)
    cus = None
    with amd.Engine() as eng:
        cus = eng.device_info()["cus"]
        Dh = eng.all_pairs_hellinger(T)
        Dk = eng.all_pairs_kl(T)
        w = np.random.RandomState(t).rand(t)
        w[::7] = 0.0
        reps = [eng.cluster_representatives(T, family, weights) for weights in (None, w)]
    ref = hellinger64(T)
    rh = check_hellinger("families hellinger t=%d" % t, Dh, T, worst, ref=ref)
    assert same_partition(hellinger_labels(ref[0]), family)
    # label for label, not only the same partition: the numbering follows the order of nearly equal merge heights
    np.testing.assert_array_equal(hellinger_labels(Dh), hellinger_labels(ref[0]))
    del ref
    ref = kl64(T)
    rk = check_kl("families kl t=%d" % t, Dk, T, worst, ref=ref)
    assert same_partition(kl_labels(ref[0]), family)
    np.testing.assert_array_equal(kl_labels(Dk), kl_labels(ref[0]))
    del ref
    rr = max(check_representatives("families representatives t=%d" % t, R, representatives64(T, family, weights), worst)
             for R, weights in zip(reps, (None, w)))
    print("\nfamilies t=%d m=%d: hellinger %s error / bound %.3g; kl %s error / bound %.3g; representatives %.3g" % (
        t, N_WORDS, host_slicing(t, N_WORDS, cus, "hellinger")["branch"], rh,
        host_slicing(t, N_WORDS, cus, "kl")["branch"], rk, rr))


def tiny_topics(side, t=70, m=1000, seed=21):
    """Dirichlet rows with, in the rows of `side`, 200 words each replaced by positive entries spread over
    2^-149 ... 2^-120 (FLT_MIN = 2^-126): subnormal, the smallest normals, and 2^-149 / 2^-127 / 2^-126 themselves."""
    rs = np.random.RandomState(seed)
    T = rs.dirichlet(np.full(m, 0.5), size=t).astype(np.float32)
    T = np.maximum(T, np.float32(1e-30))
    rows = {"row": range(0, 10), "col": range(60, 70), "both": list(range(0, 10)) + list(range(60, 70))}[side]
    for i in rows:
        words = rs.choice(m, 200, replace=False)
        T[i, words] = np.ldexp(rs.uniform(1.0, 2.0, 200), -rs.randint(121, 150, 200)).astype(np.float32)
        T[i, words[:3]] = np.array([2.0 ** -149, 2.0 ** -127, 2.0 ** -126], np.float32)
    assert (T > 0).all()
    sub = (T < 2.0 ** -126).sum(axis=1)
    assert all(sub[i] >= 100 for i in rows) and sub.sum() == sum(sub[i] for i in rows)
    return T


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["row", "col", "both", "dirichlet150"])
def test_tiny_and_subnormal_entries(amd, worst, side):
    """Positive entries below FLT_MIN are reachable (e_step_thresh = 1e-32 over a norm_pwz of 1e5 ... 1e7) and v_log_f32
    does not take subnormal inputs: every output finite and within the bounds.  "dirichlet150" is the ragged case of
    test_hip_parity.py::test_device_all_pairs_kl_vs_reference WITHOUT its `< 1e-7 -> 0` clamp."""
    if side == "dirichlet150":
        T = np.random.RandomState(5).dirichlet(np.full(3001, 0.05), size=150).astype(np.float32)
        T[7] = 0.0
        assert ((T > 0) & (T < 2.0 ** -126)).any() and ((T > 0) & (T < 1e-7)).sum() > 1000
    else:
        T = tiny_topics(side)
    t = T.shape[0]
    eng = amd.engine.get_engine()
    rk = check_kl("tiny kl " + side, eng.all_pairs_kl(T), T, worst)
    rh = check_hellinger("tiny hellinger " + side, eng.all_pairs_hellinger(T), T, worst)
    labels = (np.arange(t) % 3).astype(np.int64)
    w = 0.25 + np.random.RandomState(3).rand(t)
    rr = max(check_representatives("tiny representatives " + side, eng.cluster_representatives(T, labels, weights),
                                   representatives64(T, labels, weights), worst) for weights in (None, w))
    print("\ntiny entries (%s): kl error / bound %.3g, hellinger %.3g, representatives %.3g" % (side, rk, rh, rr))


@pytest.mark.gpu
def test_degenerate_rows_and_labels(amd, worst):
    from enstop_amd import ensemble as E
    from enstop_amd.engine import DeviceError
    eng = amd.engine.get_engine()
    rs = np.random.RandomState(31)
    t, m = 70, 500
    T = rs.dirichlet(np.full(m, 0.3), size=t).astype(np.float32)
    T[T < 1e-6] = 0.0
    T[[3, 64, 69]] = 0.0                                # rows without mass
    T[10] = T[9]
    T[66] = T[2]                                        # identical rows, within and across tiles
    T[20, : m // 2] = 0.0
    T[21, m // 2:] = 0.0
    T[67, m // 2:] = 0.0                                # 20 is disjoint from 21 and 67
    Dh = eng.all_pairs_hellinger(T)
    Dk = eng.all_pairs_kl(T)
    rh = check_hellinger("degenerate hellinger", Dh, T, worst)
    rk = check_kl("degenerate kl", Dk, T, worst)
    assert Dh[20, 21] == 1 and Dh[67, 20] == 1 and Dh[3, 64] == 0 and Dh[3, 0] == 1
    assert Dk[20, 21] == 0 and Dk[9, 10] == 0 and Dk[10, 9] == 0 and Dk[66, 2] == 0 and not Dk[3].any() and not Dk[:, 3].any()

    # -- labels
    noise = np.full(t, -1, np.int64)
    for R in (eng.cluster_representatives(T, noise), E._cluster_representatives(T, noise, engine=eng)):
        assert R.shape == (0, m) and R.dtype == np.float32
    labels = (np.arange(t) % 3).astype(np.int64)
    labels[labels == 1] = -1                            # cluster 1 has no member
    labels[5] = 3                                       # cluster 3 has one
    want = representatives64(T, labels)
    assert np.isnan(want[1]).all() and np.isfinite(want[[0, 2, 3]]).all()
    # enstop_.py:299-308 on such labels is NumPy's mean of an empty slice: a row of NaN (and a RuntimeWarning).  The
    # device (0 / 0 in k_rep_normalise), the host expressions and the combiner's helper all return that row.
    with np.errstate(invalid="ignore", divide="ignore"), pytest.warns(RuntimeWarning):
        host = E._cluster_representatives(T, labels)
    for R in (eng.cluster_representatives(T, labels), E._cluster_representatives(T, labels, engine=eng)):
        check_representatives("empty cluster", R, want, worst)
        assert np.isnan(R[1]).all() and np.isnan(host[1]).all()
    one = T[5].astype(np.float64)
    check_representatives("single member", eng.cluster_representatives(T, labels)[3:4], (one / one.sum())[None, :], worst)
    # with membership strengths the reference's np.average raises on a cluster whose weights sum to zero
    w = rs.rand(t)
    for kw in (dict(engine=eng), dict()):
        with pytest.raises(ZeroDivisionError):
            E._cluster_representatives(T, labels, w, **kw)
    labels3 = (np.arange(t) % 3).astype(np.int64)
    w[labels3 == 2] = 0.0
    w[5] = 0.7                                          # zeros inside a populated cluster (5 % 3 == 2)
    w[::4] = 0.0
    w[1] = 0.3
    rr = check_representatives("zero weights", E._cluster_representatives(T, labels3, w, engine=eng),
                               representatives64(T, labels3, w), worst)

    # -- error returns leave the engine usable
    from enstop_amd._lib import ptr
    for fn in (eng.all_pairs_hellinger, eng.all_pairs_kl):
        with pytest.raises(DeviceError):
            fn(np.zeros((MAX_TOPICS + 1, 1), np.float32))
        assert fn(np.ones((MAX_TOPICS, 1), np.float32)[:2]).shape == (2, 2)
    with pytest.raises(ValueError):
        eng.cluster_representatives(T, labels3[:-1])
    out = np.empty((2, m), np.float32)
    lab = np.ascontiguousarray(labels3, np.int32)                    # label 2 with n_clusters = 2
    assert eng._L.plsa_cluster_representatives(eng._h, ptr(T), t, m, lab, None, 2, out) != 0
    assert "n_clusters" in eng._L.plsa_last_error(eng._h).decode()
    check_hellinger("after the errors: hellinger", eng.all_pairs_hellinger(T), T)
    check_kl("after the errors: kl", eng.all_pairs_kl(T), T)
    check_representatives("after the errors: representatives", eng.cluster_representatives(T, labels3),
                          representatives64(T, labels3))
    print("\ndegenerate rows: hellinger error / bound %.3g, kl %.3g, representatives (zero weights) %.3g" % (rh, rk, rr))


@pytest.mark.gpu
def test_more_clusters_than_grid_rows_are_refused_by_name(amd):
    """A cluster is a row of the representatives' launch grid (gridDim.y, at most 65535): 65536 clusters are refused before
    anything is allocated instead of failing at the launch; 65535 run.  The engine stays usable."""
    from enstop_amd._lib import ptr
    t, m = 8, 3
    eng = amd.engine.get_engine()
    T = np.random.RandomState(0).dirichlet(np.ones(m), size=t).astype(np.float32)
    lab = np.arange(t, dtype=np.int32)
    out = np.zeros((65536, m), np.float32)
    assert eng._L.plsa_cluster_representatives(eng._h, ptr(T), t, m, lab, None, 65536, out) != 0
    assert "n_clusters=65536" in eng._L.plsa_last_error(eng._h).decode()
    assert eng._L.plsa_cluster_representatives(eng._h, ptr(T), t, m, lab, None, 65535, out) == 0
    check_representatives("65535 clusters", out[:t], representatives64(T, lab))
    assert np.isnan(out[t:65535]).all()                    # clusters without a member: NumPy's mean of an empty slice


def _mem_available():
    with open("/proc/meminfo") as f:
        for line in f:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    return 0


def _index_width_case(amd, worst, t, m, edge):
    """almost all rows zero; spikes in the first rows, the rows around element `edge` and the last rows"""
    rs = np.random.RandomState(t)
    row = edge // m
    live = np.unique([i for i in (0, 1, 2, 65, row - 1, row, row + 1, t - 3, t - 2, t - 1) if 0 <= i < t])
    assert row + 1 < t - 3 and t * m > edge
    T = np.zeros((t, m), np.float32)                    # untouched pages stay unmapped on the host
    cus = None
    words = sorted({w for kind in ("hellinger", "kl") for w in spike_positions(m, host_slicing(t, m, MI355X_CUS, kind))}
                   | {edge - row * m, max(edge - row * m - 1, 0)})
    for i in live:
        T[i, words] = rs.uniform(0.5, 1.5, len(words)) / len(words)
        T[i, rs.randint(0, m, 3)] = 0.05
    sub = np.ascontiguousarray(T[live])
    labels = np.full(t, -1, np.int64)
    labels[[0, t - 1]] = 0                              # a cluster made of the first and the last row
    labels[[row, row + 1]] = 1
    with amd.Engine() as eng:
        cus = eng.device_info()["cus"]
        Dh = eng.all_pairs_hellinger(T)
        Dk = eng.all_pairs_kl(T)
        R = eng.cluster_representatives(T, labels)
    dead = np.ones(t, bool)
    dead[live] = False
    # the zero-mass pattern everywhere else, exactly
    assert not Dk[dead].any() and not Dk[:, dead].any()
    assert not Dh[np.ix_(dead, dead)].any() and (Dh[np.ix_(dead, live)] == 1).all() and (Dh[np.ix_(live, dead)] == 1).all()
    rh = check_hellinger("t*m=%.3g hellinger" % (t * m), np.ascontiguousarray(Dh[np.ix_(live, live)]), sub, worst)
    rk = check_kl("t*m=%.3g kl" % (t * m), np.ascontiguousarray(Dk[np.ix_(live, live)]), sub, worst)
    sub_labels = labels[live]
    rr = check_representatives("t*m=%.3g representatives" % (t * m), R, representatives64(sub, sub_labels), worst)
    print("\nt=%d m=%d (%.4g elements, row %d holds element %d): hellinger %s error / bound %.3g; kl %s %.3g; representatives %.3g"
          % (t, m, t * m, row, edge, host_slicing(t, m, cus, "hellinger")["branch"], rh,
             host_slicing(t, m, cus, "kl")["branch"], rk, rr))


@pytest.mark.gpu
def test_index_width(amd, worst):
    """t * m above 2^31 elements, and above 2^32 where the host has the memory: row offsets `i * m + w` beyond 32 bits in
    every kernel of the three families."""
    from enstop_amd.engine import reset_engines
    reset_engines()
    t, m = 2112, (1 << 20) + 37
    need = t * m * 4 + (2 << 30)
    have = _mem_available()
    assert have >= need, "the 2^31-element case needs %.1f GB of host memory, %.1f GB are available" % (need / 1e9, have / 1e9)
    _index_width_case(amd, worst, t, m, 1 << 31)
    t = 4160
    need = t * m * 4 + (2 << 30)
    have = _mem_available()
    if have >= need:
        _index_width_case(amd, worst, t, m, 1 << 32)
    else:
        print("\nthe 2^32-element case was not run: it needs %.1f GB of host memory, %.1f GB are available" % (need / 1e9, have / 1e9))
