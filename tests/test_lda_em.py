"""Variational Bayes LDA on the device (include/plsa_hip_diag.h: plsa_lda_fit, plsa_lda_refit, plsa_lda_bound, plsa_lda_tables;
enstop_amd/lda.py) against the float64 model of tests/lda_model.py.

    A_dz = exp(psi(gamma_dz) - psi(S_d))        B_zw = exp(psi(lambda_zw) - psi(S_z))
    gamma_dz = alpha + sum_w x_dw phi_dwz        lambda_zw = eta + sum_d x_dw phi_dwz        phi_dwz ~ A_dz B_zw
    L = sum x_dw log sum_z A_dz B_zw + the Dirichlet parts of gamma and lambda (lda_model.py)

Kernel-level tests run on matrix_corpus(k) of test_pass_matrix.py (640 x 480, about 4 000 non-zeros: two empty documents, the
300-word document of the row-item path, the heavy word, stored zeros) with the entries of word 9 taken out, so that one word
has no entries, for k in {3, 6, 21, 64, 130, 1024}: kq = 1, padding topics, the 8 x 2 document shape, rows that straddle
workgroups raggedly (kq = 33), rows that are whole workgroups (kq = 256).  (alpha, eta) runs over (0.5, 0.5), (0.1, 0.05) and,
for k <= 64, (1 / k, 1 / k).  The start is gamma0 = alpha + 20 U0, lambda0 = eta + 50 V0, set through set_factors.

Error model (u = 2^-24; s = 4 (L + k) u is the bound of a plain step's entry and of its norm, test_pass_matrix.py's docstring).
  Tables: an entry is exp(psi(x) - psi(S)) evaluated in float64 and rounded to float32 once: u.  The float64 evaluation: two
    digammas of absolute error 2^-40 each (test_lda_math_host.py) and exp's rounding, 2^-39 + 2^-53 relative.  S: a row sum of
    gamma is a float64 sum of k <= 1024 float32 entries, a topic sum of lambda a float64 sum of m = 480: at most 1024 2^-53
    relative, which psi carries into the entry times S psi'(S) <= 1 + 1 / S <= 5 (S >= k alpha >= 0.3 here): 2^-40.  The
    model's SciPy values carry as much again.  t = u + 2^-37 < (1 + 2^-12) u, far inside the 3 u the derivation may not exceed.
  gamma: the device forms fmaf(u_z, N_d, alpha) from the pass's u_z (error s) and N_d (error s): u_z N_d carries s + s, adding a
    prior >= 0 does not raise a relative error, two roundings (the multiply-add, (float)alpha).  The pass ran on tables that
    differ from the model's by t each: a responsibility A B / sum A B moves by at most 2 t from its numerator and 2 t from its
    denominator, so a count moves by at most 4 t.  2 s_row + 2 u + 4 t.
  lambda: Vacc + (float)eta: the entry's s, one rounding, the tables' 4 t: s_col + u + 4 t.
  An empty document gets (float)alpha and a word without entries (float)eta: within u.
  L: check_ll's bound for the likelihood term, 2^-50 sum |terms| for the float64 Dirichlet sums (lda_model.bound64's scale: the
    summed terms lgamma(x) + (prior - x)(psi(x) - psi(S)) and lgamma(S), and the parts of the constants), |L| u for a float32
    trace value.  The likelihood term is k_loglik on the scaled tables plus sum x (shift_d + shift_w), a float64 sum whose
    |terms| are in the scale as well.
  The scaling: the passes run on tables whose rows (a document's of A, a word's of B) are divided by their largest entry, which
    the responsibilities do not see; lda_tables() reads the tables of the definition back, the model's step runs on the scaled
    ones (lda_model.scaled_tables64).  Without it A = 1.6e-28 times B = 1.5e-30 underflows at k = 64 and priors of 1 / 64, and
    psi(0.01) = -100.6 leaves float32 on its own.  A shift is a float64 digamma difference on either side: its error, 2^-39, is
    inside t.

The pad columns k .. kp of the tables and of the state cannot be read through the ABI (its host tables are [n, k] and [k, m]).
The kernels write 0 there by the plan's mask, which tests/test_smoothed_plan_host.py checks for every float4; here every
following step is held to the model, which never sees a pad.

doc_iter: the header defines an iteration with doc_iter = d as d - 1 gamma-only rounds and one full round.  So doc_iter = 3 is
held to two refit steps and a full step, and three refit steps followed by a full step are what doc_iter = 4 runs; both are
checked.

The communicator refusal runs on a one-rank RCCL communicator, created the way tests/test_smoothed_em.py creates one.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import lda_model as lm
import smoothed_model as sm
from test_capped_grids import CAP, knobs as cap_knobs, sizes
from test_fit_driver import PLSA_FUSED, PLSA_GRAPH, PLSA_SHARDED, make_engine, same_bits
from test_pass_matrix import C_FACTOR, EMPTY_DOCS, U32, check, matrix_corpus

PLSA_REFERENCE_SUMS, PLSA_REFERENCE_LL = 256, 512
THRESH = 1e-32
K = [3, 6, 21, 64, 130, 1024]
UNUSED_WORD = 9
T_BOUND = (1 + 2.0 ** -12) * U32
ONE = dict(n_iter=1, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED)


def priors(k):
    return [(0.5, 0.5), (0.1, 0.05)] + ([(1.0 / k, 1.0 / k)] if k <= 64 else [])


@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


@pytest.fixture(scope="module")
def worst():
    out = {}
    yield out
    for k in sorted(out):
        print("\nLDA k=%d: worst error / bound: " % k + ", ".join("%s %.3g" % kv for kv in sorted(out[k].items())))


@functools.lru_cache(maxsize=None)
def corpus(k):
    """matrix_corpus(k) without the entries of word 9: (X, U0, V0)"""
    X, U0, V0, _ = matrix_corpus(k)
    X = X.tocsr()
    rows = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    keep = X.indices != UNUSED_WORD
    X = sp.csr_matrix((X.data[keep], (rows[keep], X.indices[keep])), shape=X.shape)
    assert np.diff(X.tocsc().indptr)[UNUSED_WORD] == 0 and (X.data == 0).sum() >= 30
    return X, U0, V0


@functools.lru_cache(maxsize=None)
def start(k, alpha, eta):
    X, U0, V0 = corpus(k)
    return (np.float32(alpha) + 20 * U0).astype(np.float32), (np.float32(eta) + 50 * V0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def model_step(k, alpha, eta):
    X, _, _ = corpus(k)
    gamma0, lam0 = start(k, alpha, eta)
    return lm.lda_step64(X, gamma0, lam0, alpha, eta, THRESH)


def step_bounds(s, k):
    s_row, s_col = C_FACTOR * (s["L_row"] + k) * U32, C_FACTOR * (s["L_col"] + k) * U32
    return 2 * s_row + 2 * U32 + 4 * T_BOUND, s_col + U32 + 4 * T_BOUND


def check_step(tag, gamma, lam, want, k, alpha, eta, ratios, topics=True):
    b_u, b_v = step_bounds(want, k)
    check("gamma " + tag, gamma, want["gamma"], b_u, ratios)
    assert (gamma > 0).all(), tag
    for d in EMPTY_DOCS:
        check("empty document " + tag, gamma[d], np.full(k, alpha), U32, ratios)
    if topics:
        check("lambda " + tag, lam, want["lam"], b_v, ratios)
        assert (lam > 0).all(), tag
        check("word without entries " + tag, lam[:, UNUSED_WORD], np.full(k, eta), U32, ratios)


def check_bound(tag, got, X, gamma, lam, k, alpha, eta, ratios, float32=True):
    want, ll_scale, scale = lm.bound64(X, gamma, lam, alpha, eta)
    bound = C_FACTOR * (k + 1) * U32 * ll_scale + 2.0 ** -50 * scale + (abs(want) * U32 if float32 else 0.0)
    err = abs(float(got) - want)
    print("%s: L %.6f, model %.6f, error %.3g, bound %.3g" % (tag, got, want, err, bound))
    assert err <= bound, (tag, got, want, err, bound)
    ratios["L"] = max(ratios.get("L", 0.0), err / bound)


# ------------------------------------------------------------------------------------------------
# 1. the tables
# ------------------------------------------------------------------------------------------------
def test_the_derived_table_bound_is_within_three_u():
    assert T_BOUND <= 3 * U32
    assert U32 + 2.0 ** -37 <= T_BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_tables_against_the_model(amd, worst, k):
    X, _, _ = corpus(k)
    ratios = worst.setdefault(k, {})
    with make_engine(amd, {}, X) as eng:
        for alpha, eta in priors(k):
            gamma0, lam0 = start(k, alpha, eta)
            eng.set_factors(gamma0, lam0)
            A, B = eng.lda_tables()
            A64, B64 = lm.tables64(gamma0, lam0)
            assert A64.min() > 2.0 ** -126 and B64.min() > 2.0 ** -126         # every entry a normal float32
            check("A", A, A64, T_BOUND, ratios)
            check("B", B, B64, T_BOUND, ratios)
            g, l = eng.get_factors()                                          # the state stays as it is
            same_bits(g, gamma0, "lda_tables moved gamma")
            same_bits(l, lam0, "lda_tables moved lambda")


# ------------------------------------------------------------------------------------------------
# 2. one step, entry by entry
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_one_step_against_the_model(amd, worst, k):
    X, _, _ = corpus(k)
    ratios = worst.setdefault(k, {})
    with make_engine(amd, {}, X) as eng:
        eng.timing(True)
        for alpha, eta in priors(k):
            gamma0, lam0 = start(k, alpha, eta)
            want = model_step(k, alpha, eta)
            eng.set_factors(gamma0, lam0)
            eng.timing_reset()
            iters, trace = eng.lda_fit(alpha, eta, trace=True, **ONE)
            names = eng.timing_report()
            gamma, lam = eng.get_factors()
            tag = "alpha=%g eta=%g" % (alpha, eta)
            assert iters == 1 and len(trace) == 2, tag
            check_step(tag, gamma, lam, want, k, alpha, eta, ratios)
            for name in ("k_lda_tables", "k_lda_rows", "k_lda_topics", "k_lda_bound", "k_col_reduce"):
                assert name in names, (tag, name, sorted(names))
            assert "k_col_reduce_norm" not in names, sorted(names)
            assert names["k_lda_rows"][0] == 1 and names["k_lda_topics"][0] == 1 and names["k_lda_bound"][0] == 4, names
            # the trace is the bound before and after the step
            check_bound(tag + " before", trace[0], X, gamma0, lam0, k, alpha, eta, ratios)
            check_bound(tag + " after", trace[1], X, gamma, lam, k, alpha, eta, ratios)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [6, 130])
def test_one_step_through_the_row_items(amd, worst, k):
    """documents cut into row items of 16 entries (the 300-word document makes 19): N_d comes from k_row_reduce"""
    X, _, _ = corpus(k)
    alpha, eta = 0.1, 0.05
    gamma0, lam0 = start(k, alpha, eta)
    with make_engine(amd, {"PLSA_ROW_ITEMS": "1", "PLSA_ROW_SEG": "16"}, X) as eng:
        eng.timing(True)
        eng.set_factors(gamma0, lam0)
        eng.timing_reset()
        eng.lda_fit(alpha, eta, **ONE)
        assert "k_row_reduce" in eng.timing_report()
        gamma, lam = eng.get_factors()
        check_step("row items", gamma, lam, model_step(k, alpha, eta), k, alpha, eta, worst.setdefault(k, {}))


# ------------------------------------------------------------------------------------------------
# 3. doc_iter
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [6, 130])
def test_doc_iter_is_gamma_rounds_and_one_full_round(amd, worst, k):
    X, _, _ = corpus(k)
    alpha, eta = 0.1, 0.05
    gamma0, lam0 = start(k, alpha, eta)
    ratios = worst.setdefault(k, {})
    with make_engine(amd, {}, X) as eng:
        eng.set_factors(gamma0, lam0)
        gamma, stages = gamma0, {}
        for rounds in range(1, 4):                       # three gamma-only steps, each held to the model
            want = lm.lda_step64(X, gamma, lam0, alpha, eta, THRESH, update_v=False)
            iters, _ = eng.lda_refit(alpha, **ONE)
            gamma, lam = eng.get_factors()
            assert iters == 1
            check_step("gamma round %d" % rounds, gamma, lam, want, k, alpha, eta, ratios, topics=False)
            same_bits(lam, lam0, "a gamma-only round moved lambda")
            stages[rounds] = gamma
        full = {}
        for rounds in (2, 3):                            # ... and one full step behind two and behind three of them
            eng.set_factors(stages[rounds], lam0)
            want = lm.lda_step64(X, stages[rounds], lam0, alpha, eta, THRESH)
            eng.lda_fit(alpha, eta, **ONE)
            full[rounds] = eng.get_factors()
            check_step("full step behind %d gamma rounds" % rounds, full[rounds][0], full[rounds][1], want, k, alpha, eta, ratios)
        for doc_iter, rounds in ((3, 2), (4, 3)):
            eng.set_factors(gamma0, lam0)
            iters, trace = eng.lda_fit(alpha, eta, doc_iter=doc_iter, trace=True, **ONE)
            g, l = eng.get_factors()
            assert iters == 1 and len(trace) == 2
            same_bits(g, full[rounds][0], "doc_iter=%d: gamma" % doc_iter)
            same_bits(l, full[rounds][1], "doc_iter=%d: lambda" % doc_iter)
        # the refit's doc_iter: every iteration is that many gamma rounds
        eng.set_factors(gamma0, lam0)
        iters, _ = eng.lda_refit(alpha, doc_iter=3, **ONE)
        g, l = eng.get_factors()
        same_bits(g, stages[3], "refit with doc_iter=3: gamma")
        same_bits(l, lam0, "refit with doc_iter=3: lambda")


# ------------------------------------------------------------------------------------------------
# 4. the loop, one iteration at a time
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [6, 130])
def test_the_loop_is_the_step_iterated(amd, worst, k):
    X, _, _ = corpus(k)
    alpha, eta = 0.1, 0.05
    gamma0, lam0 = start(k, alpha, eta)
    ratios = worst.setdefault(k, {})
    loop = dict(tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED, trace=True)
    with make_engine(amd, {}, X) as eng:
        eng.set_factors(gamma0, lam0)
        gamma, lam, stages = gamma0, lam0, []
        for step in range(3):
            want = lm.lda_step64(X, gamma, lam, alpha, eta, THRESH)
            iters, trace = eng.lda_fit(alpha, eta, trace=True, **ONE)
            gamma, lam = eng.get_factors()
            check_step("loop step %d" % step, gamma, lam, want, k, alpha, eta, ratios)
            stages.append(trace)
        eng.set_factors(gamma0, lam0)
        iters, trace = eng.lda_fit(alpha, eta, n_iter=3, n_iter_per_test=1, **loop)
        g3, l3 = eng.get_factors()
        assert iters == 3 and len(trace) == 4
        same_bits(g3, gamma, "three iterations: gamma")
        same_bits(l3, lam, "three iterations: lambda")
        same_bits(trace, np.array([stages[0][0], stages[0][1], stages[1][1], stages[2][1]], np.float32), "trace")
        # a test every second iteration: the bound after iterations 0 and 2 only, the last one because it is traced
        eng.set_factors(gamma0, lam0)
        iters, sparse = eng.lda_fit(alpha, eta, n_iter=3, n_iter_per_test=2, **loop)
        assert iters == 3
        same_bits(sparse, trace[[0, 1, 3]], "trace with a test every second iteration")
        same_bits(eng.get_factors()[0], gamma, "a test every second iteration: gamma")


# ------------------------------------------------------------------------------------------------
# 5. the bound
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_bound_against_the_model(amd, worst, k):
    X, _, _ = corpus(k)
    ratios = worst.setdefault(k, {})
    with make_engine(amd, {}, X) as eng:
        for alpha, eta in priors(k):
            gamma0, lam0 = start(k, alpha, eta)
            eng.set_factors(gamma0, lam0)
            tag = "k=%d alpha=%g eta=%g" % (k, alpha, eta)
            check_bound(tag, eng.lda_bound(alpha, eta), X, gamma0, lam0, k, alpha, eta, ratios, float32=False)
            check_bound(tag + " without topics", eng.lda_bound(alpha), X, gamma0, lam0, k, alpha, None, ratios, float32=False)


@pytest.mark.gpu
def test_the_dirichlet_part_does_not_depend_on_the_launch_geometry(amd):
    """A corpus whose stored values are all 0 has a likelihood term of exactly 0, so the bound IS the Dirichlet part: a context
    capped at one workgroup per CU and a free one agree on it bit for bit (k = 1024: 163 840 and 122 880 float4s, more than a
    capped grid of 256 workgroups holds in one trip), and both are the model's within 2^-50 sum |terms|."""
    k = 1024
    X, _, _ = corpus(k)
    X0 = sp.csr_matrix((np.zeros_like(X.data), X.indices, X.indptr), shape=X.shape)
    pairs = priors(k)
    got = {}
    for capped in (True, False):
        with cap_knobs(CAP if capped else {}):
            eng = amd.Engine()
        with eng:
            eng.upload_csr(X0)
            got[capped] = []
            for alpha, eta in pairs:
                eng.set_factors(*start(k, alpha, eta))
                got[capped].append(eng.lda_bound(alpha, eta))
    for (alpha, eta), capped, free in zip(pairs, got[True], got[False]):
        assert np.float64(capped).view(np.uint64) == np.float64(free).view(np.uint64), (alpha, eta, capped, free)
        want, ll_scale, scale = lm.bound64(X0, *start(k, alpha, eta), alpha, eta)
        assert ll_scale == 0.0
        print("alpha=%g eta=%g: Dirichlet part %.6f, model %.6f, error / bound %.3g"
              % (alpha, eta, free, want, abs(free - want) / (2.0 ** -50 * scale)))
        assert abs(free - want) <= 2.0 ** -50 * scale, (alpha, eta, free, want)


# ------------------------------------------------------------------------------------------------
# 6. the bound never decreases
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_monotone_bound(amd):
    """Planted corpus of tests/lda_model.py at (alpha, eta) = (0.1, 0.01), tolerance 0, a test after every one of 30
    iterations: every value of the trace is at least its predecessor minus lda_model.monotone_bound.  The float64 model
    (test_lda_model_host.py): L rises from -202 690.4 to -132 382.4, its smallest increase is 13.03 against a bound of 0.112 --
    a margin of 116."""
    X, _, gamma0, lam0 = lm.planted()
    alpha, eta = lm.PRIORS
    L, ll_scales, scales = lm.planted_trace()
    k = sm.PLANTED["topics"]
    bound = max(lm.monotone_bound(k, X.sum(), a, b, f) for a, b, f in zip(ll_scales, scales, L))
    assert np.diff(L).min() >= 10 * bound
    with make_engine(amd, {}, X) as eng:
        eng.set_factors(gamma0, lam0)
        iters, trace = eng.lda_fit(alpha, eta, n_iter=30, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH,
                                   flags=PLSA_FUSED, trace=True)
    assert iters == 30 and len(trace) == 31
    trace = trace.astype(np.float64)
    print("\nplanted corpus on the device: L %.1f -> %.1f, smallest increase %.3f (model %.3f), bound %.3f"
          % (trace[0], trace[-1], np.diff(trace).min(), np.diff(L).min(), bound))
    assert (np.diff(trace) >= -bound).all(), np.diff(trace).min()
    assert abs(trace[0] - L[0]) <= bound


# ------------------------------------------------------------------------------------------------
# 7. the refit
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_one_refit_step_against_the_model(amd, worst, k):
    X, _, _ = corpus(k)
    ratios = worst.setdefault(k, {})
    with make_engine(amd, {}, X) as eng:
        eng.timing(True)
        for alpha, eta in priors(k):
            gamma0, lam0 = start(k, alpha, eta)
            want = lm.lda_step64(X, gamma0, lam0, alpha, eta, THRESH, update_v=False)
            eng.set_factors(gamma0, lam0)
            eng.timing_reset()
            iters, trace = eng.lda_refit(alpha, trace=True, **ONE)
            names = eng.timing_report()
            gamma, lam = eng.get_factors()
            assert iters == 1 and len(trace) == 2
            check_step("refit alpha=%g" % alpha, gamma, lam, want, k, alpha, eta, ratios, topics=False)
            same_bits(lam, lam0, "the refit wrote lambda")
            assert "k_lda_rows" in names and "k_lda_topics" not in names, sorted(names)
            assert not [name for name in names if name.startswith("k_col")], sorted(names)
            check_bound("refit alpha=%g after" % alpha, trace[1], X, gamma, lam0, k, alpha, None, ratios)


# ------------------------------------------------------------------------------------------------
# 8. capped grids
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_capped_grid_computes_the_same_bits(amd):
    """k = 6 (kq = 2, pads in the second quarter).  n and m come from the CU count as in test_capped_grids.sizes: under
    PLSA_GRID_MULT=1 k_lda_tables and k_lda_rows (n kq float4s), k_lda_tables and k_lda_topics (m kq) and k_lda_rowsum (n rows,
    128 per workgroup) make three trips at least with a ragged last one."""
    k, kq = 6, 2
    with amd.Engine() as probe:
        cus = probe.device_info()["cus"]
    n, m = sizes(k, cus)
    for count in (n, m):
        assert count * kq > 2 * cus * 256 and (count * kq) % (cus * 256) != 0, (count, cus)
    assert n > 2 * cus * 128 and n % (cus * 128) != 0, (n, cus)
    rs = np.random.RandomState(12)
    per_doc = 3
    rows = np.repeat(np.arange(n), per_doc)
    rows[:per_doc] = 1                                    # document 0 is empty
    cols = rs.randint(0, m, size=rows.shape[0])
    cols[-m:] = np.arange(m)                              # every word occurs
    X = sp.csr_matrix((rs.randint(1, 5, size=rows.shape[0]).astype(np.float32), (rows, cols)), shape=(n, m))
    X.sum_duplicates()
    alpha, eta = 0.1, 0.05
    gamma0 = (alpha + rs.gamma(1.0, 2.0, (n, k))).astype(np.float32)
    lam0 = (eta + rs.gamma(1.0, 2.0, (k, m))).astype(np.float32)
    got = {}
    for capped in (True, False):
        with cap_knobs(CAP if capped else {}):
            eng = amd.Engine()
        with eng:
            eng.upload_csr(X)
            eng.set_factors(gamma0, lam0)
            tables = eng.lda_tables()
            iters, trace = eng.lda_fit(alpha, eta, trace=True, **ONE)
            got[capped] = tables + eng.get_factors() + (trace,)
    for name, a, b in zip(("A", "B", "gamma", "lambda", "trace"), got[True], got[False]):
        same_bits(a, b, "capped: " + name)
    A, B, gamma, lam, _ = got[True]
    A64, B64 = lm.tables64(gamma0, lam0)
    check("A (capped)", A, A64, T_BOUND)
    check("B (capped)", B, B64, T_BOUND)
    np.testing.assert_allclose(gamma[0], alpha, rtol=U32)
    assert (gamma > 0).all() and (lam > 0).all()
    # the counts add up: every token is in gamma once and in lambda once
    tokens = float(X.sum())
    assert abs(gamma.astype(np.float64).sum() - n * k * alpha - tokens) <= 1e-5 * tokens
    assert abs(lam.astype(np.float64).sum() - m * k * eta - tokens) <= 1e-5 * tokens


# ------------------------------------------------------------------------------------------------
# 9. refusals
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_launch_nothing_and_leave_the_state(amd):
    k = 21
    X, _, _ = corpus(k)
    gamma0, lam0 = start(k, 0.1, 0.05)
    kw = dict(n_iter=2, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH)
    nan, inf = float("nan"), float("inf")
    with make_engine(amd, {}, X) as eng:
        eng.set_factors(gamma0, lam0)
        eng.timing(True)
        eng.timing_reset()
        bad = [(0.1, 0.05, 1, 0, "PLSA_FUSED"), (0.1, 0.05, 1, PLSA_FUSED | PLSA_SHARDED, "PLSA_SHARDED"),
               (0.1, 0.05, 1, PLSA_FUSED | PLSA_GRAPH, "PLSA_GRAPH"),
               (0.1, 0.05, 1, PLSA_FUSED | PLSA_REFERENCE_SUMS, "PLSA_REFERENCE_SUMS"),
               (0.1, 0.05, 1, PLSA_FUSED | PLSA_REFERENCE_LL, "PLSA_REFERENCE_LL"),
               (0.0, 0.05, 1, PLSA_FUSED, "alpha="), (-0.1, 0.05, 1, PLSA_FUSED, "alpha="), (nan, 0.05, 1, PLSA_FUSED, "alpha="),
               (inf, 0.05, 1, PLSA_FUSED, "alpha="), (0.1, 0.0, 1, PLSA_FUSED, "eta="), (0.1, -1.0, 1, PLSA_FUSED, "eta="),
               (0.1, nan, 1, PLSA_FUSED, "eta="), (0.1, inf, 1, PLSA_FUSED, "eta="),
               (0.1, 0.05, 0, PLSA_FUSED, "doc_iter"), (0.1, 0.05, -2, PLSA_FUSED, "doc_iter")]
        for alpha, eta, doc_iter, flags, word in bad:
            with pytest.raises(amd.DeviceError, match=word):
                eng.lda_fit(alpha, eta, doc_iter=doc_iter, flags=flags, **kw)
            if word != "eta=":
                with pytest.raises(amd.DeviceError, match=word):
                    eng.lda_refit(alpha, doc_iter=doc_iter, flags=flags, **kw)
            if word in ("alpha=", "eta="):
                with pytest.raises(amd.DeviceError, match=word):
                    eng.lda_bound(alpha, eta)
        for arithmetic in ("reference", "reference_source"):
            eng.set_arithmetic(arithmetic)
            with pytest.raises(amd.DeviceError, match="reference arithmetic"):
                eng.lda_fit(0.1, 0.05, flags=PLSA_FUSED, **kw)
            with pytest.raises(amd.DeviceError, match="reference arithmetic"):
                eng.lda_refit(0.1, flags=PLSA_FUSED, **kw)
            with pytest.raises(amd.DeviceError, match="reference arithmetic"):
                eng.lda_bound(0.1, 0.05)
            with pytest.raises(amd.DeviceError, match="reference arithmetic"):
                eng.lda_tables()
        eng.set_arithmetic(None)
        assert eng.timing_report() == {}, eng.timing_report()        # nothing was launched
        g, l = eng.get_factors()
        same_bits(g, gamma0, "a refusal moved gamma")
        same_bits(l, lam0, "a refusal moved lambda")
        iters, _ = eng.lda_fit(0.1, 0.05, flags=PLSA_FUSED, **kw)
        names = eng.timing_report()
        assert iters == 2 and names["k_lda_rows"][0] == 2 and names["k_lda_topics"][0] == 2
        first = eng.get_factors()
        # the scratch goes with release_scratch and comes back with the next call
        eng.release_scratch()
        eng.set_factors(gamma0, lam0)
        iters, _ = eng.lda_fit(0.1, 0.05, flags=PLSA_FUSED, **kw)
        assert iters == 2
        same_bits(eng.get_factors()[0], first[0], "after release_scratch: gamma")
        same_bits(eng.get_factors()[1], first[1], "after release_scratch: lambda")


def test_the_python_refusals_come_before_any_engine(monkeypatch):
    import enstop_amd
    from enstop_amd import engine, lda, plsa

    def no_engine(*args, **kwargs):
        raise AssertionError("an engine was asked for")
    for module in (engine, lda, plsa):
        monkeypatch.setattr(module, "get_engine", no_engine)
    X = sp.random(12, 9, density=0.5, format="csr", random_state=0, dtype=np.float32)
    nan = float("nan")
    for kw in (dict(doc_topic_prior=0.0), dict(doc_topic_prior=-0.1), dict(topic_word_prior=nan), dict(topic_word_prior=float("inf")),
               dict(doc_topic_prior="sparse"), dict(topic_word_prior=True), dict(doc_iter=0), dict(doc_iter=1.5), dict(n_iter=-1),
               dict(n_iter_per_test=0), dict(tolerance=-1.0), dict(init="nndsvd"), dict(init=(np.ones((12, 3)), np.ones((3, 8)))),
               dict(init=(np.zeros((12, 3)), np.ones((3, 9))))):
        with pytest.raises(ValueError):
            enstop_amd.lda_fit(X, 3, **kw)
        if "init" not in kw:
            with pytest.raises(ValueError):
                enstop_amd.LDA(n_components=3, **kw).fit(X)
    for k in (0, 1025, 2.5):
        with pytest.raises(ValueError):
            enstop_amd.lda_fit(X, k)
    with pytest.raises(ValueError):
        enstop_amd.lda_fit(-X, 3)
    lam = np.ones((3, 9), np.float32)
    for args, kw in (((X, lam, 0.0), {}), ((X, lam[:, :8], 0.1), {}), ((X, -lam, 0.1), {}),
                     ((X, lam, 0.1), dict(doc_iter=0)), ((X, lam[0], 0.1), {})):
        with pytest.raises(ValueError):
            enstop_amd.lda_transform(*args, **kw)


@pytest.mark.gpu
def test_a_shard_of_a_communicator_is_refused(amd, tmp_path):
    from enstop_amd import comm
    k = 21
    X, _, _ = corpus(k)
    gamma0, lam0 = start(k, 0.1, 0.05)
    kw = dict(n_iter=2, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED)
    with make_engine(amd, {}, X) as eng:
        eng.set_factors(gamma0, lam0)
        c = comm.RcclComm(eng, 0, 1, comm.rendezvous_id(0, str(tmp_path / "rccl.id")))
        try:
            assert eng.comm_info() == (0, 1)
            eng.timing(True)
            eng.timing_reset()
            with pytest.raises(amd.DeviceError, match="communicator"):
                eng.lda_fit(0.1, 0.05, **kw)
            with pytest.raises(amd.DeviceError, match="communicator"):
                eng.lda_refit(0.1, **kw)
            with pytest.raises(amd.DeviceError, match="communicator"):
                eng.lda_bound(0.1, 0.05)
            with pytest.raises(amd.DeviceError, match="communicator"):
                eng.lda_tables()
            assert eng.timing_report() == {}, eng.timing_report()        # nothing was launched
            g, l = eng.get_factors()
            same_bits(g, gamma0, "a refusal moved gamma")
            same_bits(l, lam0, "a refusal moved lambda")
        finally:
            c.close()
        iters, _ = eng.lda_fit(0.1, 0.05, **kw)
        assert iters == 2 and eng.timing_report()["k_lda_rows"][0] == 2


# ------------------------------------------------------------------------------------------------
# 10. what it is for
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sparse_priors_and_unseen_words(amd):
    X, X_test, _, _ = lm.planted()
    alpha, eta = lm.PRIORS
    k = 8
    with pytest.raises(ValueError):                       # the gap: MAP EM cannot express a concentration below 1
        amd.PLSA(n_components=k, doc_topic_smoothing=alpha - 1).fit(X)
    plain = amd.PLSA(n_components=k, random_state=0).fit(X)
    assert amd.held_out_scores(X_test, plain.components_, method="completion")["unscored"].sum() > 0
    model = amd.LDA(n_components=k, doc_topic_prior=alpha, topic_word_prior=eta, random_state=0).fit(X)
    assert model.components_.shape == (k, X.shape[1]) and (model.components_ > 0).all()
    assert model.embedding_.shape == (X.shape[0], k) and (model.embedding_ > 0).all()
    assert np.abs(model.topic_word_.astype(np.float64).sum(1) - 1).max() <= (X.shape[1] + 5) * U32
    assert amd.held_out_scores(X_test, model.topic_word_, method="completion")["unscored"].sum() == 0
    p = model.perplexity(X_test)
    assert np.isfinite(p) and p > 1
    held_out = model.held_out_perplexity(X_test)
    assert np.isfinite(held_out) and held_out > 1
    trace = model.bound_trace_.astype(np.float64)
    assert len(trace) >= 2 and (np.diff(trace) > 0).all() and model.bound_ == trace[-1] and model.n_iter_ >= 10
    again = amd.LDA(n_components=k, doc_topic_prior=alpha, topic_word_prior=eta, random_state=0).fit(X)
    same_bits(again.components_, model.components_, "two fits with one seed: lambda")
    same_bits(again.embedding_, model.embedding_, "two fits with one seed: gamma")
    # the fold-in: strictly positive document vectors, rows that sum to 1
    T = model.transform(X_test)
    assert T.shape == (X_test.shape[0], k) and (T > 0).all() and np.abs(T.astype(np.float64).sum(1) - 1).max() <= (k + 5) * U32
    # the functions
    gamma, lam, info = amd.lda_fit(X, k, alpha, eta, n_iter=20, random_state=0, return_info=True)
    assert (gamma > 0).all() and (lam > 0).all() and info["n_iter"] == 20 and len(info["bound_trace"]) == 3
    folded = amd.lda_transform(X_test, lam, alpha, random_state=1)
    assert folded.shape == (X_test.shape[0], k) and (folded > 0).all()
    # beside scikit-learn from the same seed (not asserted: two local optima)
    from sklearn.decomposition import LatentDirichletAllocation
    theirs = LatentDirichletAllocation(n_components=k, doc_topic_prior=alpha, topic_word_prior=eta, max_iter=model.n_iter_,
                                       learning_method="batch", random_state=0).fit(X)
    tokens = X.sum()
    print("\nplanted corpus: per-token bound %.4f after %d iterations (scikit-learn's batch fit, same seed and sweeps: %.4f); "
          "perplexity of the test half %.1f (scikit-learn %.1f), held-out completion perplexity %.1f"
          % (model.bound_ / tokens, model.n_iter_, theirs.score(X) / tokens, p, theirs.perplexity(X_test), held_out))
