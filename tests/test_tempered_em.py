"""Tempered EM on the device (include/plsa_hip_tempered.h, enstop_amd/tempered.py): the side tables, one tempered step against
the ordinary step on those tables and against float64, the loop, the snapshot slot, the refusals, and the held-out schedule end
to end on a planted corpus.

A tempered iteration raises the factors to the power beta into two side tables and runs the ordinary fused iteration on them,
so everything below the tables is held to BITS: a tempered step is `fit(n_iter=1)` from the downloaded tables (B), N
iterations are N single steps through the host (F), beta = 1 is plsa_fit (E).  Only the tables themselves (A) and the float64
restatement (D) have tolerances, and both are derived:

A.  out = (float)pow((double)x, beta).  A float64 pow good to a few float64 ulp lies within a few 2^-53 (relative) of the
    exact power; so does NumPy's.  Rounding two such values to float32 gives the same float32 or two neighbours: at most 1
    float32 ulp apart, in the normal and in the denormal range (where the ulp is 2^-149).

D.  The restatement (test_pass_matrix.step64) is run on float32(np.power(float64(x), beta)), the device on tables whose
    entries are each within 1 ulp <= 2u of those (u = 2^-24, A).  A product of two table entries is then off by at most
    (1 + 2u)^2 - 1 <= 4u (1 + u) relative.  A responsibility is a product over the sum of its row's k products, all
    positive: (1 + a) / (1 + b) with |a|, |b| <= 4u (1 + u), at most 8u (1 + 7u) from the restatement's.  An updated factor
    entry is a sum of x * responsibility over its row (column) divided by the sum of k (m k) such sums, all positive, each
    term within 8u (1 + 7u): at most 16u (1 + 17u) < 16.001u.  This comes on top of the matrix's own bound 4 (L + k) u for
    the step's float32 arithmetic; the cross term 4 (L + k) u * 16.001u is below 0.01u for L + k < 2^13.  So

        |got - want| <= (4 (L + k) + 17) 2^-24 |want|,   zeros of want exact zeros of got

    with L the longest row (P(z|d)) or column (P(w|z)).  No threshold decision can differ: with thresh = 1e-32 every
    tempered product of the matrix is either above 1e-24 or (the tiny block, 2^-126 and below) thresholded away.

Needs a real MI355X, except for the conditions on the planted corpus.
"""
import contextlib
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

from test_fit_driver import PLSA_FUSED, PLSA_GRAPH, PLSA_SHARDED, PLSA_SW_LL_ONLY, bits, reference_loop, same_bits
from test_pass_matrix import (C_FACTOR, K_MATRIX, SETTINGS, U32, _coo, check, check_ll, lane_shape, loglik64, matrix_corpus,
                              products32, step64)

PLSA_REFERENCE_SUMS, PLSA_REFERENCE_LL = 256, 512
THRESH = 1e-32
BETAS = (0.5, 0.9, 0.999)
BETA = 0.9
KNOBS = sorted({key for env in SETTINGS.values() for key in env} |
               {"PLSA_SORT_ROWS", "PLSA_SPECULATE", "PLSA_PIPELINE", "PLSA_OVERLAP", "PLSA_GRAPH", "PLSA_BALANCE", "PLSA_XCD_SPLIT"})
CONTEXTS = dict({name: SETTINGS[name] for name in ("default", "wide", "arrays", "row_items")}, unsorted={"PLSA_SORT_ROWS": "0"})
FLT_MIN = np.float32(2.0 ** -126)


def _shape_ks():
    """one topic count per lane shape of the passes, and k = 64 (where the fused document pass runs 8 x 2)"""
    seen, ks = set(), []
    for k in K_MATRIX:
        shape = lane_shape(k)[1]
        if shape not in seen:
            seen.add(shape)
            ks.append(k)
    assert len(seen) == 9
    return sorted(set(ks) | {64})


K_SHAPES = _shape_ks()


@contextlib.contextmanager
def knobs(env):
    saved = {key: os.environ.get(key) for key in KNOBS}
    try:
        for key in KNOBS:
            os.environ.pop(key, None)
        os.environ.update(env)
        yield
    finally:
        for key, value in saved.items():
            if value is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = value


def make_engine(amd, env, X):
    with knobs(env):
        eng = amd.Engine()
    eng.upload_csr(X)
    return eng


@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


@functools.lru_cache(maxsize=None)
def special_factors(k):
    """matrix_corpus(k)'s factors with the values a power has to get right planted in them: a one-hot row (exact zeros and
    1.0), a word no topic gives mass, FLT_MIN and its neighbours on both sides, the largest and the smallest denormal and a
    few in between"""
    X, U, V, sw = matrix_corpus(k)
    U, V = U.copy(), V.copy()
    U[20] = 0.0
    U[20, 0] = 1.0
    V[:, 30] = 0.0
    V[0, 31] = 1.0
    edge = np.array([FLT_MIN, np.nextafter(FLT_MIN, np.float32(1)), np.nextafter(FLT_MIN, np.float32(0)), 2.0 ** -149,
                     3 * 2.0 ** -149, 2.0 ** -140, 2.0 ** -127, 1.5 * 2.0 ** -126], np.float32)
    assert (edge[2:7] < FLT_MIN).all() and (edge > 0).all()
    for i, v in enumerate(edge):
        U[21 + i, i % k] = v
        V[i % k, 40 + i] = v
    return X, U, V, sw


def ulp_distance(a, b):
    """distance in float32 representations between non-negative float32 arrays (denormals included: spacing 2^-149)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert (a >= 0).all() and (b >= 0).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def power32(x, beta):
    return np.power(np.asarray(x, np.float32).astype(np.float64), beta).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# A. the side tables
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K_MATRIX)
def test_side_tables_are_within_one_ulp_of_the_rounded_power(amd, k):
    X, U0, V0, _ = special_factors(k)
    worst = 0
    with make_engine(amd, {}, X) as eng:
        eng.set_factors(U0, V0)
        eng.timing(True)
        for beta in BETAS:
            TU, TV = eng.temper_factors(beta)
            for name, got, x in (("U", TU, U0), ("V", TV, V0)):
                want = power32(x, beta)
                assert got.dtype == np.float32 and got.shape == x.shape
                same_bits(got[x == 0], np.zeros(int((x == 0).sum()), np.float32), "k=%d beta=%g %s: zeros" % (k, beta, name))
                assert (got[x > 0] > 0).all(), (k, beta, name)               # nothing positive is flushed
                d = ulp_distance(got, want)
                assert d.max() <= 1, "k=%d beta=%g %s: %d ulp at %r" % (k, beta, name, d.max(), np.unravel_index(d.argmax(), d.shape))
                worst = max(worst, int(d.max()))
                same_bits(got[x == 1], np.ones(int((x == 1).sum()), np.float32), "%s: 1.0" % name)
            if beta == 0.999:                                                # denormal in, denormal out
                assert 0 < TU[24, 3 % k] < FLT_MIN and 0 < TV[3 % k, 43] < FLT_MIN
            U1, V1 = eng.get_factors()
            same_bits(U1, U0, "k=%d beta=%g: temper_factors moved U" % (k, beta))
            same_bits(V1, V0, "k=%d beta=%g: temper_factors moved V" % (k, beta))
        assert eng.timing_report()["k_temper"][0] == 2 * len(BETAS)
    print("\nk=%d: side tables at most %d ulp from float32(np.power(float64(x), beta))" % (k, worst))


# ------------------------------------------------------------------------------------------------
# B, C, D. one tempered step
# ------------------------------------------------------------------------------------------------
def tempered_step(eng, U0, V0, sw, beta=BETA):
    eng.set_factors(U0, V0)
    iters, trace = eng.fit_tempered(beta, sw, n_iter=1, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED,
                                    trace=True)
    assert iters == 1 and trace.shape == (2,), (iters, trace)
    return eng.get_factors(), trace


def ordinary_step_on(eng, TU, TV, sw):
    eng.set_factors(TU, TV)
    iters, trace = eng.fit(sw, n_iter=1, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED)
    assert iters == 1 and trace.shape == (1,)
    return eng.get_factors(), trace


@pytest.mark.gpu
@pytest.mark.parametrize("k", K_MATRIX)
def test_a_tempered_step_is_the_ordinary_step_on_the_tempered_tables(amd, k):
    """B at every k, C and D with them: the factors in bits, the trace against k_loglik and float64, the step against step64"""
    X, U0, V0, sw_doc = matrix_corpus(k)
    rows, cols, x = _coo(X)
    ratios = {}
    one, two = make_engine(amd, {}, X), make_engine(amd, {}, X)
    try:
        for sw in (None, sw_doc):
            tag = "k=%d sw=%d" % (k, sw is not None)
            one.set_factors(U0, V0)
            ll0 = one.log_likelihood(sw)
            TU, TV = one.temper_factors(BETA)
            one.timing(True)
            one.timing_reset()
            (U1, V1), trace = tempered_step(one, U0, V0, sw)
            names = one.timing_report()
            one.timing(False)
            (U2, V2), riding = ordinary_step_on(two, TU, TV, sw)
            # B
            same_bits(U1, U2, tag + ": U")
            same_bits(V1, V2, tag + ": V")
            # the launch chain: two tables, the plain passes, no riding likelihood, two k_loglik
            assert names["k_temper"][0] == 2 and names["k_loglik"][0] == 2, (tag, names)
            assert "k_row_pass<fused>" in names and "k_col_pass<fused>" in names and "k_col_reduce_norm" in names, (tag, names)
            assert "k_row_pass<fused,LL>" not in names, (tag, names)
            info = one.fit_info()
            assert info["fused"] and not info["pipelined"] and not info["speculated"] and not info["graph_launches"], info
            # C: the trace holds the likelihoods of the TRUE factors
            ll1 = one.log_likelihood(sw)
            same_bits(trace, np.array([ll0, ll1], np.float32), tag + ": trace")
            want_ll, scale = loglik64(rows, cols, x, U1, V1, sw)
            check_ll("LL " + tag, ll1, want_ll, scale, k, ratios)
            assert bits(riding)[0] not in set(bits(trace)), (tag, "the tempered dot's likelihood is in the trace", riding, trace)
            # D: float64 on the rounded float64 powers
            ref = step64(X, power32(U0, BETA).astype(np.float64), power32(V0, BETA).astype(np.float64), THRESH, sw)
            extra = 17.0 * U32
            check("U " + tag, U1, ref["U"], C_FACTOR * (ref["L_row"] + k) * U32 + extra, ratios)
            check("V " + tag, V1, ref["V"], C_FACTOR * (ref["L_col"] + k) * U32 + extra, ratios)
    finally:
        one.close()
        two.close()
    print("\nk=%d: tempered step, worst error / bound: %s" % (k, ", ".join("%s %.3g" % (q, v) for q, v in sorted(ratios.items()))))


@pytest.mark.gpu
@pytest.mark.parametrize("k", K_SHAPES)
def test_the_step_is_the_same_step_under_every_context_and_with_planted_values(amd, k):
    """B at one k per lane shape under the contexts default, wide, arrays, row_items and PLSA_SORT_ROWS=0, once with sample
    weights, from factors that hold exact zeros, 1.0, FLT_MIN's neighbours and denormals"""
    X, U0, V0, sw_doc = special_factors(k)
    for name, env in CONTEXTS.items():
        one, two = make_engine(amd, env, X), make_engine(amd, env, X)
        try:
            for sw in ((None, sw_doc) if name == "default" else (None,)):
                tag = "k=%d %s sw=%d" % (k, name, sw is not None)
                one.set_factors(U0, V0)
                TU, TV = one.temper_factors(BETA)
                (U1, V1), _ = tempered_step(one, U0, V0, sw)
                (U2, V2), _ = ordinary_step_on(two, TU, TV, sw)
                same_bits(U1, U2, tag + ": U")
                same_bits(V1, V2, tag + ": V")
                assert np.isfinite(U1).all() and np.isfinite(V1).all(), tag
            info = one.pass_info()
            assert info["row_wide"] == info["col_wide"] == (name == "wide"), (name, info)
            if name != "row_items":
                assert one.packed_info()["csr"] == ("arrays" if name == "arrays" else "packed"), name
        finally:
            one.close()
            two.close()


# ------------------------------------------------------------------------------------------------
# E. beta = 1 is plsa_fit
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_beta_one_is_plsa_fit(amd):
    from conftest import golden_csr, load_golden
    from enstop_amd.plsa import plsa_init
    g = load_golden("fit_k5_earlystop")
    Xg, kg = golden_csr(g), int(g["k"])
    Ug, Vg = plsa_init(Xg, kg, "random", np.random.RandomState(int(g["fit_seed"])))
    early = (Xg, Ug.astype(np.float32), Vg.astype(np.float32), g["sw"].astype(np.float32),
             int(g["n_iter"]), int(g["n_iter_per_test"]), float(g["tol"]), float(g["thresh"]))
    X, U0, V0, sw = matrix_corpus(64)
    cases = [(X, U0, V0, None, 7, 3, 0.0, THRESH), (X, U0, V0, sw, 12, 5, 1e-9, THRESH), early]
    for X, U0, V0, sw, n_iter, per_test, tol, thresh in cases:
        tag = "n_iter=%d per_test=%d tol=%g" % (n_iter, per_test, tol)
        with make_engine(amd, {}, X) as eng:
            eng.set_factors(U0, V0)
            it_a, tr_a = eng.fit(sw, n_iter, per_test, tol, thresh, PLSA_FUSED, trace=True)
            Ua, Va = eng.get_factors()
            eng.set_factors(U0, V0)
            eng.timing(True)
            it_b, tr_b = eng.fit_tempered(1.0, sw, n_iter, per_test, tol, thresh, PLSA_FUSED, trace=True)
            Ub, Vb = eng.get_factors()
            assert "k_temper" not in eng.timing_report(), tag
        assert it_a == it_b, tag
        same_bits(tr_a, tr_b, tag + ": trace")
        same_bits(Ua, Ub, tag + ": U")
        same_bits(Va, Vb, tag + ": V")
        if X is Xg:
            assert it_a == int(g["iters"]) < n_iter, (tag, it_a)       # the run that stops early


# ------------------------------------------------------------------------------------------------
# F. the loop
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [6, 64])
def test_the_loop_is_the_step_iterated(amd, k):
    X, U0, V0, sw = matrix_corpus(k)
    beta, n_max = 0.8, 7
    eng = make_engine(amd, {}, X)
    try:
        S, kll = [(U0, V0)], []
        for i in range(n_max):                       # single steps through the host
            eng.set_factors(*S[i])
            kll.append(eng.log_likelihood(sw))
            iters, _ = eng.fit_tempered(beta, sw, n_iter=1, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED)
            assert iters == 1
            S.append(eng.get_factors())
        eng.set_factors(*S[n_max])
        kll.append(eng.log_likelihood(sw))
        trail = [np.float32(v) for v in kll]
        for n_iter, per_test in ((1, 1), (5, 2), (7, 10)):
            tag = "k=%d N=%d per_test=%d" % (k, n_iter, per_test)
            eng.set_factors(U0, V0)
            iters, trace = eng.fit_tempered(beta, sw, n_iter, per_test, 0.0, THRESH, PLSA_FUSED, trace=True)
            assert iters == n_iter, tag
            U, V = eng.get_factors()
            same_bits(U, S[n_iter][0], tag + ": U")
            same_bits(V, S[n_iter][1], tag + ": V")
            # every likelihood is k_loglik's: the reference loop with the same values riding and trailing
            want_iters, want_trace = reference_loop(n_iter, per_test, 0.0, trail, trail, stops=False)
            assert want_iters == n_iter and len(want_trace) == 1 + len([i for i in range(n_iter) if i % per_test == 0]), tag
            same_bits(trace, np.asarray(want_trace, np.float32), tag + ": trace")
            assert np.float64(eng.log_likelihood(sw)).view(np.uint64) == np.float64(kll[n_iter]).view(np.uint64), tag
            # without the trace flag the test of the last iteration is not evaluated: same factors
            eng.set_factors(U0, V0)
            iters, short = eng.fit_tempered(beta, sw, n_iter, per_test, 0.0, THRESH, PLSA_FUSED)
            last_tested = (n_iter - 1) % per_test == 0
            same_bits(short, np.asarray(want_trace[:len(want_trace) - (1 if last_tested else 0)], np.float32), tag + ": untraced")
            same_bits(eng.get_factors()[0], S[n_iter][0], tag + ": U untraced")
    finally:
        eng.close()


@pytest.mark.gpu
def test_fixed_beta_fit_is_the_initialisation_followed_by_the_tempered_loop(amd):
    """plsa_fit_fixed_beta puts plsa_fit's starting factors on the device (_driver.init_factors) and runs fit_tempered: no
    zero-iteration fit stands between the two, and none is missed -- the same two calls on an engine of one's own give the
    same bits."""
    from enstop_amd._driver import init_factors
    from enstop_amd.engine import default_flags
    from enstop_amd.tempered import plsa_fit_fixed_beta
    rs = np.random.RandomState(5)
    dense = np.ceil(rs.rand(6, 9) * 4) * (rs.rand(6, 9) < 0.3)
    dense[np.arange(9) % 6, np.arange(9)] += 1.0                   # no empty document, no empty word
    X = sp.csr_matrix(dense.astype(np.float32))
    assert X.shape == (6, 9) and 15 <= X.nnz <= 25
    seed = 11
    U, V, info = plsa_fit_fixed_beta(X, 3, 0.8, random_state=seed, n_iter=4, n_iter_per_test=2)
    with make_engine(amd, {}, X) as eng:
        init_factors(eng, 3, "random", np.random.RandomState(seed), X)
        iters, trace = eng.fit_tempered(0.8, None, 4, 2, 0.001, 1e-32, default_flags(), trace=True)
        Ue, Ve = eng.get_factors()
    assert info["n_iter"] == iters and iters >= 1
    same_bits(info["log_likelihood_trace"], trace, "trace")
    same_bits(U, Ue, "U")
    same_bits(V, Ve, "V")


# ------------------------------------------------------------------------------------------------
# G. snapshot / restore
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_snapshot_and_restore(amd):
    k = 64
    X, U0, V0, sw = matrix_corpus(k)
    held = sp.csr_matrix(X.multiply(X > 2).astype(np.float32))
    held.eliminate_zeros()
    eng, plain = make_engine(amd, {}, X), make_engine(amd, {}, X)
    try:
        with pytest.raises(amd.DeviceError, match="no snapshot"):
            eng.restore_factors()
        eng.set_factors(U0, V0)
        with pytest.raises(amd.DeviceError, match="no snapshot"):
            eng.restore_factors()
        (U1, V1), _ = tempered_step(eng, U0, V0, sw)             # S1
        eng.snapshot_factors()
        (U2, V2), _ = tempered_step(eng, U1, V1, sw)             # S2 (set_factors(S1) inside: the snapshot is not the live buffers)
        eng.fit_tempered(BETA, sw, n_iter=3, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED)
        eng.restore_factors()
        Ur, Vr = eng.get_factors()
        same_bits(Ur, U1, "restore: U")
        same_bits(Vr, V1, "restore: V")
        iters, _ = eng.fit_tempered(BETA, sw, n_iter=1, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED)
        Ua, Va = eng.get_factors()
        same_bits(Ua, U2, "a step after restore: U")
        same_bits(Va, V2, "a step after restore: V")
        eng.restore_factors()                                     # the slot keeps the snapshot
        same_bits(eng.get_factors()[0], U1, "second restore")
        # afterwards the context is what a context that never tempered is
        plain.set_factors(U1, V1)
        for e in (eng, plain):
            e.out = dict(score=e.score_rows(held, sw), fit=e.fit(sw, 4, 2, 0.0, THRESH, PLSA_FUSED, trace=True), fit_uv=e.get_factors(),
                         refit=e.refit(sw, 3, 1, 0.0, THRESH, PLSA_FUSED, trace=True), refit_uv=e.get_factors(),
                         pass_info=e.pass_info(), packed_info=e.packed_info(), shape=e.shape)
        a, b = eng.out, plain.out
        for i in range(3):
            same_bits(a["score"][i], b["score"][i], "score_rows after tempering: %d" % i)
        for key in ("fit", "refit"):
            assert a[key][0] == b[key][0], key
            same_bits(a[key][1], b[key][1], key + " trace")
            same_bits(a[key + "_uv"][0], b[key + "_uv"][0], key + " U")
            same_bits(a[key + "_uv"][1], b[key + "_uv"][1], key + " V")
        assert a["pass_info"] == b["pass_info"] and a["packed_info"] == b["packed_info"] and a["shape"] == b["shape"]
        # release_scratch frees the side tables and the slot; the next tempered call works and gives the same bits
        eng.release_scratch()
        with pytest.raises(amd.DeviceError, match="no snapshot"):
            eng.restore_factors()
        (Ub, Vb), _ = tempered_step(eng, U1, V1, sw)
        same_bits(Ub, U2, "after release_scratch: U")
        same_bits(Vb, V2, "after release_scratch: V")
        # another k: the snapshot is refused, by name
        eng.snapshot_factors()
        Xs, Us, Vs, _ = matrix_corpus(6)
        eng.set_factors(Us, Vs)
        with pytest.raises(amd.DeviceError, match="k=64.*k=6"):
            eng.restore_factors()
        same_bits(eng.get_factors()[0], Us, "a refused restore moved U")
        # another shape
        eng.snapshot_factors()
        eng.upload_csr(X[:100])
        eng.set_factors(Us[:100], Vs)
        with pytest.raises(amd.DeviceError, match="640 x 480.*100 x 480"):
            eng.restore_factors()
    finally:
        eng.close()
        plain.close()


# ------------------------------------------------------------------------------------------------
# H. refusals
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_launch_nothing_and_leave_the_factors(amd):
    k = 16
    X, U0, V0, sw = matrix_corpus(k)
    with make_engine(amd, {}, X) as eng:
        eng.set_factors(U0, V0)
        eng.timing(True)
        eng.timing_reset()
        bad = [(BETA, 0, "PLSA_FUSED"), (BETA, PLSA_SW_LL_ONLY, "PLSA_FUSED"),
               (BETA, PLSA_FUSED | PLSA_SHARDED, "PLSA_SHARDED"), (BETA, PLSA_FUSED | PLSA_GRAPH, "PLSA_GRAPH"),
               (BETA, PLSA_FUSED | PLSA_REFERENCE_SUMS, "PLSA_REFERENCE_SUMS"), (BETA, PLSA_FUSED | PLSA_REFERENCE_LL, "PLSA_REFERENCE_LL"),
               (1.0, PLSA_FUSED | PLSA_GRAPH, "PLSA_GRAPH"), (1.0, 0, "PLSA_FUSED"),
               (0.0, PLSA_FUSED, "beta"), (-0.5, PLSA_FUSED, "beta"), (1.0000001, PLSA_FUSED, "beta"), (2.0, PLSA_FUSED, "beta"),
               (float("nan"), PLSA_FUSED, "beta"), (float("inf"), PLSA_FUSED, "beta")]
        for beta, flags, word in bad:
            with pytest.raises(amd.DeviceError, match=word):
                eng.fit_tempered(beta, sw, n_iter=2, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=flags)
        for beta in (0.0, 1.5, float("nan")):
            with pytest.raises(amd.DeviceError, match="beta"):
                eng.temper_factors(beta)
        for arithmetic in ("reference", "reference_source"):
            eng.set_arithmetic(arithmetic)
            with pytest.raises(amd.DeviceError, match="reference arithmetic"):
                eng.fit_tempered(BETA, sw, n_iter=2, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED)
            with pytest.raises(amd.DeviceError, match="reference arithmetic"):
                eng.fit_tempered(1.0, sw, n_iter=2, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED)
        eng.set_arithmetic(None)
        assert eng.timing_report() == {}, eng.timing_report()        # nothing was launched
        U, V = eng.get_factors()
        same_bits(U, U0, "a refusal moved U")
        same_bits(V, V0, "a refusal moved V")
        iters, _ = eng.fit_tempered(BETA, sw, n_iter=2, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED)
        assert iters == 2 and eng.timing_report()["k_temper"][0] == 4


# ------------------------------------------------------------------------------------------------
# I. end to end on a planted corpus
# ------------------------------------------------------------------------------------------------
E2E = dict(n=400, m=300, topics=5, tokens=30, background=0.1, k=25, seed=7, fresh=100, random_state=0, validation_fraction=0.1)


@functools.lru_cache(maxsize=None)
def planted_corpus():
    """Host NumPy: 5 topics on disjoint blocks of 60 words (Zipf-like inside a block) plus 10 % background over all words; a
    document mixes Dirichlet(0.3) of the topics and holds 30 tokens.  -> (X [400, 300] to fit, fresh [100, 300])"""
    p = E2E
    rs = np.random.RandomState(p["seed"])
    block = p["m"] // p["topics"]
    within = 1.0 / np.arange(1, block + 1) ** 0.7
    within /= within.sum()
    T = np.full((p["topics"], p["m"]), p["background"] / p["m"])
    for z in range(p["topics"]):
        T[z, z * block:(z + 1) * block] += (1.0 - p["background"]) * within
    theta = rs.dirichlet(np.full(p["topics"], 0.3), size=p["n"] + p["fresh"])
    P = theta @ T
    X = np.stack([rs.multinomial(p["tokens"], P[d] / P[d].sum()) for d in range(p["n"] + p["fresh"])])
    X = sp.csr_matrix(X.astype(np.float32))
    return X[:p["n"]].tocsr(), X[p["n"]:].tocsr()


def the_split(amd):
    """what plsa_fit_tempered(random_state=0) does first: the split, then the starting factors, from one stream"""
    from enstop_amd.plsa import plsa_init
    X, _ = planted_corpus()
    rng = np.random.RandomState(E2E["random_state"])
    observed, held = amd.split_documents(X, 1.0 - E2E["validation_fraction"], rng)
    U, V = plsa_init(observed, E2E["k"], "random", rng)
    scored = (np.diff(observed.indptr) > 0) & (np.diff(held.indptr) > 0)
    return observed, held, scored, U.astype(np.float32), V.astype(np.float32)


def em64(entries, U, V, beta=1.0):
    """one (tempered) EM step in float64, no threshold"""
    rows, cols, x = entries
    v = (V[:, cols].T * U[rows]) ** beta
    P = v / v.sum(1, keepdims=True) * x[:, None]
    A, B = np.zeros_like(U), np.zeros((V.shape[1], U.shape[1]))
    np.add.at(A, rows, P)
    np.add.at(B, cols, P)
    return A / A.sum(1, keepdims=True), (B / B.sum(0, keepdims=True)).T


def perplexity64(entries, U, V, scored):
    """(perplexity, per-document ll [n], per-document bound of DESIGN.md section 15) from float32 factors, in float64"""
    rows, cols, x = entries
    k = U.shape[1]
    dot = products32(rows, cols, U, V).astype(np.float64).sum(1)
    use = scored[rows] & (dot > 0)
    lg = np.log(dot[use])
    ll = np.bincount(rows[use], weights=x[use] * lg, minlength=U.shape[0])
    bound = np.bincount(rows[use], weights=x[use] * (4.0 * (k + 1) * U32 * np.maximum(1.0, np.abs(lg)) + k * 2.0 ** -149 / dot[use]),
                        minlength=U.shape[0])
    return float(np.exp(-ll.sum() / x[use].sum())), ll, bound


def test_planted_corpus_conditions(amd):
    """CPU, before anything runs on the device: no held-out token is of a word absent from the observed part, and in the
    float64 restatement at beta = 1 the validation perplexity has its minimum strictly inside the 200 iterations"""
    X, fresh = planted_corpus()
    assert X.shape == (400, 300) and fresh.shape == (100, 300)
    assert (np.asarray(X.sum(1)).ravel() == 30).all() and (np.asarray(fresh.sum(1)).ravel() == 30).all()
    observed, held, scored, U, V = the_split(amd)
    assert (observed + held != X).nnz == 0 and 0.08 < held.sum() / X.sum() < 0.12
    seen = np.asarray(observed.sum(0)).ravel() > 0
    assert held[:, ~seen].sum() == 0
    assert scored.sum() >= 350
    o, h = _coo(observed), _coo(held)
    o, h = (o[0], o[1], o[2].astype(np.float64)), (h[0], h[1], h[2].astype(np.float64))
    U, V = U.astype(np.float64), V.astype(np.float64)
    curve = [perplexity64(h, U.astype(np.float32), V.astype(np.float32), scored)[0]]
    for it in range(1, 201):
        U, V = em64(o, U, V)
        if it % 10 == 0:
            curve.append(perplexity64(h, U.astype(np.float32), V.astype(np.float32), scored)[0])
    best = int(np.argmin(curve))
    assert 0 < best < len(curve) - 1, curve
    assert curve[-1] > 2 * curve[best]                                # the likelihood-stopped regime is far past it


@pytest.mark.gpu
def test_end_to_end_on_the_planted_corpus(amd):
    from enstop_amd.engine import reset_engines
    from enstop_amd.tempered import TemperingSchedule, validation_perplexity
    X, fresh = planted_corpus()
    observed, held, scored, _, _ = the_split(amd)
    h = _coo(held)
    h = (h[0], h[1], h[2].astype(np.float64))
    seen = []

    def callback(report, eng):
        ll, tokens, unscored = eng.score_rows(held)                   # a second call: the same bits
        p, share = validation_perplexity(ll, tokens, unscored, scored)
        assert np.float64(p).view(np.uint64) == np.float64(report["perplexities"][-1]).view(np.uint64)
        U, V = eng.get_factors()
        p64, ll64, bound = perplexity64(h, U, V, scored)
        assert (np.abs(ll - ll64)[scored] <= bound[scored]).all(), "burst %d" % len(seen)
        assert (eng.shape[0], eng.shape[1]) == X.shape and (eng.download_active_csr() != observed).nnz == 0
        seen.append((p, p64, share, float((np.abs(ll - ll64)[scored] / np.maximum(bound[scored], 1e-300)).max())))

    with knobs({}):
        reset_engines()
        kw = dict(random_state=E2E["random_state"], validation_fraction=E2E["validation_fraction"])
        U, V, report = amd.plsa_fit_tempered(X, E2E["k"], callback=callback, **kw)
        ppl, betas = report["perplexities"], report["betas"]
        assert len(seen) == len(ppl) == len(betas) == len(report["actions"]) == len(report["training_log_likelihoods"]) >= 2
        assert report["unscored_share"] == 0 and not any(report["unscored_shares"])
        phase_one = [p for p, b in zip(ppl, betas) if b == 1.0]
        assert betas[0] == 1.0 and 10 * len(phase_one) < 200 and any(b < 1.0 for b in betas)    # left beta = 1 before n_iter
        assert report["selected_perplexity"] is not None and all(report["selected_perplexity"] <= p for p in phase_one)
        assert report["selected_perplexity"] == min(p for p, ok in zip(ppl, report["improved"]) if ok)
        assert report["n_iter"] == sum(report["iterations"]) <= 200
        # replay
        again = TemperingSchedule()
        again.start()
        for p, actions in zip(ppl, report["actions"]):
            assert again.observe(p) == actions
        assert again.stopped and again.selected["perplexity"] == report["selected_perplexity"]
        assert again.selected["beta"] == report["selected_beta"] and again.selected["spent"] == report["selected_iteration"]
        assert U.shape == (400, E2E["k"]) and V.shape == (E2E["k"], 300) and U.dtype == V.dtype == np.float32
        np.testing.assert_allclose(U.sum(1), 1.0, rtol=1e-5)
        np.testing.assert_allclose(V.sum(1), 1.0, rtol=1e-4)

        # the estimator, on the same counts as integers (it row-normalises float input before anything else, as the
        # reference's does; integer counts pass through, and their float32 casts are X's entries)
        Xi = X.astype(np.int64)
        est = amd.PLSA(n_components=E2E["k"], n_iter=200, random_state=E2E["random_state"], tempering="auto").fit(Xi)
        same_bits(est.components_, V, "PLSA(tempering='auto').components_")
        same_bits(est.embedding_, U, "PLSA(tempering='auto').embedding_")
        assert est.beta_ == report["selected_beta"] and est.n_iter_ == report["selected_iteration"]
        assert est.validation_perplexity_ == report["selected_perplexity"] and est.tempering_report_["perplexities"] == ppl
        same_bits(est.transform(Xi), U, "transform(X) is the returned fold-in")
        plain = amd.PLSA(n_components=E2E["k"], random_state=E2E["random_state"]).fit(Xi)
        none = amd.PLSA(n_components=E2E["k"], random_state=E2E["random_state"], tempering=None).fit(Xi)
        same_bits(none.components_, plain.components_, "tempering=None: components_")
        same_bits(none.embedding_, plain.embedding_, "tempering=None: embedding_")
        assert none.n_iter_ == plain.n_iter_ and not hasattr(none, "beta_")
        fixed = amd.PLSA(n_components=E2E["k"], random_state=E2E["random_state"], tempering=0.9).fit(Xi)
        assert fixed.beta_ == 0.9 and fixed.validation_perplexity_ is None and 1 <= fixed.n_iter_ <= 100
        assert np.isfinite(fixed.components_).all() and not np.array_equal(fixed.components_, plain.components_)
        for cls in (amd.StreamedPLSA, amd.BlockParallelPLSA, amd.GPUPLSA, amd.DistributedPLSA):
            with pytest.raises(ValueError, match="tempering"):
                cls(n_components=3).set_params(tempering="auto").fit(Xi)
        with pytest.raises(ValueError, match="reference"):
            amd.PLSA(n_components=3, arithmetic="reference", tempering="auto").fit(Xi)
        with pytest.raises(ValueError, match="tempering"):
            amd.PLSA(n_components=3, tempering="sometimes").fit(Xi)

        # the figures DESIGN.md section 16 records (no ratio between them is asserted)
        stopped = amd.PLSA(n_components=E2E["k"], random_state=E2E["random_state"])
        stopped.components_ = None
        figures = {}
        for name, model in (("schedule", est), ("likelihood-stopped", plain)):
            figures[name] = model.perplexity(fresh, method="completion", on_zero="skip")
        # beta = 1 stopped by validation: the schedule with no lowering allowed (beta_min = 1: the first lowering is refused)
        _, V1, r1 = amd.plsa_fit_tempered(X, E2E["k"], beta_min=1.0, **kw)
        assert set(r1["betas"]) == {1.0}
        stopped.components_ = V1
        figures["beta=1 stopped by validation"] = stopped.perplexity(fresh, method="completion", on_zero="skip")
        reset_engines()
    print("\nplanted corpus (400 x 300, k = 25): bursts (beta, validation perplexity, float64 restatement, worst per-document "
          "error / bound): %s" % ", ".join("(%.3f, %.2f, %.2f, %.3g)" % (b, s[0], s[1], s[3]) for b, s in zip(betas, seen)))
    print("selected: beta %.3f after %d iterations, validation perplexity %.2f; completion perplexity on 100 fresh documents: %s"
          % (report["selected_beta"], report["selected_iteration"], report["selected_perplexity"],
             ", ".join("%s %.1f" % kv for kv in figures.items())))
    assert all(np.isfinite(v) for v in figures.values())
