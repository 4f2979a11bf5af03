"""The step plsa_fit really runs, entry for entry against the float64 step -- and every driver loop, bit for bit, as that
step iterated.

test_pass_matrix.py holds one EM step to `step64` through em_accumulate / em_finish: k_col_pass -> k_col_reduce into the
accumulator, then k_colsum_partial, k_colsum_final, k_v_normalise.  An unsharded plsa_fit (what bench.py times) runs another
chain behind the same column pass (csrc/plsa_hip.hip: run_col_tail): norm_pwz from the float64 per-chunk sums the pass
itself writes (block_colsum -> chunk_sums; above 2048 chunks through k_norm_reduce), k_colsum_final, and k_col_reduce_norm
(per-column sums and the division in one sweep, heavy columns through an LDS copy of the norms).  A chunk whose sum row is
stale leaves every numerator right and every P(w|z) row off by a constant factor of order 1 / nnz, which no whole-fit
comparison to 1e-4 sees.

Part A: one production step, `set_factors(U0, V0); fit(n_iter=1, PLSA_FUSED)`, against step64 and against the sibling step
of a second engine with the same settings (em_accumulate, accumulator_get, em_finish), for every k of K_MATRIX.

    U, likelihood: the document pass is the same kernel in both steps: the same bits; and the matrix's bounds (b_row, check_ll)
    V:             |got - want| <= 4 (L_col + k) 2^-24 |want| (the matrix's model); zeros exact
    one divisor:   k_col_reduce_norm and k_col_reduce share col_reduce_body and the grid, so the sibling's accumulator `acc`
                   is bit for bit what was divided.  V[z, w] = fl(acc[w, z] / n_z): one correctly rounded division by ONE
                   float32 per topic, so over the entries with acc > 0 and V normal the float64 ratios r = acc / V lie in
                   [n_z / (1 + u), n_z / (1 - u)]:  max r / min r <= (1 + u) / (1 - u) <= 1 + 2u + 4u^2,  u = 2^-24.
                   A column divided by a stale or foreign norm breaks it.
    the divisor is the norm:  n_z := median r, S_z := sum_w acc[w, z] in float64.  acc[w, z] is a float32 sum of the column's
                   I_w item rows in some fixed order: within (I_w - 1) u of their exact sum.  The norm is the float64 sum of
                   ALL item rows (per chunk, then over the chunks) rounded to float32 once: one u.  The recovered divisor
                   carries the division's rounding: one more u.  So
                       |n_z - S_z| <= (I_max + 2) u S_z,   I_max = ceil(longest column / item_entries)
                   (one u of slack for the second-order terms).  About 5e-6 where a lost one-entry item is about 2e-4: this
                   is the assertion that sees a missed chunk.  The worst observed fraction of each bound is printed per k.

Which kernels ran is read from the timing names (part A runs with timing on, which also keeps hipGraph replay off) and
from Engine.fit_info().  test_norm_stage_switch_and_xcd_split takes the step to the shapes the matrix corpus cannot reach:
both sides of the `rows > 2048` switch to the two-stage norm at two lane shapes, and the XCD-split walk of the chunks on
small tables, fused and from a materialised P (k_col_pass<P> feeds the same tail).

Part B: a reference chain S_0 = (U0, V0), S_{i+1} = get_factors() after set_factors(S_i); fit(n_iter=1), on a context with
one stream and no look-ahead (PLSA_SPECULATE=0 PLSA_PIPELINE=0 PLSA_OVERLAP=0); the round trip through the host removes any
buffer parity, and step 1 of the chain is what part A verified.  Every form of the loop (two event-linked streams, the
speculating third buffer set, fork / join, one stream, hipGraph replay from the environment and from the flag) must return
S_N in bits for every (N, n_iter_per_test), the trace the reference's loop (enstop/plsa.py:583-640) gives on the chain's
likelihoods -- riding values from k_row_pass<fused,LL>, the trailing one from k_loglik -- stop where that loop stops, and
leave the context in the returned state (log_likelihood() and one more fit(n_iter=1) say so).  plsa_refit, the materialised
fit, PLSA_SW_LL_ONLY and PLSA_FUSED | PLSA_SHARDED without a communicator are held to their own one-step chains.

Needs a real MI355X for everything except the corpus builders, the loop restatement and the stop-choice helper.
"""
import contextlib
import os

import numpy as np
import pytest
import scipy.sparse as sp

from test_pass_matrix import (step64, check, check_ll, lane_shape, matrix_corpus, K_MATRIX, U32, C_FACTOR, TINY_THRESH,
                              EMPTY_DOCS)

PLSA_FUSED, PLSA_SW_LL_ONLY, PLSA_SHARDED, PLSA_GRAPH = 1, 8, 64, 128      # include/plsa_hip.h
KNOBS = ("PLSA_PACKED", "PLSA_HEAVY_ITEMS", "PLSA_COL_SEG", "PLSA_BALANCE", "PLSA_XCD_SPLIT", "PLSA_SPECULATE",
         "PLSA_PIPELINE", "PLSA_OVERLAP", "PLSA_GRAPH", "PLSA_FORCE_WIDE", "PLSA_ROW_ITEMS", "PLSA_ROW_SEG",
         "PLSA_OVERLAP_FULL_LIMIT", "PLSA_SMALL_GRID", "PLSA_ITEM_ORDER")


@contextlib.contextmanager
def knobs(env):
    """PLSA_* knobs are read when a context is created: exactly `env` of them set inside, the environment restored after"""
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


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b, what):
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=what)


# ------------------------------------------------------------------------------------------------
# corpora on both sides of the two-stage norm, and one that splits its chunks over the XCDs at a third lane shape
# ------------------------------------------------------------------------------------------------
COL_SEG = 16                     # PLSA_COL_SEG pinned: a column of `len` entries is ceil(len / 16) items
NORM_SWITCH = 2048               # run_col_tail: more chunk rows than this go through k_norm_reduce first
# (k, m, n, share of two-entry columns): k = 1024 walks 4 items per chunk, k = 64 walks 16
SWITCH_CASES = [(1024, 8192, 700, 0.5), (1024, 8193, 700, 0.5), (64, 32768, 9000, 0.01), (64, 32769, 9000, 0.01)]


def factors(rs, n, m, k):
    U = rs.rand(n, k) + 0.05
    U /= U.sum(1, keepdims=True)
    V = rs.rand(k, m) + 0.05
    V /= V.sum(1, keepdims=True)
    return U.astype(np.float32), V.astype(np.float32)


def switch_corpus(k, m, n, two):
    """every word in one or two documents: one column item each, so items == m and chunks == ceil(m / (256 / lpn))"""
    rs = np.random.RandomState(7 * k + m)
    lens = 1 + (rs.rand(m) < two)
    cols = np.repeat(np.arange(m), lens)
    first = rs.randint(0, n, m)
    rows = np.repeat(first, lens)
    second = np.flatnonzero(np.diff(cols, prepend=-1) == 0)                # the second entry of a two-entry column
    rows[second] = (rows[second] + 1 + rs.randint(0, n - 1, second.shape[0])) % n
    x = rs.randint(1, 8, cols.shape[0]).astype(np.float32)
    X = sp.csr_matrix((x, (rows, cols)), shape=(n, m))
    assert X.nnz == cols.shape[0]
    U, V = factors(rs, n, m, k)
    return X, U, V, (0.5 + rs.rand(n)).astype(np.float32)


def split_corpus(k=130, n=5000, m=3000, nnz=30000):
    """about 30 000 non-zeros over a P(z|d) table of 2.6 MB: the XCD split at column shape (32, 2)"""
    rs = np.random.RandomState(130)
    cells = np.unique(rs.randint(0, n * m, nnz))
    x = rs.randint(1, 8, cells.shape[0]).astype(np.float32)
    X = sp.csr_matrix((x, (cells // m, cells % m)), shape=(n, m))
    U, V = factors(rs, n, m, k)
    return X, U, V, (0.5 + rs.rand(n)).astype(np.float32)


def items_and_chunks(X, k, item_entries=COL_SEG):
    """host restatement of the column items (k_col_item_counts) and of the chunks the column pass walks (run_col_pass)"""
    lens = np.diff(X.tocsc().indptr)
    per_col = (lens + item_entries - 1) // item_entries
    items = int(per_col.sum())
    gpb = 256 // lane_shape(k)[1][0]
    return items, (items + gpb - 1) // gpb, gpb, int(per_col.max(initial=0))


@pytest.mark.parametrize("k, m, n, two", SWITCH_CASES)
def test_switch_corpora_sit_on_both_sides_of_2048_chunks(k, m, n, two):
    X, U, V, _ = switch_corpus(k, m, n, two)
    lens = np.diff(X.tocsc().indptr)
    assert lens.min() >= 1 and lens.max() == 2 and (lens == 2).sum() >= 100
    items, chunks, gpb, i_max = items_and_chunks(X, k)
    kp, col, _ = lane_shape(k)
    assert col == ((64, 4) if k == 1024 else (16, 1)) and gpb == (4 if k == 1024 else 16)
    assert items == m and i_max == 1
    assert chunks == (NORM_SWITCH if m % 2 == 0 else NORM_SWITCH + 1)
    assert (chunks > NORM_SWITCH) == (m % 2 == 1)
    if m % 2:
        assert items - (chunks - 1) * gpb == 1                    # the last chunk holds one item: the io < n_items guard
    assert n * kp * 4 > 2 << 20 and chunks >= 64                   # the column pass splits its chunks over the XCDs
    assert X.nnz <= 33500 and X.nnz * k <= 16000 * 1024            # the sizes the float64 restatement is run at


def test_split_corpus_reaches_the_xcd_split_at_a_third_shape():
    X, _, _, _ = split_corpus()
    kp, col, _ = lane_shape(130)
    items, chunks, gpb, _ = items_and_chunks(X, 130)
    assert col == (32, 2) and gpb == 8 and chunks >= 64 and X.shape[0] * kp * 4 > 2 << 20
    assert 29000 <= X.nnz <= 30000


# ------------------------------------------------------------------------------------------------
# the reference's loop on a chain of likelihoods, and the choice of stops
# ------------------------------------------------------------------------------------------------
def stop32(cur, prev, tol, zero_arm=True):
    """enstop/plsa.py:634-638 as the drivers evaluate it: float32 change / fabsf(cur), compared in float64"""
    cur, prev = np.float32(cur), np.float32(prev)
    change = np.abs(cur - prev)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.float32(change / np.abs(cur))
    return bool((zero_arm and change == 0) or float(rel) < tol)


def reference_loop(n_iter, per_test, tol, ride, trail, stops=True):
    """enstop/plsa.py:583-640 on a chain: the likelihood of S_0, then after iteration i with i % per_test == 0 the likelihood
    of S_{i+1} and the stop test.  ride[i]: the value the fused loop has for S_i (it rides on pass i, which exists for
    i < n_iter); trail[i]: k_loglik of S_i, what a traced test of the LAST iteration reports.  -> (iterations, trace).
    n_iter == 0: only the k_loglik value of S_0."""
    if n_iter == 0:
        return 0, [trail[0]]
    trace = [ride[0]]
    prev = ride[0]
    for i in range(n_iter):
        if i % per_test == 0:
            cur = ride[i + 1] if i + 1 < n_iter else trail[i + 1]
            trace.append(cur)
            if i + 1 < n_iter and stops:                          # (after the last iteration the verdict changes nothing)
                if stop32(cur, prev, tol):
                    return i + 1, trace
                prev = cur
    return n_iter, trace


def graph_pair_exists(n_iter, per_test):
    """two successive iterations i, i + 1 < n_iter neither of which carries a likelihood (pass i carries the test of
    iteration i - 1, pass 0 the initial one) and the first of which is not itself tested: what PLSA_GRAPH replays"""
    return any(i % per_test != 0 and (i - 1) % per_test != 0 for i in range(1, n_iter - 1))


def stop_choices(trace, n_riding):
    """tolerances that stop the loop at chosen tests.  trace: a tolerance-0 trace; tests 0 .. n_riding - 1 ride on a later pass
    (only their verdict can end the loop).  c_j: the relative change test j sees.  -> [(j or None, tolerance)]: the first
    test (twice its change), a middle and the last riding one (the geometric mean of c_j and the smallest earlier change,
    used only where that exceeds c_j by more than 0.1 %), and None = never (half the smallest change)."""
    t = np.asarray(trace, np.float32)
    c = [float(np.float32(np.abs(t[j + 1] - t[j]) / np.abs(t[j + 1]))) for j in range(n_riding)]
    out = []
    for j in sorted({0, n_riding // 2, n_riding - 1}):
        if j == 0:
            if c[0] > 0:
                out.append((0, 2.0 * c[0]))
        elif min(c[:j]) > 1.001 * c[j] and c[j] > 0:
            out.append((j, float(np.sqrt(c[j] * min(c[:j])))))
    if min(c) > 0:
        out.append((None, 0.5 * min(c)))
    return out


def test_reference_loop_and_stop_choices_on_a_synthetic_trace():
    ride = [np.float32(v) for v in (-1000, -900, -850, -840, -838, -837.5, -837.4, -837.39, -837.389)]
    trail = [np.float32(v - 0.25) for v in ride] + [np.float32(-837.0)]
    # n_iter_per_test 2, five iterations: tests after iterations 0, 2 (riding on passes 1, 3) and 4 (trailing)
    assert reference_loop(5, 2, 0.0, ride, trail) == (5, [ride[0], ride[1], ride[3], trail[5]])
    assert reference_loop(4, 2, 0.0, ride, trail) == (4, [ride[0], ride[1], ride[3]])
    assert reference_loop(1, 1, 0.0, ride, trail) == (1, [ride[0], trail[1]])
    assert reference_loop(3, 4, 0.0, ride, trail) == (3, [ride[0], ride[1]])
    assert reference_loop(0, 1, 0.0, ride, trail) == (0, [trail[0]])
    # changes seen with per_test 1: 100/900, 50/850, 10/840, 2/838, ...
    assert reference_loop(8, 1, 0.1, ride, trail) == (2, [ride[0], ride[1], ride[2]])          # 0.111 goes on, 0.0588 stops
    assert reference_loop(8, 1, 0.2, ride, trail) == (1, [ride[0], ride[1]])
    assert reference_loop(2, 1, 1.0, ride, trail) == (1, [ride[0], ride[1]])
    assert reference_loop(1, 1, 1.0, ride, trail) == (1, [ride[0], trail[1]])                  # nothing left to stop
    assert reference_loop(8, 1, 0.2, ride, trail, stops=False)[0] == 8
    flat = [np.float32(-5)] * 4
    assert reference_loop(3, 1, 0.0, flat, flat) == (1, flat[:2])                                # the `change == 0` arm
    assert stop32(-837.39, -837.4, 1e-4) and not stop32(-837.39, -837.4, 1e-6)
    _, trace = reference_loop(8, 1, 0.0, ride, trail)
    choices = stop_choices(trace, 7)
    assert [j for j, _ in choices] == [0, 3, 6, None]
    for j, tol in choices:
        iters, got = reference_loop(8, 1, tol, ride, trail)
        assert (iters, got) == ((8, trace) if j is None else (j + 1, trace[:j + 2])), (j, tol)
    # a change that does not fall by 0.1 % is no usable stop
    assert [j for j, _ in stop_choices([-100.0, -90.0, -81.0, -72.9], 3)] == [0, None]
    # per_test 1 or 2: every second pass at least carries a likelihood, no pair is free of one
    assert not graph_pair_exists(9, 1) and not graph_pair_exists(9, 2) and not graph_pair_exists(3, 4)
    assert graph_pair_exists(4, 3) and graph_pair_exists(4, 4) and graph_pair_exists(9, 3)


# ------------------------------------------------------------------------------------------------
# part A: one production step
# ------------------------------------------------------------------------------------------------
STEP_SETTINGS = {
    "default": {},
    "arrays": {"PLSA_PACKED": "0"},
    "heavy": {"PLSA_HEAVY_ITEMS": "2", "PLSA_COL_SEG": "8"},
    "balance": {"PLSA_BALANCE": "1"},            # the TIMED instantiations run before the real launch where the chunks are split
    "no_split": {"PLSA_XCD_SPLIT": "0"},
}
STEP_RUNS = [(False, 1e-32), (True, 1e-32), (True, 0.0), (False, 0.0)]          # (weighted, thresh): both TINY forms
RATIO_ONE_DIVISOR = 2 * U32 + 4 * U32 * U32


@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


@pytest.fixture(scope="module")
def worst():
    out = {}
    yield out
    if out:
        print("\nfit driver: worst error / bound per quantity: " + ", ".join("%s %.3g" % (key, v) for key, v in sorted(out.items())))


def divisor_checks(acc, V, k, i_max, tag, ratios):
    """one divisor per topic, and that divisor is the norm (module docstring)"""
    A = np.asarray(acc[:, :k], np.float64)
    tiny = np.finfo(np.float32).tiny
    worst_ratio = worst_norm = 0.0
    for z in range(k):
        a, v = A[:, z], V[z]
        sel = (a > 0) & (np.abs(v) >= tiny)
        assert sel.any(), "%s: topic %d has no usable entry" % (tag, z)
        r = a[sel] / v[sel].astype(np.float64)
        spread = r.max() / r.min() - 1.0
        assert spread <= RATIO_ONE_DIVISOR, "%s: topic %d divided by more than one float32: max r / min r - 1 = %.3g (%.3g allowed)" % (
            tag, z, spread, RATIO_ONE_DIVISOR)
        n_z, S_z = float(np.median(r)), float(a.sum())
        bound = (i_max + 2) * U32 * S_z
        assert abs(n_z - S_z) <= bound, "%s: topic %d divided by %.9g, its column sums add up to %.9g (off by %.3g x the bound %.3g)" % (
            tag, z, n_z, S_z, abs(n_z - S_z) / bound, bound / S_z)
        worst_ratio = max(worst_ratio, spread / RATIO_ONE_DIVISOR)
        worst_norm = max(worst_norm, abs(n_z - S_z) / bound)
    ratios["divisor " + tag] = worst_ratio
    ratios["norm " + tag] = worst_norm


def production_step(eng, sib, X, U0, V0, sw, thresh, k, ref, tag, ratios, path="fused"):
    """one step on `eng` the way plsa_fit (path 'fused') or e_step + m_step ('kernels') runs it, the sibling step on `sib`
    through em_accumulate / em_finish, and every assertion of part A.  -> (U, V, likelihood, fit_info)"""
    n, m = X.shape
    kp = (k + 3) // 4 * 4
    fused = path == "fused"
    eng.set_factors(U0, V0)
    eng.timing_reset()
    if fused:
        iters, trace = eng.fit(sw, n_iter=1, n_iter_per_test=1, tolerance=0.0, e_step_thresh=thresh, flags=PLSA_FUSED)
        assert iters == 1 and trace.shape == (1,), (tag, iters, trace)
        ll = trace[0]
    else:
        ll = eng.log_likelihood(sw)
        eng.e_step(thresh, want_host_copy=False)
        eng.m_step(sw)
    info = eng.fit_info()
    names = set(eng.timing_report())
    U, V = eng.get_factors()
    sib.set_factors(U0, V0)
    ll_sib = sib.em_accumulate(sw, thresh, want_ll=True, materialised=not fused)
    acc = sib.accumulator_get().reshape(m, kp)
    sib.em_finish()
    U_sib, _ = sib.get_factors()
    L_row, L_col = ref["L_row"], ref["L_col"]
    b_row, b_col = C_FACTOR * (L_row + k) * U32, C_FACTOR * (L_col + k) * U32
    # U and the likelihood: the same document pass in both steps
    if fused:
        same_bits(U, U_sib, "U of plsa_fit vs em_accumulate: " + tag)
        assert np.float32(ll).view(np.uint32) == np.float32(ll_sib).view(np.uint32), (tag, ll, ll_sib)
    check("U " + tag, U, ref["U"], b_row, ratios)
    check_ll("LL " + tag, ll, ref["ll"], ref["ll_scale"], k, ratios)
    # V against the float64 step; padding topics of what was divided exactly 0
    check("V " + tag, V, ref["V"], b_col, ratios)
    assert not acc[:, k:].any(), tag
    bal = eng.balance_info()
    lens = np.diff(X.tocsc().indptr)
    i_max = int(-(-lens.max() // bal["item_entries"]))
    divisor_checks(acc, V, k, i_max, tag, ratios)
    # which kernels ran
    assert {"k_col_pass<fused>" if fused else "k_col_pass<P>", "k_col_reduce_norm", "k_colsum_final"} <= names, (tag, names)
    assert not {"k_col_reduce", "k_colsum_partial", "k_v_normalise"} & names, (tag, names)
    assert ("k_norm_reduce" in names) == info["two_stage_norm"], (tag, info, names)
    assert info["col_tail"] == "sweep" and info["graph_launches"] == 0, (tag, info)
    if fused:
        assert info["fused"] and "k_row_pass<fused,LL>" in names, (tag, info, names)
    return U, V, ll, info


@pytest.mark.gpu
@pytest.mark.parametrize("k", K_MATRIX)
def test_production_step_against_the_float64_step(amd, worst, k):
    """Part A on the matrix corpus: every lane shape, both TINY forms, with and without weights, packed and unpacked, forced
    heavy columns, measured XCD boundaries, XCD split off."""
    X, U0, V0, sw_doc = matrix_corpus(k)
    n, m = X.shape
    kp = (k + 3) // 4 * 4
    want = {(w, t): step64(X, U0, V0, t, sw_doc if w else None) for w, t in STEP_RUNS}
    lens = np.diff(X.tocsc().indptr)
    ratios = {}
    for name, env in STEP_SETTINGS.items():
        eng, sib = make_engine(amd, env, X), make_engine(amd, env, X)
        try:
            eng.timing(True)
            for weighted, thresh in STEP_RUNS:
                tag = "k=%d %s sw=%d thresh=%g" % (k, name, weighted, thresh)
                U, V, ll, info = production_step(eng, sib, X, U0, V0, sw_doc if weighted else None, thresh, k,
                                                 want[weighted, thresh], tag, ratios)
                for d in EMPTY_DOCS:
                    assert not U[d].any(), tag
                assert eng.packed_info()["csc"] == ("arrays" if name == "arrays" else "packed"), tag
                assert not info["two_stage_norm"], (tag, info)                  # about 500 items: never 2048 chunks
                if name == "no_split":
                    assert not info["xcd_split"], (tag, info)
                else:                                                           # run_col_pass: 64 chunks and a table over 2 MB
                    items, chunks, _, _ = items_and_chunks(X, k, eng.balance_info()["item_entries"])
                    assert eng.balance_info()["n_items"] == items, tag
                    assert info["xcd_split"] == (chunks >= 64 and n * kp * 4 > 2 << 20), (tag, info, chunks)
                if name == "balance" and info["xcd_split"]:
                    assert eng.balance_info()["timed_launches"] >= 1, tag      # the TIMED instantiation ran
            if name == "heavy":
                assert eng.balance_info()["item_entries"] == 8
                assert ((lens + 7) // 8 > 2).sum() >= 1                         # columns on the heavy (LDS norms) branch
        finally:
            eng.close()
            sib.close()
    per_q = {}
    for key, v in ratios.items():
        q = key.split(" ")[0]
        per_q[q] = max(per_q.get(q, 0.0), v)
        worst[q] = max(worst.get(q, 0.0), v)
    print("\nk=%d: worst error / bound: %s" % (k, ", ".join("%s %.3g" % (q, v) for q, v in sorted(per_q.items()))))


SHAPE_CASES = [("switch",) + case for case in SWITCH_CASES] + [("split", 130, 3000, 5000, 0.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind, k, m, n, two", SHAPE_CASES)
def test_norm_stage_switch_and_xcd_split(amd, worst, kind, k, m, n, two):
    """Part A at the shapes the matrix corpus cannot reach: 2048 chunks (one norm stage) and 2049 (two stages, the last
    chunk holding one item) at column shapes (64, 4) and (16, 1), and the XCD-split walk of the chunks at (32, 2) -- each one
    step, fused and from a materialised P; with PLSA_XCD_SPLIT=0 the same bits."""
    X, U0, V0, sw = switch_corpus(k, m, n, two) if kind == "switch" else split_corpus(k, n, m)
    items, chunks, gpb, _ = items_and_chunks(X, k)
    runs = [("fused", True, 1e-32), ("fused", False, 0.0), ("kernels", True, 1e-32)]
    want = {(w, t): step64(X, U0, V0, t, sw if w else None) for _, w, t in runs}
    ratios, got = {}, {}
    for split in (True, False):
        env = {"PLSA_COL_SEG": str(COL_SEG)}
        if not split:
            env["PLSA_XCD_SPLIT"] = "0"
        eng, sib = make_engine(amd, env, X), make_engine(amd, env, X)
        try:
            eng.timing(True)
            for path, weighted, thresh in runs:
                tag = "%s k=%d m=%d split=%d %s sw=%d thresh=%g" % (kind, k, m, split, path, weighted, thresh)
                U, V, ll, info = production_step(eng, sib, X, U0, V0, sw if weighted else None, thresh, k,
                                                 want[weighted, thresh], tag, ratios, path)
                bal = eng.balance_info()
                assert bal["item_entries"] == COL_SEG and bal["n_items"] == items, (tag, bal)
                if kind == "switch":
                    assert items == m and chunks == (NORM_SWITCH if m % 2 == 0 else NORM_SWITCH + 1), (tag, items, chunks)
                assert info["two_stage_norm"] == (chunks > NORM_SWITCH), (tag, info, chunks)
                assert info["xcd_split"] == split, (tag, info)
                got[split, path, weighted, thresh] = (U, V, ll)
        finally:
            eng.close()
            sib.close()
    for (split, path, weighted, thresh), (U, V, ll) in got.items():
        if split:
            U1, V1, ll1 = got[False, path, weighted, thresh]
            what = "%s k=%d m=%d %s sw=%d: PLSA_XCD_SPLIT=0 vs split" % (kind, k, m, path, weighted)
            same_bits(U1, U, what + ": U")
            same_bits(V1, V, what + ": V")
            assert np.float64(ll1).view(np.uint64) == np.float64(ll).view(np.uint64), (what, ll1, ll)
    per_q = {}
    for key, v in ratios.items():
        q = key.split(" ")[0]
        per_q[q] = max(per_q.get(q, 0.0), v)
        worst[q] = max(worst.get(q, 0.0), v)
    print("\n%s k=%d m=%d (%d chunks): worst error / bound: %s" % (
        kind, k, m, chunks, ", ".join("%s %.3g" % (q, v) for q, v in sorted(per_q.items()))))


# ------------------------------------------------------------------------------------------------
# part B: every driver loop is that step iterated
# ------------------------------------------------------------------------------------------------
REF_ENV = {"PLSA_SPECULATE": "0", "PLSA_PIPELINE": "0", "PLSA_OVERLAP": "0"}       # one stream, no look-ahead
N_GRID = (1, 2, 3, 4, 5, 8, 9)
P_GRID = (1, 2, 3, 4)
N_MAX = max(N_GRID)
N_STOP = 17                      # the stop runs: tests after iterations 0, 4, 8, 12 still ride at n_iter_per_test = 4, and the
                                 # changes they see fall from test to test (the first EM steps of a random start need not)
THRESH = 1e-32
# form -> (knobs of the context, flags added to the fit, pipelined, may speculate, replays graphs)
FORMS = {
    "default": ({}, 0, True, True, False),
    "speculate": ({"PLSA_SPECULATE": "1"}, 0, True, True, False),
    "no_speculate": ({"PLSA_SPECULATE": "0"}, 0, True, False, False),
    "no_pipeline": ({"PLSA_PIPELINE": "0"}, 0, False, True, False),
    "no_overlap": ({"PLSA_OVERLAP": "0"}, 0, False, True, False),
    "graph_env": ({"PLSA_GRAPH": "1"}, 0, False, False, True),
    "graph_flag": ({}, PLSA_GRAPH, False, False, True),
}
_chains = {}


def step_chain(amd, k, weighted):
    """S_0 .. S_{N_STOP + 1} by single steps with a host round trip in between, with the likelihood that rides on each step
    (float32, as the trace holds it) and the k_loglik value of each state (float64; the trace holds its float32).  For the
    unweighted chain also both likelihoods with weights (PLSA_SW_LL_ONLY: the weights enter the likelihood only)."""
    key = (k, weighted)
    if key in _chains:
        return _chains[key]
    X, U0, V0, sw_doc = matrix_corpus(k)
    sw = sw_doc if weighted else None
    eng = make_engine(amd, REF_ENV, X)
    try:
        S, ride, kll, ride_sw, kll_sw = [(U0, V0)], [], [], [], []
        for i in range(N_STOP + 1):
            eng.set_factors(*S[i])
            kll.append(eng.log_likelihood(sw))
            if not weighted:
                kll_sw.append(eng.log_likelihood(sw_doc))
                iters, trace = eng.fit(sw_doc, n_iter=1, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH,
                                       flags=PLSA_FUSED | PLSA_SW_LL_ONLY)
                ride_sw.append(trace[0])
                only_ll = eng.get_factors()
                eng.set_factors(*S[i])
            iters, trace = eng.fit(sw, n_iter=1, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED)
            assert iters == 1 and trace.shape == (1,)
            info = eng.fit_info()
            assert info["fused"] and not info["pipelined"] and not info["speculated"] and not info["graph_launches"], info
            ride.append(trace[0])
            S.append(eng.get_factors())
            if not weighted:                                       # weights that enter the likelihood only: the same step
                same_bits(only_ll[0], S[-1][0], "PLSA_SW_LL_ONLY step %d: U" % i)
                same_bits(only_ll[1], S[-1][1], "PLSA_SW_LL_ONLY step %d: V" % i)
        eng.set_factors(*S[N_STOP + 1])
        kll.append(eng.log_likelihood(sw))
    finally:
        eng.close()
    out = dict(X=X, sw=sw, sw_doc=sw_doc, S=S, ride=ride, kll=kll, trail=[np.float32(v) for v in kll],
               ride_sw=ride_sw, kll_sw=kll_sw, trail_sw=[np.float32(v) for v in kll_sw])
    _chains[key] = out
    return out


def run_and_check(eng, fit, sw, S, kll, n_iter, per_test, tol, want_iters, want_trace, tag, flags=PLSA_FUSED):
    """one driver call from S_0: count, factors and trace, then the state it left behind.  fit: eng.fit or eng.refit"""
    eng.set_factors(*S[0])
    iters, trace = fit(sw, n_iter=n_iter, n_iter_per_test=per_test, tolerance=tol, e_step_thresh=THRESH, flags=flags,
                       trace=True)
    info = eng.fit_info()
    assert iters == want_iters, (tag, iters, want_iters, trace)
    U, V = eng.get_factors()
    same_bits(U, S[iters][0], tag + ": U is not U of S_%d" % iters)
    same_bits(V, S[iters][1], tag + ": V is not V of S_%d" % iters)
    same_bits(trace, np.asarray(want_trace, np.float32), tag + ": trace")
    # the state left behind, without setting factors
    ll = eng.log_likelihood(sw)
    assert np.float64(ll).view(np.uint64) == np.float64(kll[iters]).view(np.uint64), (tag, "likelihood of the state left", ll, kll[iters])
    again, _ = fit(sw, n_iter=1, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=flags & ~PLSA_GRAPH)
    assert again == 1, tag
    U, V = eng.get_factors()
    same_bits(U, S[iters + 1][0], tag + ": one more step: U is not U of S_%d" % (iters + 1))
    same_bits(V, S[iters + 1][1], tag + ": one more step: V is not V of S_%d" % (iters + 1))
    return info


def riding_tests(n_iter, per_test):
    return len([i for i in range(n_iter) if i % per_test == 0 and i + 1 < n_iter])


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("k", [6, 64, 130])
def test_every_loop_form_is_the_step_iterated(amd, k, form):
    env, extra, pipelined, may_speculate, graphs = FORMS[form]
    for weighted in (False, True):
        ch = step_chain(amd, k, weighted)
        S, ride, trail, kll, sw = ch["S"], ch["ride"], ch["trail"], ch["kll"], ch["sw"]
        eng = make_engine(amd, env, ch["X"])        # timing stays off: it would switch the graph replay off
        try:
            # -- tolerance 0: N iterations are the step applied N times
            for n_iter in N_GRID:
                for per_test in P_GRID:
                    tag = "k=%d %s sw=%d N=%d per_test=%d" % (k, form, weighted, n_iter, per_test)
                    want_iters, want_trace = reference_loop(n_iter, per_test, 0.0, ride, trail)
                    assert want_iters == n_iter, tag                 # (no change is exactly 0 on this corpus)
                    info = run_and_check(eng, eng.fit, sw, S, kll, n_iter, per_test, 0.0, n_iter, want_trace, tag,
                                         PLSA_FUSED | extra)
                    assert info["fused"] and info["col_tail"] == "sweep", (tag, info)
                    assert info["pipelined"] == pipelined, (tag, info)
                    assert info["speculated"] == (may_speculate and per_test >= 2 and n_iter >= 3), (tag, info)
                    if graphs and graph_pair_exists(n_iter, per_test):
                        assert info["graph_launches"] >= 1, (tag, info)
                    else:
                        assert info["graph_launches"] == 0, (tag, info)
            # -- stops: at the first test, a middle one, the last one that can stop, never
            for per_test in P_GRID:
                _, full = reference_loop(N_STOP, per_test, 0.0, ride, trail)
                choices = stop_choices(full, riding_tests(N_STOP, per_test))
                assert len(choices) >= 3, ("the corpus gives too few usable stops", k, weighted, per_test, full)
                for j, tol in choices:
                    tag = "k=%d %s sw=%d N=%d per_test=%d stop at test %s (tolerance %.3g)" % (k, form, weighted, N_STOP, per_test, j, tol)
                    want_iters, want_trace = reference_loop(N_STOP, per_test, tol, ride, trail)
                    if j is None:
                        assert (want_iters, want_trace) == (N_STOP, full), tag
                    else:
                        assert want_iters == j * per_test + 1 and want_trace == full[:j + 2], tag
                    run_and_check(eng, eng.fit, sw, S, kll, N_STOP, per_test, tol, want_iters, want_trace, tag, PLSA_FUSED | extra)
        finally:
            eng.close()


K_OTHER = 64


@pytest.mark.gpu
def test_refit_is_its_own_step_iterated(amd):
    """plsa_refit, fused: P(z|d) follows its own one-iteration chain, P(w|z) stays untouched bit for bit, the trace is the
    reference's on the chain (a negative likelihood never stops a refit, enstop/plsa.py:913-918)."""
    X, U0, V0, sw = matrix_corpus(K_OTHER)
    kw = dict(n_iter=1, n_iter_per_test=1, tolerance=0.0, e_step_thresh=THRESH, flags=PLSA_FUSED)
    eng = make_engine(amd, REF_ENV, X)
    try:
        eng.set_factors(U0, V0)
        eng.refit(None, **kw)
        same_bits(eng.get_factors()[0], step_chain(amd, K_OTHER, False)["S"][1][0], "unweighted R_1 is not U of S_1")
        R, ride, kll = [(U0, V0)], [], []
        for i in range(N_MAX + 2):
            eng.set_factors(*R[i])
            kll.append(eng.log_likelihood(sw))
            if i <= N_MAX:
                iters, trace = eng.refit(sw, **kw)
                assert iters == 1 and trace.shape == (1,)
                ride.append(trace[0])
                R.append(eng.get_factors())
                same_bits(R[-1][1], V0, "refit step %d moved P(w|z)" % i)
    finally:
        eng.close()
    assert all(v < 0 for v in kll)
    trail = [np.float32(v) for v in kll]
    eng = make_engine(amd, {}, X)
    try:
        for n_iter in N_GRID:
            for per_test in P_GRID:
                for tol in (0.0, 0.5):
                    tag = "refit k=%d N=%d per_test=%d tolerance=%g" % (K_OTHER, n_iter, per_test, tol)
                    _, want_trace = reference_loop(n_iter, per_test, tol, ride, trail, stops=False)
                    info = run_and_check(eng, eng.refit, sw, R, kll, n_iter, per_test, tol, n_iter, want_trace, tag)
                    assert info["fused"] and info["col_tail"] is None and not info["pipelined"], (tag, info)
    finally:
        eng.close()


@pytest.mark.gpu
def test_materialised_fit_is_e_step_m_step_iterated(amd):
    """plsa_fit without PLSA_FUSED against the chain of e_step(); m_step() calls; every trace entry is k_loglik of its state."""
    X, U0, V0, sw = matrix_corpus(K_OTHER)
    eng = make_engine(amd, REF_ENV, X)
    try:
        M, kll = [(U0, V0)], []
        for i in range(N_MAX + 2):
            eng.set_factors(*M[i])
            kll.append(eng.log_likelihood(sw))
            if i <= N_MAX:
                eng.e_step(THRESH, want_host_copy=False)
                eng.m_step(sw)
                M.append(eng.get_factors())
    finally:
        eng.close()
    trail = [np.float32(v) for v in kll]
    eng = make_engine(amd, {}, X)
    try:
        for n_iter in N_GRID:
            for per_test in P_GRID:
                tag = "materialised k=%d N=%d per_test=%d" % (K_OTHER, n_iter, per_test)
                want_trace = [trail[0]] + [trail[i + 1] for i in range(n_iter) if i % per_test == 0]
                info = run_and_check(eng, eng.fit, sw, M, kll, n_iter, per_test, 0.0, n_iter, want_trace, tag, flags=0)
                assert not info["fused"] and info["col_tail"] == "sweep" and not info["pipelined"], (tag, info)
    finally:
        eng.close()


@pytest.mark.gpu
def test_weights_in_the_likelihood_only(amd):
    """PLSA_SW_LL_ONLY: the factors of the unweighted chain, the trace of the weighted likelihoods of its states."""
    ch = step_chain(amd, K_OTHER, False)
    eng = make_engine(amd, {}, ch["X"])
    try:
        for n_iter in N_GRID:
            for per_test in P_GRID:
                tag = "sw in the likelihood only k=%d N=%d per_test=%d" % (K_OTHER, n_iter, per_test)
                _, want_trace = reference_loop(n_iter, per_test, 0.0, ch["ride_sw"], ch["trail_sw"])
                info = run_and_check(eng, eng.fit, ch["sw_doc"], ch["S"], ch["kll_sw"], n_iter, per_test, 0.0, n_iter, want_trace,
                                     tag, flags=PLSA_FUSED | PLSA_SW_LL_ONLY)
                assert info["fused"] and info["col_tail"] == "sweep", (tag, info)
    finally:
        eng.close()


@pytest.mark.gpu
def test_sharded_fit_without_a_communicator_is_accumulate_finish_iterated(amd):
    """PLSA_FUSED | PLSA_SHARDED on one context: the chain of em_accumulate(); em_finish(), the four-kernel column tail."""
    X, U0, V0, sw = matrix_corpus(K_OTHER)
    eng = make_engine(amd, REF_ENV, X)
    try:
        S, ride, kll = [(U0, V0)], [], []
        for i in range(N_MAX + 2):
            eng.set_factors(*S[i])
            kll.append(eng.log_likelihood(sw))
            if i <= N_MAX:
                ride.append(np.float32(eng.em_accumulate(sw, THRESH, want_ll=True)))
                eng.em_finish()
                S.append(eng.get_factors())
    finally:
        eng.close()
    trail = [np.float32(v) for v in kll]
    eng = make_engine(amd, {}, X)
    try:
        for n_iter in N_GRID:
            for per_test in P_GRID:
                tag = "sharded k=%d N=%d per_test=%d" % (K_OTHER, n_iter, per_test)
                want_iters, want_trace = reference_loop(n_iter, per_test, 0.0, ride, trail)
                info = run_and_check(eng, eng.fit, sw, S, kll, n_iter, per_test, 0.0, want_iters, want_trace, tag,
                                     flags=PLSA_FUSED | PLSA_SHARDED)
                assert info["fused"] and info["col_tail"] == "four_kernels", (tag, info)
                assert not info["pipelined"] and not info["speculated"] and not info["graph_launches"], (tag, info)
    finally:
        eng.close()
