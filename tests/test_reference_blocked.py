"""The reference arithmetic in bounded memory (include/plsa_hip_blocked.h, `p_budget=`): plsa_fit / plsa_refit with P(z|w,d) of
ONE BLOCK of whole documents at a time.  Every chain of the reference M-step runs over the non-zeros in document-major order,
so a sum is either complete inside a block (a document's row) or handed from block to block (a word's column accumulator,
norm_pwz): the same additions in the same order.  Nothing here is a tolerance: a budgeted fit returns the BITS of the
unbudgeted one, of the reference's fixtures and of the strict oracle.  Needs a real MI355X: -m gpu.

Budgets are derived from the corpus as 4 * kp * (max(nnz // B, longest document) + 64) bytes; every blocked case checks the
blocks the engine reports against the greedy plan computed here, and that P(z|w,d) was allocated within the budget.
"""
import numpy as np
import pytest

from conftest import load_golden, golden_csr, coo_arrays
from test_reference_arithmetic import same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


def kp_of(k):
    return (k + 3) // 4 * 4


def budget_for(X, k, B):
    longest = int(np.diff(X.indptr).max())
    return 4 * kp_of(k) * (max(X.nnz // B, longest) + 64)


def plan_for(X, k, budget):
    """non-zeros of the blocks of the greedy plan: whole documents, in order, (block_nnz + 64) * kp * 4 <= budget"""
    max_rows = budget // (4 * kp_of(k)) - 64
    sizes, cuts, b0 = [], [0], 0
    for d in range(X.shape[0]):
        if X.indptr[d + 1] - b0 > max_rows:
            sizes.append(int(X.indptr[d] - b0)); cuts.append(d); b0 = X.indptr[d]
    sizes.append(int(X.nnz - b0)); cuts.append(X.shape[0])
    return sizes, cuts


def check_blocks(info, X, k, budget, at_least=3):
    sizes, _ = plan_for(X, k, budget)
    assert info["budget"] == budget and info["blocks"] == len(sizes) and info["largest_block_nnz"] == max(sizes), (info, sizes)
    assert info["blocks"] >= at_least, info
    assert 0 < info["p_allocated_bytes"] <= budget, info
    return sizes


def shared_info(amd):
    from enstop_amd.engine import get_engine
    eng = get_engine()
    assert eng.p_budget == 0, "the shared engine kept the budget of a finished call"
    return eng.p_block_info()


# ------------------------------------------------------------------------------------------------------------------------
# 1. the reference's own fixtures under a budget
# ------------------------------------------------------------------------------------------------------------------------
FIT_CASES = [(case, arithmetic, 4) for case in ("fit_k8_tol0", "fit_k5_earlystop", "fit_k4_weighted", "fit_k8_thresh", "fit_k16_mid")
             for arithmetic in ("reference", "reference_source")] + [("fit_k4_big", "reference", 8)]


@pytest.mark.parametrize("case,arithmetic,B", FIT_CASES)
def test_fit_bits_under_a_budget(amd, case, arithmetic, B):
    """test_fit_bits (tests/test_reference_arithmetic.py) with p_budget: iteration count equal, factors bit for bit, the
    likelihood trace within that test's tolerances."""
    g = load_golden(case)
    X = golden_csr(g)
    init = (g["U_init"], g["V_init"]) if "U_init" in g else "random"
    budget = budget_for(X, int(g["k"]), B)
    for flags in (0, amd.PLSA_FUSED):
        U, V, info = amd.plsa_fit(X, int(g["k"]), g["sw"], init=init, n_iter=int(g["n_iter"]),
                                  n_iter_per_test=int(g["n_iter_per_test"]), tolerance=float(g["tol"]),
                                  e_step_thresh=float(g["thresh"]), random_state=int(g["fit_seed"]),
                                  flags=flags, return_info=True, arithmetic=arithmetic, p_budget=budget)
        check_blocks(shared_info(amd), X, int(g["k"]), budget)
        assert info["n_iter"] == int(g["iters"])
        same_bits(U, g["U"], case + " P(z|d)")
        if "V" in g:
            same_bits(V, g["V"], case + " P(w|z)")
        else:
            same_bits(V[:, g["V_cols"]], g["V_sample"], case + " P(w|z) sample")
        tr, ref = np.asarray(info["log_likelihood_trace"], np.float64), np.asarray(g["ll_trace"], np.float64)
        n_cmp = min(len(tr), len(ref))
        fin = np.isfinite(ref[:n_cmp])
        tol = 2e-6 if arithmetic == "reference_source" else 1e-5
        if arithmetic == "reference_source" or case != "fit_k4_big":
            assert np.all(np.abs(tr[:n_cmp][fin] - ref[:n_cmp][fin]) <= tol * np.abs(ref[:n_cmp][fin])), (tr, ref)


@pytest.mark.parametrize("case", ["refit_k6", "refit_k8_weighted"])
def test_refit_bits_under_a_budget(amd, case):
    g = load_golden(case)
    X = golden_csr(g)
    k = g["topics"].shape[0]
    budget = budget_for(X, k, 4)
    for arithmetic in ("reference", "reference_source"):
        U, info = amd.plsa_refit(X, g["topics"], g["sw"], n_iter=int(g["n_iter"]), n_iter_per_test=int(g["n_iter_per_test"]),
                                 tolerance=float(g["tol"]), random_state=np.random.RandomState(42), return_info=True,
                                 arithmetic=arithmetic, p_budget=budget)
        check_blocks(shared_info(amd), X, k, budget)
        assert info["n_iter"] == int(g["iters"])
        same_bits(U, g["U"], case)


def test_estimator_keyword(amd, monkeypatch):
    """PLSA(arithmetic="reference", p_budget=...) reaches the driver; so does ENSTOP_AMD_P_BUDGET_MB when the keyword is None,
    and a default-arithmetic fit under the same budget is the engine's own, unblocked."""
    g = load_golden("fit_k16_mid")
    X = golden_csr(g)
    k = int(g["k"])
    kw = dict(n_iter=int(g["n_iter"]), n_iter_per_test=int(g["n_iter_per_test"]), tolerance=float(g["tol"]),
              e_step_thresh=float(g["thresh"]), random_state=int(g["fit_seed"]))
    budget = budget_for(X, k, 4)
    est = amd.PLSA(n_components=k, arithmetic="reference", p_budget=budget, **kw).fit(X.astype(np.int64))
    check_blocks(shared_info(amd), X, k, budget)
    same_bits(est.embedding_, g["U"], "estimator")
    same_bits(est.components_, g["V"], "estimator")
    Ud, Vd = amd.plsa_fit(X, k, g["sw"], flags=0, **kw)
    Ub, Vb = amd.plsa_fit(X, k, g["sw"], flags=0, p_budget=budget, **kw)          # default arithmetic: no effect
    same_bits(Ub, Ud, "default arithmetic under a budget"); same_bits(Vb, Vd, "default arithmetic under a budget")
    assert np.any(Ud.view(np.uint32) != g["U"].view(np.uint32))
    mb = 0.125                                                   # 131 072 bytes: 1 984 rows of 16 floats, three blocks and more
    monkeypatch.setenv("ENSTOP_AMD_P_BUDGET_MB", str(mb))
    Ur, Vr = amd.plsa_fit(X, k, g["sw"], arithmetic="reference", **kw)
    check_blocks(shared_info(amd), X, k, int(mb * (1 << 20)))
    same_bits(Ur, g["U"], "budget from the environment"); same_bits(Vr, g["V"], "budget from the environment")


# ------------------------------------------------------------------------------------------------------------------------
# one EM iteration on an engine of its own: E-step + M-step of the drivers, against the strict oracle's
# ------------------------------------------------------------------------------------------------------------------------
def oracle_iteration(X, U0, V0, sw, thresh=1e-32, update_v=True):
    from oracle.plsa_oracle import Oracle
    o = Oracle(variant="strict")
    r, c, v = coo_arrays(X)
    n, k = U0.shape
    P = np.zeros((X.nnz, k), np.float32)
    o.plsa_e_step(r, c, v, V0, U0, P, thresh)
    Vo, Uo = V0.copy(), U0.copy()
    nw, nd = np.zeros(k, np.float32), np.zeros(n, np.float32)
    if not update_v:
        o.plsa_refit_m_step(r, c, v, Vo, Uo, P, np.ones(n, np.float32), nd)
    elif sw is None:
        o.plsa_m_step(r, c, v, Vo, Uo, P, nw, nd)
    else:
        o.plsa_m_step_w_sample_weight(r, c, v, Vo, Uo, P, sw, nw, nd)
    return Uo, Vo


def engine_iteration(eng, U0, V0, sw, budget, thresh=1e-32, update_v=True):
    eng.set_arithmetic("reference")
    eng.set_factors(U0, V0)
    eng.set_p_budget(budget)
    drive = eng.fit if update_v else eng.refit
    iters, _ = drive(sw, n_iter=1, n_iter_per_test=1, tolerance=0.0, e_step_thresh=thresh, flags=0)
    assert iters == 1
    U, V = eng.get_factors()
    return U, V, eng.p_block_info()


_chain_want = {}


@pytest.mark.parametrize("mode", ["pairs", "serial"])
@pytest.mark.parametrize("weights", ["none", "powers_of_two", "negative"])
@pytest.mark.parametrize("k", [8, 70])
def test_chain_carry_on_tie_heavy_input(amd, k, weights, mode, monkeypatch):
    """norm_pwz handed from block to block (serial chain: the accumulators start at the carry; pairs: the float64 prefix and the
    walk's sum do) on input where a wrong hand-over shows: one-hot P(z|d) rows make P(z|w,d) one-hot, so every topic's chain sees
    long stretches of + 0.0 and small integer addends (ties all along), one count of 3e6 jumps several binades, and negative
    weights take the running sums through zero.  Five blocks and more, of sizes that are no multiple of a tile or a chunk.
    blocked = unblocked = oracle, bit for bit."""
    import scipy.sparse as sp
    monkeypatch.setenv("PLSA_REF_CHAIN", mode)
    rs = np.random.RandomState(k)
    n, m = 4000, 300
    X = sp.random(n, m, density=0.08, format="csr", random_state=rs, dtype=np.float64)
    X.data = rs.randint(1, 5, size=X.nnz).astype(np.float64)
    X = X.astype(np.float32)
    X.data[X.nnz // 2] = 3.0e6
    U0 = np.zeros((n, k), np.float32); U0[np.arange(n), rs.randint(0, k, size=n)] = 1.0
    V0 = np.full((k, m), 1.0 / m, np.float32)
    sw = {"none": None, "powers_of_two": (2.0 ** rs.randint(-2, 3, size=n)).astype(np.float32),
          "negative": (rs.randn(n) * np.where(np.arange(n) < n // 2, 1.0, 3.0)).astype(np.float32)}[weights]
    if (k, weights) not in _chain_want:
        _chain_want[k, weights] = oracle_iteration(X, U0, V0, sw)
    Uo, Vo = _chain_want[k, weights]
    budget = budget_for(X, k, 5)
    with amd.Engine() as eng:                                    # (PLSA_REF_CHAIN is read when a context is created)
        eng.upload_csr(X)
        U1, V1, info1 = engine_iteration(eng, U0, V0, sw, 0)
        assert info1["blocks"] == 1 and info1["budget"] == 0 and info1["largest_block_nnz"] == X.nnz, info1
        Ub, Vb, info = engine_iteration(eng, U0, V0, sw, budget)
        chain = eng.reference_chain_info()
    sizes = check_blocks(info, X, k, budget, at_least=5)
    assert all(s % 64 for s in sizes[:-1]) and all(s % 256 for s in sizes[:-1]), sizes
    same_bits(V1, Vo, "unblocked P(w|z)"); same_bits(U1, Uo, "unblocked P(z|d)")
    same_bits(Vb, Vo, "blocked P(w|z)"); same_bits(Ub, Uo, "blocked P(z|d)")
    if mode == "pairs":                                          # the walks of all blocks are counted: the unblocked run's chunks
        groups = (k + 63) // 64                                  # and every block's (PAIR_L = 256 addends), per 64 topics
        assert chain["chunks"] == groups * ((X.nnz + 255) // 256 + sum((s + 255) // 256 for s in sizes)), (chain, sizes)
        assert 0 < chain["slow_chunks"] <= chain["chunks"], chain       # (the first chunk of a chain from + 0.0 always goes the slow way)
    else:
        assert chain["chunks"] == 0 and chain["serial_chain_now"], chain


@pytest.mark.parametrize("heavy_min", ["16", None])
@pytest.mark.parametrize("k", [8, 70, 200])
def test_column_carry(amd, k, heavy_min, monkeypatch):
    """A word's accumulator handed from block to block in Vacc, through k_ref_col_pass and (from PLSA_REF_HEAVY_MIN entries on)
    k_ref_norm_chain<GATHER>: a word in every document (entries in every block), a word of the first third of the documents only
    (the later blocks must leave its sums alone), a word of ten leading documents, an empty column (zeros, written by the first
    block).  blocked = unblocked = oracle, with and without weights, and again after release_scratch."""
    import scipy.sparse as sp
    if heavy_min is None:
        monkeypatch.delenv("PLSA_REF_HEAVY_MIN", raising=False)
    else:
        monkeypatch.setenv("PLSA_REF_HEAVY_MIN", heavy_min)
    rs = np.random.RandomState(100 + k)
    n, m = 1500, 90
    X = sp.random(n, m, density=0.05, format="lil", random_state=rs, dtype=np.float64)
    X[:, 7] = 1.0
    X[:, 11] = 0.0; X[:n // 3, 11] = 2.0
    X[:, 30] = 0.0; X[:10, 30] = 1.0
    X[:, 20] = 0.0
    X = X.tocsr(); X.data = np.ceil(X.data * 3); X.eliminate_zeros(); X = X.astype(np.float32)
    counts = np.diff(X.tocsc().indptr)
    assert counts[7] == n and counts[11] == n // 3 and counts[30] == 10 and counts[20] == 0
    U0 = rs.rand(n, k); U0 /= U0.sum(1, keepdims=True)
    V0 = rs.rand(k, m); V0 /= V0.sum(1, keepdims=True)
    U0 = U0.astype(np.float32); V0 = V0.astype(np.float32)
    sw = (0.25 + rs.rand(n)).astype(np.float32)
    budget = budget_for(X, k, 4)
    want = {w: oracle_iteration(X, U0, V0, weights) for w, weights in (("plain", None), ("weighted", sw))}
    with amd.Engine() as eng:
        eng.upload_csr(X)
        for released in (False, True):
            if released:
                eng.release_scratch()
            for w, weights in (("plain", None), ("weighted", sw)):
                Uo, Vo = want[w]
                if not released:
                    U1, V1, _ = engine_iteration(eng, U0, V0, weights, 0)
                    same_bits(V1, Vo, "unblocked P(w|z), " + w); same_bits(U1, Uo, "unblocked P(z|d), " + w)
                Ub, Vb, info = engine_iteration(eng, U0, V0, weights, budget)
                sizes = check_blocks(info, X, k, budget, at_least=4)
                assert X.indptr[n // 3] <= sum(sizes[:-2]), "the word of the first third reaches into the last two blocks"
                same_bits(Vb, Vo, "blocked P(w|z), %s, released=%s" % (w, released))
                same_bits(Ub, Uo, "blocked P(z|d), %s, released=%s" % (w, released))
                assert not Vb[:, 20].any()


@pytest.mark.parametrize("row_tiled", ["0", "1"])
@pytest.mark.parametrize("k", [5, 64, 130])
def test_block_edges(amd, k, row_tiled, monkeypatch):
    """Where blocks begin and end: empty documents first, last and in a run that closes a block (the greedy cut puts a run of empty
    documents at the END of the block in front of it: their rows of P would begin where the block's end); a budget that is
    exactly the longest document's need (that document is a block of its own), one byte less (an error that names it), and a
    budget for all of P (one block).  Both document-pass kernels; fit and refit; same bits as the unblocked step and the oracle."""
    import scipy.sparse as sp
    monkeypatch.setenv("PLSA_REF_ROW_TILED", row_tiled)
    rs = np.random.RandomState(300 + k)
    n, m = 777, 210
    run = (250, 263)
    X = sp.random(n, m, density=0.04, format="lil", random_state=rs, dtype=np.float64)
    X[4, 0] = 1.0; X[6, 0] = 1.0
    X[5, :] = 1.0                                                  # one document with every word
    X[0, :] = 0.0; X[n - 1, :] = 0.0; X[9, :] = 0.0
    for d in range(*run):
        X[d, :] = 0.0
    X[run[1], 3] = 1.0
    X = X.tocsr(); X.data = np.ceil(X.data * 3); X.eliminate_zeros(); X = X.astype(np.float32)
    lens = np.diff(X.indptr)
    assert lens.max() == lens[5] == m and lens[0] == lens[n - 1] == 0 and not lens[run[0]:run[1]].any() and lens[run[1]] > 0
    kp = kp_of(k)
    U0 = rs.rand(n, k); U0 /= U0.sum(1, keepdims=True)
    V0 = rs.rand(k, m); V0 /= V0.sum(1, keepdims=True)
    U0 = U0.astype(np.float32); V0 = V0.astype(np.float32)
    sw = (0.25 + rs.rand(n)).astype(np.float32)
    Uo, Vo = oracle_iteration(X, U0, V0, sw)
    Ur, _ = oracle_iteration(X, U0, V0, None, update_v=False)
    # a budget of exactly the entries in front of the run: block 0 ends with the run, the document behind it opens block 1
    closing = 4 * kp * (int(X.indptr[run[0]]) + 64)
    assert plan_for(X, k, closing)[1][1] == run[1] and X.indptr[run[0]] >= m
    exact = 4 * kp * (m + 64)
    sizes, cuts = plan_for(X, k, exact)
    at = cuts.index(5)
    assert cuts[at + 1] == 6 and sizes[at] == m, "the longest document is not a block of its own"
    with amd.Engine() as eng:
        eng.upload_csr(X)
        U1, V1, _ = engine_iteration(eng, U0, V0, sw, 0)
        same_bits(V1, Vo, "unblocked P(w|z)"); same_bits(U1, Uo, "unblocked P(z|d)")
        for budget in (budget_for(X, k, 3), budget_for(X, k, 7), closing, exact):
            Ub, Vb, info = engine_iteration(eng, U0, V0, sw, budget)
            check_blocks(info, X, k, budget)
            same_bits(Vb, Vo, "P(w|z), budget %d" % budget); same_bits(Ub, Uo, "P(z|d), budget %d" % budget)
        assert info["largest_block_nnz"] == m
        for budget in (closing, exact):
            Ub, Vb, info = engine_iteration(eng, U0, V0, None, budget, update_v=False)
            check_blocks(info, X, k, budget)
            same_bits(Ub, Ur, "refit P(z|d), budget %d" % budget); same_bits(Vb, V0, "refit leaves P(w|z)")
        with pytest.raises(amd.DeviceError, match=r"document 5 has %d non-zeros.* %d bytes" % (m, exact)):
            engine_iteration(eng, U0, V0, sw, exact - 1)
        whole = 4 * kp * (X.nnz + 64)
        for budget in (whole, 3 * whole):
            Ub, Vb, info = engine_iteration(eng, U0, V0, sw, budget)
            assert info["blocks"] == 1 and info["largest_block_nnz"] == X.nnz and info["p_allocated_bytes"] <= budget, info
            same_bits(Vb, Vo, "one block P(w|z)"); same_bits(Ub, Uo, "one block P(z|d)")
        # budgets and loans do not mix
        eng.p_reserve(whole)
        with pytest.raises(amd.DeviceError, match="plsa_set_p_budget.*plsa_p_reserve"):
            engine_iteration(eng, U0, V0, sw, budget_for(X, k, 3))


def test_context_reuse(amd):
    """One context: a blocked fit, the budget taken away, a fit, a bootstrap resample, a blocked fit -- each returns what a fresh
    context returns for the same matrix, and the plan is the ACTIVE matrix' (the resample has other documents, other cuts)."""
    import scipy.sparse as sp
    rs = np.random.RandomState(77)
    n, m, k = 900, 160, 12
    X = sp.random(n, m, density=0.06, format="csr", random_state=rs, dtype=np.float64)
    X.data = rs.randint(1, 6, size=X.nnz).astype(np.float64)
    X = X.astype(np.float32)
    idx = np.sort(rs.randint(0, n, size=n)).astype(np.int64)
    Xb = X[idx]
    U0 = rs.rand(n, k); U0 /= U0.sum(1, keepdims=True)
    V0 = rs.rand(k, m); V0 /= V0.sum(1, keepdims=True)
    U0 = U0.astype(np.float32); V0 = V0.astype(np.float32)
    kw = dict(n_iter=7, n_iter_per_test=3, tolerance=0.0, e_step_thresh=1e-32)

    def fit(eng, budget):
        eng.set_factors(U0, V0)
        eng.set_p_budget(budget)
        iters, _ = eng.fit(None, flags=amd.PLSA_REFERENCE_SUMS, **kw)
        assert iters == 7
        return eng.get_factors() + (eng.p_block_info(),)

    def fresh(Xf, budget):
        with amd.Engine() as eng:
            eng.upload_csr(Xf)
            return fit(eng, budget)

    b_base, b_boot = budget_for(X, k, 5), budget_for(Xb, k, 5)
    want_base, want_boot = fresh(X, 0), fresh(Xb, 0)
    with amd.Engine() as eng:
        eng.upload_csr(X)
        for step, (Xa, budget, want) in enumerate([(X, b_base, want_base), (X, 0, want_base), (Xb, b_boot, want_boot), (X, b_base, want_base)]):
            if step == 2:
                eng.bootstrap(idx)
                A = eng.download_active_csr()
                assert A.shape == Xb.shape and np.array_equal(A.indptr, Xb.indptr)
            if step == 3:
                eng.bootstrap(None)
            U, V, info = fit(eng, budget)
            same_bits(U, want[0], "step %d P(z|d)" % step); same_bits(V, want[1], "step %d P(w|z)" % step)
            if budget:
                check_blocks(info, Xa, k, budget, at_least=5)
                fr = fresh(Xa, budget)
                same_bits(U, fr[0], "step %d against a fresh blocked context" % step)
                assert fr[2] == info
            else:
                assert info["blocks"] == 1 and info["budget"] == 0 and info["largest_block_nnz"] == Xa.nnz, info
    assert plan_for(X, k, b_base)[1] != plan_for(Xb, k, b_boot)[1]


def test_plan_follows_the_topic_count(amd):
    """The plan depends on kp (rows per block = budget / (4 kp) - 64): one context, one upload, one budget, a fit with k = 8 and
    then one with k = 64 -- the second runs in more, smaller blocks, P(z|w,d) stays inside the budget, and both return the bits of
    a fresh unbudgeted context; then k = 8 again."""
    import scipy.sparse as sp
    rs = np.random.RandomState(91)
    n, m = 800, 150
    X = sp.random(n, m, density=0.06, format="csr", random_state=rs, dtype=np.float64)
    X.data = rs.randint(1, 6, size=X.nnz).astype(np.float64)
    X = X.astype(np.float32)
    budget = budget_for(X, 8, 4)                                 # k = 64: an eighth of the rows per block
    assert 4 * 64 * (int(np.diff(X.indptr).max()) + 64) <= budget
    factors, want = {}, {}
    for k in (8, 64):
        U0 = rs.rand(n, k); U0 /= U0.sum(1, keepdims=True)
        V0 = rs.rand(k, m); V0 /= V0.sum(1, keepdims=True)
        factors[k] = (U0.astype(np.float32), V0.astype(np.float32))
        with amd.Engine() as eng:
            eng.upload_csr(X)
            want[k] = engine_iteration(eng, factors[k][0], factors[k][1], None, 0)
    with amd.Engine() as eng:
        eng.upload_csr(X)
        seen = []
        for k in (8, 64, 8):
            U, V, info = engine_iteration(eng, factors[k][0], factors[k][1], None, budget)
            check_blocks(info, X, k, budget)
            same_bits(U, want[k][0], "k = %d P(z|d)" % k); same_bits(V, want[k][1], "k = %d P(w|z)" % k)
            seen.append(info["blocks"])
    assert seen[1] > seen[0] == seen[2], seen


def test_a_refused_budget_leaves_no_plan_behind(amd):
    """A good budget, then one that the longest document does not fit: an error -- and the same error again for the same budget
    (the half-built plan of the failed call must not be taken for a plan), also when the first document is the one that fails;
    a budget below one row names the least usable budget; the good budget works again afterwards, same bits."""
    import scipy.sparse as sp
    rs = np.random.RandomState(92)
    n, m, k = 400, 120, 12
    X = sp.random(n, m, density=0.06, format="lil", random_state=rs, dtype=np.float64)
    X[300, :] = 1.0                                                # the longest document comes after several cuts
    X = X.tocsr(); X.data = np.ceil(X.data * 3); X = X.astype(np.float32)
    lens = np.diff(X.indptr)
    assert lens.argmax() == 300 and lens[300] == m
    U0 = rs.rand(n, k); U0 /= U0.sum(1, keepdims=True)
    V0 = rs.rand(k, m); V0 /= V0.sum(1, keepdims=True)
    U0 = U0.astype(np.float32); V0 = V0.astype(np.float32)
    good = budget_for(X, k, 4)
    small = 4 * kp_of(k) * (m + 64) - 1                           # document 300 misses it by one byte
    assert len(plan_for(X, k, small + 1)[0]) > 4 and plan_for(X, k, small + 1)[1].index(300) > 2
    first = 4 * kp_of(k) * (int(lens[0]) + 64) - 1                # ... and this one not even document 0 fits
    assert lens[0] > 0
    with amd.Engine() as eng:
        eng.upload_csr(X)
        U1, V1, _ = engine_iteration(eng, U0, V0, None, 0)
        Ug, Vg, info = engine_iteration(eng, U0, V0, None, good)
        check_blocks(info, X, k, good)
        same_bits(Ug, U1, "P(z|d)"); same_bits(Vg, V1, "P(w|z)")
        for budget, doc in ((small, 300), (small, 300), (first, 0), (first, 0)):
            with pytest.raises(amd.DeviceError, match=r"document %d has %d non-zeros" % (doc, lens[doc])):
                engine_iteration(eng, U0, V0, None, budget)
        for _ in range(2):
            with pytest.raises(amd.DeviceError, match=r"least usable budget at k = %d is %d bytes" % (k, 65 * kp_of(k) * 4)):
                engine_iteration(eng, U0, V0, None, 64 * kp_of(k) * 4)
        Ug, Vg, info = engine_iteration(eng, U0, V0, None, good)
        check_blocks(info, X, k, good)
        same_bits(Ug, U1, "P(z|d) after the refused budgets"); same_bits(Vg, V1, "P(w|z) after the refused budgets")
