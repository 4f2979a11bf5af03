"""Every grid-capped kernel beyond its first trip.

Almost every kernel of csrc/ is launched through grid_for(work, per_block, grid_cap) or a plan built from grid_cap
(plsa_launch_plan.hpp: row_pass, col_pass; plsa_tempered_plan.hpp: temper_grid) and walks its work with a stride loop.
grid_cap = CUs * PLSA_GRID_MULT, 128 workgroups per CU by default: at the sizes of the entry-by-entry suites every workgroup
makes at most one trip.  Here a context is created under PLSA_GRID_MULT=1 ("capped": one workgroup per CU) and

  1. held to the float64 restatements the uncapped suites use (test_pass_matrix.step64 and its bounds, tests/nmf_reference.py,
     the strict oracle for the reference arithmetic, NumPy for the builders), and
  2. compared with a context created with the knob unset ("free") on the same inputs, bit for bit wherever a sum is owned by
     a document, a column, an item or a chunk, whose number does not depend on the grid.

Sizes are derived, not written down: with C = the CU count (Engine.device_info) and p = the work one workgroup takes per
trip (from the lane shapes Engine.pass_info reports), a work count W wraps when W > 2 C p (three trips at least) and
W mod (C p) is neither 0 nor a multiple of p (a short last trip whose last workgroup is ragged).  `sizes` picks the
smallest n and m that do so for every walk over documents, columns and float4s of a factor at once, `capped_structure` then
chooses the length of its one long document so that the row items, the E-step's pieces and its 64-entry tiles do too.
One launch is NOT on C workgroups: k_col_reduce / k_col_reduce_norm run on reduce_grid = C + one workgroup per heavy column,
and their column loop strides by all of them; `capped_structure` grows m until the columns wrap on that grid, with the heavy
columns counted from the corpus itself, under each column setting the file uses (default, HEAVY_ENV, the small-grid cases).
(The heavy-column loop itself, h = block, block + reduce_grid, ..., cannot make a second trip: reduce_grid > n_heavy.)
An elementwise walk over rows that are whole workgroups (kp / 4 a multiple of 256) cannot be ragged inside a workgroup: only
its short last trip is asked for.  The flat E-step wraps up to k = 64 only (beyond, 131 072 non-zeros pass nnz k = 2e7); the
piecewise E-step wraps at every k.  PLSA_E_ROWS=1 is taken on trust: both E-step traversals time under the name "k_e_step".
test_every_case_wraps_three_times_with_a_ragged_tail restates that arithmetic on a CPU for C = 256 (the MI355X; the only
place a CU count is written down) through tests/launch_plan_host.cpp, the per-column sums on the reduce_grid that col_pass
returns; test_builder_cases_wrap does the same for upload, bootstrap, the initialisations and the generators.
That the cap is in force is read back, not assumed:
MemberBatch.info()["row_grid"] is the planned document-pass grid of a member context, which reads its knobs through the same
read_knobs.

What depends on the grid and what does not (read off the kernels):
    U, norm_pdz          one group per document (k_row_pass), or per row item and then per document in item order
                         (k_row_reduce): grid-independent.
    acc, V, norm_pwz     one partial row per column item (k_col_pass), added per column in item order (k_col_reduce /
                         k_col_reduce_norm, heavy columns in group order through LDS); norm_pwz from one float64 row per
                         CHUNK of 256 / lpn items in chunk order, or from NORM_BLOCKS = 256 slabs of words
                         (k_colsum_partial): chunk and slab counts do not depend on the grid.  Grid-independent.
    P(z|w,d)             one group (or wave tile) per entry: grid-independent.
    log-likelihood, NMF divergence    one float64 partial per WORKGROUP (ll_partials, nmf.obj), summed by k_ll_final: the
                         grouping of the terms follows the grid.  |capped - free| <= 2 nnz 2^-53 scale, scale the sum of the
                         terms' magnitudes (nnz - 1 additions on either side, each within 2^-53 of a partial sum <= scale).
    reference arithmetic every sum one accumulator in the reference's order, the likelihood included: bits.

Stride loops that carry a barrier or reuse LDS across trips, and why each is safe under a capped grid (read before the first
capped launch; the trip count must be the same for every thread of a workgroup that reaches the barrier):
    col_pass_body        one chunk per trip; chunk = c_lo + q, the bound c_hi and the stride nq come from blockIdx / gridDim /
                         xcd_lo only: uniform.  Groups beyond n_items skip the work, not block_colsum's barrier; the barrier
                         behind block_colsum keeps the next trip from rewriting scol before it is read.
    col_reduce_body      heavy columns: h = block, stride nblocks: uniform; the per-group item loop in between has no barrier;
                         the second barrier protects sacc from the next heavy column.  The per-column loop behind it has none.
                         The heavy loop runs in EVERY workgroup of the launch (workgroup b takes heavy column b, b + grid, ...):
                         reduce_grid = capped grid + n_heavy only adds workgroups, no heavy column depends on them.
    row_pass_body, k_loglik, k_score_rows, k_nmf_divergence      the document loop has no barrier (group_sum and the entry
                         broadcasts are shuffles inside one group of lanes, which enters a trip whole or not at all); the
                         block reduction of the likelihood partials comes after the loop, reached by all 256 threads.
    row_reduce_body      no barrier, no LDS.
    colsum_slab_body, norm_reduce_body, colsum_final_body, k_nmf_colsum_partial      the loop with the barriers runs over kp
                         in steps of 256: uniform; their grids are NORM_BLOCKS / norm_blocks, never the cap.
    k_e_step             one 64-entry tile per wave and trip, no LDS, no barrier; the wave's trip count is its own.
    k_ref_e_step_tiled, k_ref_row_pass_tiled      a wave owns its LDS tile; wave_lds_fence() between writing and reading it and
                         again before the next trip writes it; no workgroup barrier.
    k_synth_draw_topics  four documents per trip; `base` and its stride come from blockIdx / gridDim: uniform; waves beyond n
                         skip the work, not the three barriers; the last keeps tcdf from being rewritten early.
    k_v_normalise, k_nmf_h_finish, k_col_reduce_norm      one barrier after the LDS copy of the norms, before the stride loop.
None was found unsafe.

Needs a real MI355X for everything except the trip arithmetic.
"""
import contextlib
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT, coo_arrays
from test_fit_driver import KNOBS as DRIVER_KNOBS, PLSA_FUSED, PLSA_GRAPH
from test_launch_plan_host import program, call, ceil_div          # noqa: F401  (program: the sanitized host build, a fixture)
from test_pass_matrix import (step64, check, check_ll, lane_shape, U32, C_FACTOR, TINY_THRESH, EMPTY_DOCS, KNOBS as MATRIX_KNOBS,
                              e_step64, m_step64, loglik64, _coo)

U53 = 2.0 ** -53
CUS_MI355X = 256                 # the CPU restatement only: the GPU tests read the count from the device
K_CAPPED = [4, 6, 16, 32, 64, 100, 255, 512, 1024]           # the shapes (1,1) ... (64,4); k = 64 with its 8 x 2 document pass
K_FLAT_E_STEP = [4, 6, 16, 32, 64]      # where the flat E-step (64-entry tiles, 4 per workgroup) wraps within nnz k <= 2e7
KNOBS = sorted(set(DRIVER_KNOBS) | set(MATRIX_KNOBS) |
               {"PLSA_GRID_MULT", "PLSA_SMALL_GRID", "PLSA_E_ROWS", "PLSA_E_SEG", "PLSA_SORT_ROWS", "PLSA_ROW_XCD", "PLSA_ROW_SHAPE",
                "PLSA_CHUNKS_PER_LANE", "PLSA_ORDER_BAND", "PLSA_MT_STREAMS", "PLSA_MT_MIN_BLOCKS", "PLSA_MT_CHAIN"})
CAP = {"PLSA_GRID_MULT": "1"}


@contextlib.contextmanager
def knobs(env):
    """PLSA_* knobs are read when a context is created: exactly `env` of them set inside (PLSA_GRID_MULT and PLSA_SMALL_GRID
    among those cleared), the environment restored after"""
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


def make_engine(amd, env, capped, X=None):
    with knobs(dict(env, **CAP) if capped else env):
        eng = amd.Engine()
    if X is not None:
        eng.upload_csr(X)
    return eng


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b, what):
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=what)


def same_csr(A, B, what):
    for part in ("indptr", "indices"):
        np.testing.assert_array_equal(getattr(A, part), getattr(B, part), err_msg="%s: %s" % (what, part))
    same_bits(A.data.astype(np.float32), B.data.astype(np.float32), what + ": data")


# ------------------------------------------------------------------------------------------------
# sizing
# ------------------------------------------------------------------------------------------------
def trips(W, C, p):
    return ceil_div(ceil_div(W, p), C)


def wraps(W, C, p, unit=1):
    """three trips at least, the last one short, its last workgroup ragged -- where W, which comes in multiples of `unit`, can
    leave a workgroup ragged at all (a factor row of 1024 floats is 256 float4s: whole workgroups of an elementwise kernel)"""
    rem = W % (C * p)
    return W > 2 * C * p and rem != 0 and (unit % p == 0 or rem % p != 0)


def smallest(C, walks, start=0):
    """the smallest count (from `start` on) that wraps in every walk (scale, p): scale * count items of work, p per workgroup
    and trip"""
    count = max(start, max(2 * C * p // scale for scale, p in walks) + 1)
    for count in range(count, count + 4 * C * max(p for _, p in walks)):
        if all(wraps(scale * count, C, p, scale) for scale, p in walks):
            return count
    raise AssertionError("no count wraps in every walk of %r" % (walks,))


def per_block(k):
    kp, col, row = lane_shape(k)
    return kp, 256 // row[0], 256 // col[0]


@functools.lru_cache(maxsize=None)
def sizes(k, cus):
    """(n, the least m).  Documents: the document pass (256 / row_lpn per workgroup), k_loglik / k_score_rows / k_e_step_rows
    over whole documents (256 / lpn), the wave-per-row builders (4), the float4s of P(z|d) (k_temper: 256).  Words: the float4s
    of P(w|z) (k_v_normalise, k_temper, k_nmf_h_finish: 256) and k_col_reduce (256 / lpn) on a grid of C workgroups; its real
    grid has one more workgroup per heavy column, which depends on the corpus: capped_structure grows m until that wraps."""
    kp, p_row, p_col = per_block(k)
    n = smallest(cus, [(1, p_row), (1, p_col), (1, 4), (kp // 4, 256)])
    m = smallest(cus, [(1, p_col), (kp // 4, 256)])
    return n, m


LONG_DOC, HEAVY_WORD, UNUSED_WORD = 3, 5, 9
HEAVY_LEN, LONG_MIN = 600, 300
TINY_DOCS, N_TINY_WORDS = (11, 12, 13, 14), 4
ITEM_SEG = 16                    # PLSA_ROW_SEG and PLSA_E_SEG of the settings below
HEAVY_ITEMS_DEFAULT = 32         # csrc/plsa_hip.hip: heavy_items
HEAVY_ENV = {"PLSA_HEAVY_ITEMS": "4", "PLSA_COL_SEG": "8"}        # columns of more than 32 entries take a workgroup each
SMALL_GRID_SEG = 8               # PLSA_COL_SEG of the small-grid cases: the items can be counted


def col_item_len(nnz, cus, lpn):
    """plsa_launch_plan.hpp col_item_len without an override, restated (the CPU test holds it to the header)"""
    slots = cus * 32 * (64 // lpn)
    want = nnz // max(slots + slots // 4, 1)
    seg = 16
    while seg * 2 <= want and seg < 64:
        seg *= 2
    return seg


def column_settings(k, nnz, cus):
    """name -> (entries per column item, items beyond which a column is heavy) of the contexts this file creates"""
    return {"default": (col_item_len(nnz, cus, lane_shape(k)[1][0]), HEAVY_ITEMS_DEFAULT),
            "heavy": (int(HEAVY_ENV["PLSA_COL_SEG"]), int(HEAVY_ENV["PLSA_HEAVY_ITEMS"])),
            "small_grid": (SMALL_GRID_SEG, HEAVY_ITEMS_DEFAULT)}


def heavy_columns(X, seg, heavy_items):
    clens = np.diff(X.tocsc().indptr)
    return int(((clens + seg - 1) // seg > heavy_items).sum())


def reduce_grids(k, X, cus):
    """name -> the grid of k_col_reduce / k_col_reduce_norm (plan::col_pass: the capped grid over the columns plus one
    workgroup per heavy column; the column loop strides by ALL of them)"""
    p_col = per_block(k)[2]
    return {name: min(ceil_div(X.shape[1], p_col), cus) + heavy_columns(X, seg, heavy_items)
            for name, (seg, heavy_items) in column_settings(k, X.nnz, cus).items()}


def doc_lengths(k):
    """entries per ordinary document: enough for 131 072 non-zeros (the flat E-step's third trip at 256 CUs) up to k = 64,
    short beyond (nnz k stays below 2e7: the float64 step is computed on the host)"""
    return (3, 10) if k <= 16 else (6, 12) if k <= 64 else (3, 6)


def _structure(k, cus, lengths, n, m):
    kp, p_row, p_col = per_block(k)
    rs = np.random.RandomState(2000 + k)
    lo, hi = lengths or doc_lengths(k)
    lens = rs.randint(lo, hi + 1, n)
    lens[list(EMPTY_DOCS)] = 0
    lens[LONG_DOC] = 0
    r = np.repeat(np.arange(n, dtype=np.int64), lens)
    c = rs.randint(0, m, r.shape[0]).astype(np.int64)
    heavy = np.setdiff1d(rs.choice(n, HEAVY_LEN, replace=False), list(EMPTY_DOCS) + [LONG_DOC])
    tiny_words = np.arange(m - N_TINY_WORDS, m)
    tr, tc = np.meshgrid(TINY_DOCS, tiny_words, indexing="ij")
    r = np.concatenate([r, heavy, tr.ravel()])
    c = np.concatenate([c, np.full(heavy.shape[0], HEAVY_WORD), tc.ravel()])
    c[c == UNUSED_WORD] = UNUSED_WORD + 1
    keys = np.unique(r * m + c)
    base_lens = np.bincount(keys // m, minlength=n)
    base_items = int(((base_lens + ITEM_SEG - 1) // ITEM_SEG).sum())
    allowed = np.setdiff1d(np.arange(m), [UNUSED_WORD])
    for long_len in range(LONG_MIN, min(LONG_MIN + 1024, allowed.shape[0])):
        items = base_items + ceil_div(long_len, ITEM_SEG)
        nnz = keys.shape[0] + long_len
        ok = wraps(items, cus, p_row) and wraps(items, cus, p_col)
        if k in K_FLAT_E_STEP and lengths is None:
            ok = ok and wraps(ceil_div(nnz, 64), cus, 4) and nnz % 64 != 0
        if ok:
            break
    else:
        raise AssertionError("no long-document length makes the items wrap at k=%d" % k)
    keys = np.union1d(keys, LONG_DOC * m + rs.choice(allowed, long_len, replace=False))
    x = rs.randint(1, 8, size=keys.shape[0]).astype(np.float32)
    pick = rs.choice(keys.shape[0], 60, replace=False)
    x[pick[:40]] = 0.0                                            # stored zeros
    x[pick[40:]] = np.resize(np.array([256, 300, 2.5, 4000, 0.75], np.float32), 20)
    X = sp.csr_matrix((x, (keys // m, keys % m)), shape=(n, m))
    assert X.nnz == keys.shape[0] and (X.data == 0).sum() == 40
    return X


@functools.lru_cache(maxsize=None)
def capped_structure(k, cus, lengths=None):
    """The corpus of one topic count in the style of test_pass_matrix.matrix_corpus: two empty documents, a word that never
    occurs, a word in 600 documents (heavy under the default 32 items of 16 entries, and under HEAVY_ENV with the other columns
    of more than 32 entries), one long document whose length is chosen so that the 16-entry row items / E-step pieces and
    (k <= 64) the 64-entry tiles wrap as well, stored zeros, a few escaped counts, and the block of TINY_DOCS x the last four
    words.  n is `sizes`'; m starts there and grows until the columns wrap on k_col_reduce's REAL grid, C + the heavy columns
    of this very corpus, under every column setting of the file."""
    kp, p_row, p_col = per_block(k)
    n, m = sizes(k, cus)
    for _ in range(8):
        X = _structure(k, cus, lengths, n, m)
        grids = reduce_grids(k, X, cus)
        if all(wraps(m, G, p_col) for G in grids.values()):
            return X
        m = smallest(cus, [(1, p_col), (kp // 4, 256)], start=2 * (max(grids.values()) + 4) * p_col + 1)
    raise AssertionError("the columns of k=%d do not wrap on the real reduce grid" % k)


@functools.lru_cache(maxsize=None)
def capped_corpus(k, cus, lengths=None):
    """(X, U0, V0, sw): capped_structure with matrix_corpus' factors -- the TINY block's products lie near 2^-139"""
    X = capped_structure(k, cus, lengths)
    n, m = X.shape
    rs = np.random.RandomState(3000 + k)
    U = (rs.rand(n, k) + 0.05).astype(np.float64)
    U /= U.sum(1, keepdims=True)
    V = (rs.rand(k, m) + 0.05).astype(np.float64)
    V /= V.sum(1, keepdims=True)
    U, V = U.astype(np.float32), V.astype(np.float32)
    U[list(TINY_DOCS)] = (2.0 ** -69 * (0.7 + 0.3 * rs.rand(len(TINY_DOCS), k))).astype(np.float32)
    V[:, m - N_TINY_WORDS:] = (2.0 ** -70 * (0.7 + 0.3 * rs.rand(k, N_TINY_WORDS))).astype(np.float32)
    sw = (0.5 + rs.rand(n)).astype(np.float32)
    for a in (U, V, sw):
        a.setflags(write=False)
    return X, U, V, sw


def items_of(lens, seg):
    return int(((np.asarray(lens) + seg - 1) // seg).sum())


def walks_of(k, X, cus):
    """name -> (work count, work per workgroup and trip, what the count is a multiple of, workgroups of the capped launch) of
    every capped walk of case 1"""
    kp, p_row, p_col = per_block(k)
    n, m = X.shape
    items = items_of(np.diff(X.indptr), ITEM_SEG)
    out = {"k_row_pass, k_row_reduce (documents)": (n, p_row, 1, cus),
           "k_loglik, k_score_rows (documents)": (n, p_col, 1, cus),
           "k_expand_rows (documents, a wave each)": (n, 4, 1, cus),
           "k_temper (float4s of P(z|d))": (n * kp // 4, 256, kp // 4, cus),
           "k_row_pass (row items of 16)": (items, p_row, 1, cus),
           "k_e_step_rows (pieces of 16)": (items, p_col, 1, cus),
           "k_v_normalise, k_temper (float4s of P(w|z))": (m * kp // 4, 256, kp // 4, cus)}
    for name, G in reduce_grids(k, X, cus).items():
        out["k_col_reduce (columns, %s)" % name] = (m, p_col, 1, G)
    if k in K_FLAT_E_STEP:
        out["k_e_step (64-entry tiles)"] = (ceil_div(X.nnz, 64), 4, 1, cus)
    return out


# column pass under PLSA_SMALL_GRID=1 (case 2): (k, entries per document); PLSA_COL_SEG pinned so that the items can be counted
SMALL_GRID_CASES = [(64, (6, 12)), (100, (6, 12))]


def chunks_of(k, X, seg):
    items = items_of(np.diff(X.tocsc().indptr), seg)
    gpb = per_block(k)[2]
    return items, ceil_div(items, gpb), gpb


def overlap_full_limit():
    """the default of PLSA_OVERLAP_FULL_LIMIT, read from the context's declaration"""
    text = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_hip.hip")).read()
    return float(re.search(r"double overlap_full_limit = ([0-9.e+]+);", text).group(1))


# reference arithmetic (case 3): 8 lanes per document / column, 32 of either per workgroup; 64-entry tiles, 2 per workgroup
K_REF = 8


@functools.lru_cache(maxsize=None)
def ref_corpus(cus):
    n = smallest(cus, [(1, 32), (1, 4)])
    rs = np.random.RandomState(77)
    lens = rs.randint(6, 13, n)
    lens[5] = 0
    r = np.repeat(np.arange(n, dtype=np.int64), lens)
    keys = np.unique(r * n + rs.randint(0, n, r.shape[0]))
    while not (wraps(keys.shape[0], cus, 256) and wraps(ceil_div(keys.shape[0], 64), cus, 2)):
        keys = keys[:-1]
    X = sp.csr_matrix((rs.randint(1, 6, keys.shape[0]).astype(np.float32), (keys // n, keys % n)), shape=(n, n))
    U = rs.rand(n, K_REF); U /= U.sum(1, keepdims=True)
    V = rs.rand(K_REF, n); V /= V.sum(1, keepdims=True)
    return X, U.astype(np.float32), V.astype(np.float32), (0.25 + rs.rand(n)).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# CPU: every case wraps
# ------------------------------------------------------------------------------------------------
def test_the_wrap_rule():
    C, p = 256, 16
    assert not wraps(2 * C * p, C, p) and wraps(2 * C * p + 1, C, p) and trips(2 * C * p + 1, C, p) == 3
    assert not wraps(3 * C * p, C, p) and not wraps(2 * C * p + 5 * p, C, p) and wraps(2 * C * p + 5 * p + 3, C, p)
    assert wraps(2 * C + 1, C, 1) and not wraps(3 * C, C, 1)
    assert smallest(C, [(1, 16)]) == 2 * C * 16 + 1 and smallest(C, [(1, 16), (1, 32)]) == 2 * C * 32 + 1


def check_walks(program, walks, C, tag):
    """every walk against grid_for of the header at cap C; the per-column sums (a grid beyond the cap) against the wrap rule on
    the grid they are given"""
    for name, (W, p, unit, G) in walks.items():
        assert wraps(W, G, p, unit) and trips(W, G, p) >= 3, (tag, name, W, p, G)
        (grid,), = call(program, "grid_for", [(W, p, C)])
        assert grid == C and G >= C, (tag, name, W, p, grid)
        assert ceil_div(W, G * p) >= 3 and W % (G * p) != 0 and ((W % (G * p)) % p != 0 or unit % p == 0), (tag, name, W, p, G)


@pytest.mark.parametrize("k", K_CAPPED)
def test_every_case_wraps_three_times_with_a_ragged_tail(program, k):
    """The arithmetic of this file for 256 CUs (an MI355X) against plsa_launch_plan.hpp run on a CPU at grid_cap = 256: every
    walk of every case makes three trips at least and ends in a short trip with a ragged last workgroup -- the per-column sums
    on the reduce_grid that col_pass returns for the default, the heavy and the small-grid column settings."""
    C = CUS_MI355X
    kp, p_row, p_col = per_block(k)
    X = capped_structure(k, C)
    n, m = X.shape
    assert n == sizes(k, C)[0] and m >= sizes(k, C)[1] and X.nnz * k <= 2e7
    lens, clens = np.diff(X.indptr), np.diff(X.tocsc().indptr)
    assert all(lens[d] == 0 for d in EMPTY_DOCS) and clens[UNUSED_WORD] == 0
    assert lens[LONG_DOC] >= LONG_MIN and lens[LONG_DOC] == lens.max() and clens[HEAVY_WORD] >= HEAVY_LEN - 3
    walks = walks_of(k, X, C)
    assert ("k_e_step (64-entry tiles)" in walks) == (k in K_FLAT_E_STEP)
    check_walks(program, walks, C, k)
    # the plans the passes launch from: the document pass over documents and over row items ...
    items = items_of(lens, ITEM_SEG)
    (g_doc, r_doc), (g_item, r_item) = call(program, "row_pass", [(n, 0, 0, 256 // p_row, C, 0), (n, items, 1, 256 // p_row, C, 0)])
    assert g_doc == r_doc == g_item == r_item == C and items > n - len(EMPTY_DOCS)
    # ... and the column tail: the item length and the grid come from the header, the heavy columns from the corpus
    (seg_default,), = call(program, "col_item_len", [(X.nnz, C, 256 // p_col, 0)])
    settings = column_settings(k, X.nnz, C)
    assert settings["default"] == (seg_default, HEAVY_ITEMS_DEFAULT)
    for name, (seg, heavy_items) in settings.items():
        n_heavy = heavy_columns(X, seg, heavy_items)
        assert n_heavy >= 1 and ceil_div(int(clens[HEAVY_WORD]), seg) > heavy_items, (k, name, n_heavy)
        (_, reduce_grid, _), = call(program, "col_pass", [(items_of(clens, seg), m, 256 // p_col, n_heavy, C)])
        assert reduce_grid == C + n_heavy == walks["k_col_reduce (columns, %s)" % name][3], (k, name, reduce_grid)
        assert ceil_div(m, reduce_grid * p_col) >= 3 and (m % (reduce_grid * p_col)) % p_col != 0, (k, name, m, reduce_grid)
    # uncapped (128 workgroups per CU) none of these wraps: what the free context runs
    (g_free, _), = call(program, "row_pass", [(n, 0, 0, 256 // p_row, 128 * C, 0)])
    assert g_free == ceil_div(n, p_row) and g_free > C


def bootstrap_rows(cus):
    """rows of the resample: k_boot_gather walks n_out + 1 row pointers, a wave each"""
    return smallest(cus, [(1, 4)]) + 36


def synthetic_sizes(cus):
    """(documents, words, target tokens): k_synth_draw / k_synth_draw_topics a wave per document, k_synth_heads / k_synth_emit a
    thread per token"""
    n = smallest(cus, [(1, 4)]) + 2 * cus * 4
    return n, 3000, max(40 * n, 3 * 256 * cus + 999)


K_BUILDERS = 16                  # upload, bootstrap and the initialisations run on this topic count's corpus


def builder_walks(cus):
    X = capped_structure(K_BUILDERS, cus)
    n, m = X.shape
    n_synth, _, target = synthetic_sizes(cus)
    return {"k_validate_csr, k_iota, k_csc_gather (entries)": (X.nnz, 256, 1, cus),
            "k_expand_rows, k_init_rows (documents, a wave each)": (n, 4, 1, cus),
            "k_boot_gather (row pointers of the resample)": (bootstrap_rows(cus) + 1, 4, 1, cus),
            "k_mt_scale_v (cells of P(w|z))": (K_BUILDERS * m, 256, K_BUILDERS, cus),
            "k_synth_draw, k_synth_draw_topics (documents)": (n_synth, 4, 1, cus),
            "k_synth_heads, k_synth_emit (tokens)": (target, 256, 1, cus)}


def test_builder_cases_wrap(program):
    check_walks(program, builder_walks(CUS_MI355X), CUS_MI355X, "builders")


@pytest.mark.parametrize("k, lengths", SMALL_GRID_CASES)
def test_small_grid_cases_wrap_and_stay_small(k, lengths):
    C = CUS_MI355X
    X = capped_structure(k, C, lengths)
    n, m = X.shape
    kp = per_block(k)[0]
    items, chunks, gpb = chunks_of(k, X, SMALL_GRID_SEG)
    assert X.nnz * kp < overlap_full_limit() == 2e9                   # PLSA_SMALL_GRID applies below the limit only
    assert chunks > 2 * C and chunks % C != 0 and items % gpb != 0   # three trips of one chunk each, the last chunk ragged
    assert chunks // 8 > 2 * (C // 8)                                 # ... and with the chunks split over the 8 XCDs
    assert chunks >= 64 and n * kp * 4 > 2 << 20                      # the split's own conditions (plan::xcd_split)
    n_heavy = heavy_columns(X, SMALL_GRID_SEG, HEAVY_ITEMS_DEFAULT)
    assert n_heavy >= 1 and wraps(m, C + n_heavy, gpb)                # the per-column sums on C + n_heavy workgroups
    assert lane_shape(64)[1] == (16, 1) and lane_shape(100)[1] == (16, 2)


def test_reference_corpus_wraps():
    C = CUS_MI355X
    X, _, _, _ = ref_corpus(C)
    n = X.shape[0]
    assert wraps(n, C, 32) and wraps(X.nnz, C, 256) and wraps(ceil_div(X.nnz, 64), C, 2) and np.diff(X.indptr)[5] == 0
    assert n < 300000                                                 # k_ref_row_pass, not its tiled form (ref_plan::row_tiled)


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


@pytest.fixture(scope="module")
def cus(amd):
    with amd.Engine() as eng:
        return eng.device_info()["cus"]


@pytest.fixture(scope="module")
def pair(amd):
    """one capped and one free context with no other knob set"""
    capped, free = make_engine(amd, {}, True), make_engine(amd, {}, False)
    yield capped, free
    capped.close()
    free.close()


@pytest.fixture(scope="module")
def worst():
    out = {}
    yield out
    if out:
        print("\ncapped grids: worst error / bound per kernel family: " +
              ", ".join("%s %.3g" % (key, v) for key, v in sorted(out.items())))


def keep_worst(worst, family, ratios):
    for key, v in ratios.items():
        name = "%s %s" % (family, key.split(" ")[0])
        worst[name] = max(worst.get(name, 0.0), v)


def ll_gap(a, b, nnz, scale, what):
    bound = 2.0 * nnz * U53 * scale
    assert abs(a - b) <= bound, "%s: %r against %r, apart by %.3g, bound %.3g" % (what, a, b, abs(a - b), bound)


@pytest.mark.gpu
def test_the_cap_is_in_force(amd, cus):
    """a member context reads its knobs through the engine's read_knobs: its planned document-pass grid is the CU count under
    PLSA_GRID_MULT=1 and one workgroup per 256 / row_lpn documents without"""
    k = 32
    X, U0, V0, _ = capped_corpus(k, cus)
    n = X.shape[0]
    p_row = per_block(k)[1]
    grids = {}
    for capped in (True, False):
        with knobs(CAP if capped else {}):
            eng = amd.Engine()
            eng.upload_csr(X)
            batch = eng.member_batch(2)
        try:
            for j in range(2):
                batch.prepare(j, k, U=U0, V=V0)
            batch.fit(2, n_iter=1, n_iter_per_test=5, tolerance=0.0, e_step_thresh=1e-32, flags=PLSA_FUSED)
            assert batch.last_batched == 2
            grids[capped] = [batch.info(j)["row_grid"] for j in range(2)]
            assert batch.member(0).pass_info()["row"][0] == 256 // p_row
        finally:
            eng.close()
    assert grids[True] == [cus, cus] and grids[False] == [ceil_div(n, p_row)] * 2 and ceil_div(n, p_row) > 2 * cus, grids


# ---- case 1: one EM step, every default lane shape ----------------------------------------------------------------
STEP_SETTINGS = {
    "default": {},
    "arrays": {"PLSA_PACKED": "0"},
    "row_items": {"PLSA_ROW_ITEMS": "1", "PLSA_ROW_SEG": str(ITEM_SEG)},
    "heavy": HEAVY_ENV,
    "e_rows": {"PLSA_E_ROWS": "1", "PLSA_E_SEG": str(ITEM_SEG)},
}
FUSED = ("default", "arrays", "row_items", "heavy")
KERNELS = ("default", "e_rows")         # (the E-step and the passes from P read the two index arrays whatever PLSA_PACKED says)
COMBOS = [(weighted, thresh) for weighted in (False, True) for thresh in (1e-32, 0.0)]


def fused_step(eng, U0, V0, sw, thresh, m):
    eng.set_factors(U0, V0)
    out = dict(ll=eng.em_accumulate(sw, thresh, want_ll=True))
    out["acc"] = eng.accumulator_get().reshape(m, -1)
    eng.em_finish()
    out["U"], out["V"] = eng.get_factors()
    eng.set_factors(U0, V0)                      # ... and the pass without the likelihood: another instantiation
    eng.em_accumulate(sw, thresh, want_ll=False)
    eng.em_finish()
    out["U_plain"], out["V_plain"] = eng.get_factors()
    return out


def kernel_step(eng, U0, V0, sw, thresh):
    eng.set_factors(U0, V0)
    out = dict(ll=eng.log_likelihood(sw), P=eng.e_step(thresh))
    out["norm_pwz"], out["norm_pdz"] = eng.m_step(sw)
    out["U"], out["V"] = eng.get_factors()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k", K_CAPPED)
def test_one_em_step_capped(amd, cus, worst, k):
    """E-step to a materialised P, M-step from P, fused step (with and without the riding likelihood), stand-alone likelihood,
    with and without weights, thresholds on both sides of TINY_THRESH, packed and unpacked, row items, heavy columns, the
    piecewise E-step: the capped context against the float64 step with test_pass_matrix' bounds, and bit for bit (the
    likelihood: within the re-association bound) against the free context."""
    X, U0, V0, sw_doc = capped_corpus(k, cus)
    n, m = X.shape
    kp, col_shape, row_shape = lane_shape(k)
    for name, (W, p, unit, G) in walks_of(k, X, cus).items():
        assert wraps(W, G, p, unit), (name, W, p, G)
    settings = column_settings(k, X.nnz, cus)
    clens = np.diff(X.tocsc().indptr)
    rows, cols, x = _coo(X)
    P64 = {thresh: e_step64(rows, cols, U0, V0, thresh) for thresh in (1e-32, 0.0)}
    LL64 = {weighted: loglik64(rows, cols, x, U0, V0, sw_doc if weighted else None) for weighted in (False, True)}
    L_row, L_col = max(2, int(np.diff(X.indptr).max())), max(2, int(np.diff(X.tocsc().indptr).max()))
    b_row, b_col, b_p = C_FACTOR * (L_row + k) * U32, C_FACTOR * (L_col + k) * U32, C_FACTOR * (2 + k) * U32
    want = {}
    for weighted, thresh in COMBOS:
        U1, V1, npwz, npdz = m_step64(rows, cols, x, P64[thresh], n, m, sw_doc if weighted else None)
        want[weighted, thresh] = dict(U=U1, V=V1, norm_pwz=npwz, norm_pdz=npdz, acc=V1 * npwz[:, None])
    ratios = {}
    p_checked = set()
    for name, env in STEP_SETTINGS.items():
        capped, free = make_engine(amd, env, True, X), make_engine(amd, env, False, X)
        try:
            for weighted, thresh in COMBOS:
                sw = sw_doc if weighted else None
                ref = want[weighted, thresh]
                ll_want, ll_scale = LL64[weighted]
                tag = "k=%d %s sw=%d thresh=%g" % (k, name, weighted, thresh)
                if name in FUSED:
                    got, other = fused_step(capped, U0, V0, sw, thresh, m), fused_step(free, U0, V0, sw, thresh, m)
                    info = capped.pass_info()
                    assert info["col"][:2] == col_shape and info["row"][:2] == row_shape, (tag, info)
                    assert capped.packed_info() == free.packed_info() == \
                        (dict(csr="arrays", csc="arrays") if name == "arrays" else dict(csr="packed", csc="packed")), tag
                    check("U fused " + tag, got["U"], ref["U"], b_row, ratios)
                    check("V fused " + tag, got["V"], ref["V"], b_col, ratios)
                    assert got["acc"].shape == (m, kp) and not got["acc"][:, k:].any(), tag
                    check("acc fused " + tag, got["acc"][:, :k].T, ref["acc"], b_col, ratios)
                    check_ll("LL fused " + tag, got["ll"], ll_want, ll_scale, k, ratios)
                    for key in ("U", "V", "acc", "U_plain", "V_plain"):
                        same_bits(got[key], other[key], "%s: %s capped against free" % (tag, key))
                    same_bits(got["U"], got["U_plain"], tag + ": U with and without the riding likelihood")
                    same_bits(got["V"], got["V_plain"], tag + ": V with and without the riding likelihood")
                    ll_gap(got["ll"], other["ll"], X.nnz, ll_scale, tag + ": riding likelihood capped against free")
                    for d in EMPTY_DOCS:
                        assert not got["U"][d].any(), tag
                    assert not got["V"][:, UNUSED_WORD].any(), tag
                if name in KERNELS:
                    got, other = kernel_step(capped, U0, V0, sw, thresh), kernel_step(free, U0, V0, sw, thresh)
                    if (name, thresh) not in p_checked:
                        p_checked.add((name, thresh))
                        check("P kernels " + tag, got["P"], P64[thresh], b_p, ratios)
                    check("U kernels " + tag, got["U"], ref["U"], b_row, ratios)
                    check("V kernels " + tag, got["V"], ref["V"], b_col, ratios)
                    check("norm_pwz kernels " + tag, got["norm_pwz"], ref["norm_pwz"], b_col, ratios)
                    check("norm_pdz kernels " + tag, got["norm_pdz"], ref["norm_pdz"], b_row, ratios)
                    check_ll("LL kernels " + tag, got["ll"], ll_want, ll_scale, k, ratios)
                    for key in ("P", "U", "V", "norm_pwz", "norm_pdz"):
                        same_bits(got[key], other[key], "%s: %s capped against free" % (tag, key))
                    ll_gap(got["ll"], other["ll"], X.nnz, ll_scale, tag + ": k_loglik capped against free")
            if name in FUSED:
                # the heavy columns are there: the device cut the columns into the items the restatement counts them from
                seg, heavy_items = settings["heavy" if name == "heavy" else "default"]
                for eng in (capped, free):
                    bal = eng.balance_info()
                    assert (bal["item_entries"], bal["n_items"]) == (seg, items_of(clens, seg)), (name, bal)
                assert heavy_columns(X, seg, heavy_items) >= 1
            if name == "row_items":
                capped.timing(True)
                capped.timing_reset()
                fused_step(capped, U0, V0, None, 1e-32, m)
                assert "k_row_reduce" in capped.timing_report()
                capped.timing(False)
        finally:
            capped.close()
            free.close()
    keep_worst(worst, "EM step:", ratios)
    print("\nk=%d rows %s cols %s, %d x %d, %d entries: worst error / bound %.3g (%s)" % (
        k, row_shape, col_shape, n, m, X.nnz, max(ratios.values()), max(ratios, key=ratios.get)))


# ---- case 2: the capped column pass --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("k, lengths", SMALL_GRID_CASES)
def test_column_pass_under_small_grid(amd, cus, worst, k, lengths, split):
    """PLSA_SMALL_GRID=1: the column pass itself on one workgroup per CU (every workgroup walks three chunks or more, with the
    chunks split over the XCDs and without): the production step (fit, n_iter = 1: k_col_pass, the norm from its chunk rows,
    k_col_reduce_norm) and the accumulate / finish step, against the float64 step and bit for bit against the free context."""
    X, U0, V0, sw_doc = capped_corpus(k, cus, lengths)
    n, m = X.shape
    kp = per_block(k)[0]
    items, chunks, gpb = chunks_of(k, X, SMALL_GRID_SEG)
    assert chunks > 2 * cus and chunks % cus != 0 and items % gpb != 0 and X.nnz * kp < overlap_full_limit()
    n_heavy = heavy_columns(X, SMALL_GRID_SEG, HEAVY_ITEMS_DEFAULT)
    assert n_heavy >= 1 and wraps(m, cus + n_heavy, gpb)              # k_col_reduce_norm on its real grid
    env ={"PLSA_COL_SEG": str(SMALL_GRID_SEG), "PLSA_XCD_SPLIT": split}
    small = make_engine(amd, dict(env, PLSA_SMALL_GRID="1"), True, X)
    free = make_engine(amd, env, False, X)
    ratios = {}
    try:
        for weighted, thresh in ((False, 1e-32), (True, 0.0)):
            sw = sw_doc if weighted else None
            ref = step64(X, U0, V0, thresh, sw)
            b_row, b_col = C_FACTOR * (ref["L_row"] + k) * U32, C_FACTOR * (ref["L_col"] + k) * U32
            tag = "k=%d split=%s sw=%d thresh=%g" % (k, split, weighted, thresh)
            out = []
            for eng in (small, free):
                eng.set_factors(U0, V0)
                iters, trace = eng.fit(sw, n_iter=1, n_iter_per_test=5, tolerance=0.0, e_step_thresh=thresh, flags=PLSA_FUSED)
                assert iters == 1
                info = eng.fit_info()
                assert info["xcd_split"] == (split == "1") and info["col_tail"] == "sweep", (tag, info)
                assert eng.balance_info()["n_items"] == items and eng.balance_info()["item_entries"] == SMALL_GRID_SEG
                fitted = eng.get_factors()
                step = fused_step(eng, U0, V0, sw, thresh, m)
                step["U_fit"], step["V_fit"] = fitted
                out.append(step)
            got, other = out
            check("U " + tag, got["U_fit"], ref["U"], b_row, ratios)
            check("V " + tag, got["V_fit"], ref["V"], b_col, ratios)
            check("V_finish " + tag, got["V"], ref["V"], b_col, ratios)
            check("acc " + tag, got["acc"][:, :k].T, ref["V"] * ref["norm_pwz"][:, None], b_col, ratios)
            for key in ("U", "V", "acc", "U_fit", "V_fit"):
                same_bits(got[key], other[key], "%s: %s under PLSA_SMALL_GRID=1 against free" % (tag, key))
    finally:
        small.close()
        free.close()
    keep_worst(worst, "small grid:", ratios)


# ---- case 3: drivers that launch from the same plans ----------------------------------------------------------------
K_DRIVER = 64


# loop forms of test_fit_driver.FORMS: knobs -> (pipelined, replays graphs)
FIT_FORMS = {"default": ({}, True, False), "no_pipeline": ({"PLSA_PIPELINE": "0"}, False, False),
             "graph": ({"PLSA_GRAPH": "1"}, False, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FIT_FORMS))
def test_fit_and_refit_capped_against_free(amd, cus, form):
    """plsa_fit (fused) and plsa_refit over a fixed number of iterations with no test that could stop them: same factors"""
    X, U0, V0, sw = capped_corpus(K_DRIVER, cus)
    env, pipelined, graphs = FIT_FORMS[form]
    out = []
    for capped in (True, False):
        eng = make_engine(amd, env, capped, X)
        try:
            eng.set_factors(U0, V0)
            iters, _ = eng.fit(sw, n_iter=4, n_iter_per_test=10, tolerance=0.0, e_step_thresh=1e-32, flags=PLSA_FUSED)
            info = eng.fit_info()
            assert iters == 4 and info["fused"] and info["pipelined"] == pipelined and (info["graph_launches"] > 0) == graphs, info
            fit = eng.get_factors()
            eng.set_factors(U0, V0)
            iters, _ = eng.refit(sw, n_iter=3, n_iter_per_test=10, tolerance=0.0, e_step_thresh=1e-32, flags=PLSA_FUSED)
            assert iters == 3
            out.append(fit + eng.get_factors())
        finally:
            eng.close()
    for a, b, what in zip(out[0], out[1], ("fit U", "fit V", "refit U", "refit V")):
        same_bits(a, b, "%s: %s capped against free" % (form, what))
    same_bits(out[0][3], V0, "refit moved the topics")


@pytest.mark.gpu
def test_score_rows_capped(amd, cus, pair, worst):
    """per-document values are a group's own: bit for bit; their total against the float64 likelihood with check_ll"""
    k = K_DRIVER
    X, U0, V0, sw = capped_corpus(k, cus)
    rows, cols, x = _coo(X)
    want, scale = loglik64(rows, cols, x, U0, V0, sw)
    out = []
    for eng in pair:
        eng.upload_csr(X)
        eng.set_factors(U0, V0)
        out.append(eng.score_rows(None, sw) + (eng.log_likelihood(sw),))
    for a, b, what in zip(out[0][:3], out[1][:3], ("ll", "tokens", "unscored")):
        same_bits(a, b, "score_rows %s capped against free" % what)
    ratios = {}
    check_ll("total", float(out[0][0].sum()), want, scale, k, ratios)
    ll_gap(out[0][3], out[1][3], X.nnz, scale, "k_loglik capped against free")
    ll_gap(float(out[0][0].sum()), out[0][3], X.nnz, scale, "sum of the rows against k_loglik")
    assert not out[0][0][list(EMPTY_DOCS)].any()
    keep_worst(worst, "score_rows:", ratios)


@pytest.mark.gpu
def test_one_tempered_iteration_capped(amd, cus, pair):
    """k_temper over both side tables (each more than 2 C 256 float4s), then the fused iteration on them"""
    k = K_DRIVER
    X, U0, V0, sw = capped_corpus(k, cus)
    kp = per_block(k)[0]
    assert wraps(X.shape[0] * kp // 4, cus, 256, kp // 4) and wraps(X.shape[1] * kp // 4, cus, 256, kp // 4)
    out = []
    for eng in pair:
        eng.upload_csr(X)
        eng.set_factors(U0, V0)
        tables = eng.temper_factors(0.9)
        iters, trace = eng.fit_tempered(0.9, sw, n_iter=1, n_iter_per_test=1, tolerance=0.0, e_step_thresh=1e-32, flags=PLSA_FUSED,
                                        trace=True)
        assert iters == 1
        out.append(tables + eng.get_factors())
    for a, b, what in zip(out[0], out[1], ("P(z|d)^beta", "P(w|z)^beta", "U", "V")):
        same_bits(a, b, "tempered %s capped against free" % what)


@pytest.mark.gpu
def test_one_online_step_capped(amd, cus):
    """the blend and k_v_normalise run on the block context's stream with the block context's cap"""
    k = K_DRIVER
    X, U0, V0, sw = capped_corpus(k, cus)
    m = X.shape[1]
    out = []
    for capped in (True, False):
        home, eng = make_engine(amd, {}, capped), make_engine(amd, {}, capped, X)
        try:
            with amd.OnlineState(home, m, k) as state:
                state.set_topics(V0)
                eng.set_factors(U0, np.ascontiguousarray(V0[::-1]))
                ll = state.step(eng, 0.25, 1.5, 1, sw, 1e-32, want_ll=True, flags=PLSA_FUSED)
                assert np.isfinite(ll)
                out.append((state.get_topics(), state.statistic_get(), eng.get_factors()[0]))
        finally:
            eng.close()
            home.close()
    for a, b, what in zip(out[0], out[1], ("V", "S", "U")):
        same_bits(a, b, "online step %s capped against free" % what)


@pytest.mark.gpu
def test_one_nmf_step_capped(amd, cus, pair, worst):
    import nmf_reference as R
    from test_nmf_matrix import _held, _held_objective
    k = K_DRIVER
    X = capped_structure(k, cus)
    n, m = X.shape
    rs = np.random.RandomState(5)
    W0, H0 = (rs.rand(n, k) + 0.01).astype(np.float32), (rs.rand(k, m) + 0.01).astype(np.float32)
    L_row, L_col = int(np.diff(X.indptr).max()), int(np.diff(X.tocsc().indptr).max())
    out = []
    for eng in pair:
        eng.upload_csr(X)
        eng.nmf_set_factors(W0, H0)
        d0 = eng.nmf_divergence()
        eng.nmf_update_w()
        W1, _ = eng.nmf_get_factors(want_h=False)
        eng.nmf_update_h()
        _, H1 = eng.nmf_get_factors(want_w=False)
        out.append((W1, H1, d0, eng.nmf_divergence()))
    assert heavy_columns(X, *column_settings(k, X.nnz, cus)["default"]) >= 1      # k_col_reduce adds the item partials
    same_bits(out[0][0], out[1][0], "NMF W capped against free")
    same_bits(out[0][1], out[1][1], "NMF H capped against free")
    Ww, _ = R.step64(X, W0, H0)
    _, Hw = R.step64_h(X, out[0][0], H0)
    ratios = {}
    _held(out[0][0], Ww, L_row, k, "NMF W", ratios, "W")
    _held(out[0][1], Hw, L_col, k, "NMF H", ratios, "H")
    D, scale = R.divergence64(X, W0, H0, want_d=True)
    _held_objective(out[0][2], D, scale, k, "NMF divergence", ratios, "divergence")
    # nmf_divergence returns sqrt(2 D) (Engine.nmf_divergence; held to D above).  D comes from two sums of one float64 partial
    # per workgroup, of x log(x / wh) and of x: within the re-association bound on the magnitudes of all those terms
    for i, (W, H) in ((2, (W0, H0)), (3, (out[0][0], out[0][1]))):
        x = X.data.astype(np.float64)
        keep = x > R.EPS32
        wh = np.maximum(R.wh_entries(X, W.astype(np.float64), H.astype(np.float64)), R.EPS32)
        terms = float(np.abs(x[keep] * np.log(x[keep] / wh[keep])).sum() + x[keep].sum())
        ll_gap(out[0][i] ** 2 / 2, out[1][i] ** 2 / 2, X.nnz, terms, "NMF divergence %d capped against free" % (i - 2))
    keep_worst(worst, "NMF:", ratios)


@pytest.mark.gpu
def test_a_batch_of_members_capped(amd, cus):
    """three bootstrap members through the batched launch chain: the members' own capped grids against their free ones"""
    from test_batched_members import _batched
    k = 32
    X, U0, V0, _ = capped_corpus(k, cus)
    n = X.shape[0]
    rs = np.random.RandomState(11)
    specs = [dict(idx=rs.randint(0, n, n), U=U0, V=V0) for _ in range(3)]
    fit_kw = dict(n_iter=3, n_iter_per_test=10, tolerance=0.0, e_step_thresh=1e-32, flags=PLSA_FUSED)
    out = []
    for capped in (True, False):
        with knobs(CAP if capped else {}):
            eng = amd.Engine()
            eng.upload_csr(X)
            eng.member_batch(3)
        try:
            got, batch = _batched(eng, X, k, specs, fit_kw)
            assert batch.last_batched == 3
            out.append([(g[0], g[2], g[3], g[6]["row_grid"], g[6]["heavy_columns"]) for g in got])
        finally:
            eng.close()
    for j, (a, b) in enumerate(zip(*out)):
        assert a[0] == b[0] == 3 and a[3] == cus and b[3] > 2 * cus, (j, a[3], b[3])
        Xj = X[specs[j]["idx"]]
        h = heavy_columns(Xj, *column_settings(k, Xj.nnz, cus)["default"])
        assert a[4] == b[4] == h >= 1 and wraps(X.shape[1], cus + h, per_block(k)[2]), (j, a[4], b[4], h)
        same_bits(a[1], b[1], "member %d U capped against free" % j)
        same_bits(a[2], b[2], "member %d V capped against free" % j)


@pytest.mark.gpu
def test_reference_arithmetic_capped(amd, cus):
    """PLSA_REFERENCE_SUMS / PLSA_REFERENCE_LL fix every order: the strict oracle's bits (what test_reference_arithmetic holds
    the uncapped kernels to), the free context's bits, the likelihood included, where k_ref_row_pass, k_ref_col_pass, the
    tiled E-step and k_ref_ll_terms all wrap"""
    from oracle.plsa_oracle import Oracle
    from test_reference_arithmetic import same_bits as ref_bits
    X, U0, V0, sw = ref_corpus(cus)
    n = X.shape[0]
    k = K_REF
    assert wraps(n, cus, 32) and wraps(X.nnz, cus, 256) and wraps(ceil_div(X.nnz, 64), cus, 2)
    r, c, v = coo_arrays(X)
    o = Oracle(variant="strict")
    o.set_threads(4)
    o.set_ll_sequential(True)
    Po = np.zeros((X.nnz, k), np.float32)
    o.plsa_e_step(r, c, v, V0, U0, Po, np.float32(1e-32))
    Vo, Uo = V0.copy(), U0.copy()
    nwo, ndo = np.zeros(k, np.float32), np.zeros(n, np.float32)
    o.plsa_m_step_w_sample_weight(r, c, v, Vo, Uo, Po, sw, nwo, ndo)
    ll_o = float(o.log_likelihood(r, c, v, V0, U0, sw))
    out = []
    for capped in (True, False):
        eng = make_engine(amd, {}, capped, X)
        try:
            eng.set_arithmetic("reference_source")
            eng.set_factors(U0, V0)
            ll = eng.log_likelihood(sw)
            P = eng.e_step(1e-32)
            nw, nd = eng.m_step(sw)
            out.append((P, nw, nd) + eng.get_factors() + (np.float64(ll),))
        finally:
            eng.close()
    for a, b, what in zip(out[0], out[1], ("P", "norm_pwz", "norm_pdz", "U", "V", "log-likelihood")):
        same_bits(a, b, "reference arithmetic %s capped against free" % what)
    for a, b, what in zip(out[0], (Po, nwo, ndo, Uo, Vo), ("P(z|w,d)", "norm_pwz", "norm_pdz", "P(z|d)", "P(w|z)")):
        ref_bits(a, b, "capped " + what)
    assert abs(float(out[0][5]) - ll_o) <= 2e-6 * abs(ll_o), (out[0][5], ll_o)


# ---- case 4: builders and utilities ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_upload_and_the_builders_capped(amd, cus, pair):
    """k_validate_csr on the way in; k_expand_rows, k_iota, k_csc_gather and k_pack_entries behind the first step (whose
    results case 1 checks); the active matrix comes back as it went in, and a bad index is still seen in the last trip"""
    k = K_BUILDERS
    X, U0, V0, _ = capped_corpus(k, cus)
    assert all(wraps(W, G, p, unit) for W, p, unit, G in builder_walks(cus).values())
    for eng in pair:
        eng.upload_csr(X)
        eng.set_factors(U0, V0)
        eng.em_accumulate(None, 1e-32)
        eng.em_finish()
        eng.e_step(1e-32, want_host_copy=False)
        assert eng.packed_info() == dict(csr="packed", csc="packed")
        same_csr(eng.download_active_csr(), X, "download_active_csr")
    bad = X.copy()
    bad.indices[-1] = X.shape[1]
    with pytest.raises(ValueError):
        pair[0].upload_csr(bad)


@pytest.mark.gpu
def test_bootstrap_capped(amd, cus, pair):
    X = capped_structure(K_BUILDERS, cus)
    n = X.shape[0]
    rs = np.random.RandomState(7)
    idx = rs.randint(0, n, bootstrap_rows(cus))
    assert wraps(idx.shape[0] + 1, cus, 4) and idx.shape[0] > 4 * cus
    ref = X[idx]
    out = []
    for eng in pair:
        eng.upload_csr(X)
        eng.bootstrap(idx)
        out.append(eng.download_active_csr())
        eng.bootstrap(None)
        same_csr(eng.download_active_csr(), X, "the base after bootstrap(None)")
    same_csr(out[0], ref, "capped bootstrap against X[idx]")
    same_csr(out[0], out[1], "bootstrap capped against free")


@pytest.mark.gpu
def test_factor_initialisation_capped(amd, cus, pair):
    """the MT19937 initialisation against NumPy's own stream (n > 4 C documents, k m > 256 C cells), k_init_rows capped = free"""
    k = K_BUILDERS
    X = capped_structure(k, cus)
    n, m = X.shape
    assert wraps(n, cus, 4) and wraps(k * m, cus, 256, k)
    rng_h = np.random.RandomState(k + 3)
    rng_h.randint(0, 10, size=3)
    Uh, Vh = amd.plsa_init(X, k, rng=rng_h)
    tail = rng_h.rand(5)
    out = []
    for eng in pair:
        eng.upload_csr(X)
        rng_d = np.random.RandomState(k + 3)
        rng_d.randint(0, 10, size=3)
        eng.init_factors_numpy_stream(k, rng_d)
        Ud, Vd = eng.get_factors()
        np.testing.assert_array_equal(Ud, Uh.astype(np.float32))
        np.testing.assert_array_equal(Vd, Vh.astype(np.float32))
        np.testing.assert_array_equal(tail, rng_d.rand(5))
        eng.init_factors_device(k, seed=77)
        out.append(eng.get_factors())
    same_bits(out[0][0], out[1][0], "k_init_rows U capped against free")
    same_bits(out[0][1], out[1][1], "k_init_rows V capped against free")
    assert np.abs(out[0][0].sum(1) - 1).max() < 1e-5 and np.abs(out[0][1].sum(1) - 1).max() < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("topics", [0, 12])
def test_synthetic_generators_capped(amd, cus, pair, topics):
    """more than 4 C documents (a wave each, four per workgroup) and more than 256 C tokens (k_synth_heads, k_synth_emit)"""
    n, m, target = synthetic_sizes(cus)
    assert wraps(n, cus, 4) and wraps(target, cus, 256)
    kw = dict(seed=9, topics=topics, alpha=0.05, background=0.1) if topics else dict(seed=9)
    out = []
    for eng in pair:
        nnz = eng.generate_synthetic(n, m, target, **kw)
        A = eng.download_active_csr()
        assert A.nnz == nnz and A.shape == (n, m) and nnz > 256 * cus and np.diff(A.indptr).min() >= 1
        assert (A.data >= 1).all() and int(A.indices.max()) < m
        out.append((A, eng.synthetic_dominant_topics() if topics else None))
    same_csr(out[0][0], out[1][0], "synthetic corpus capped against free")
    if topics:
        np.testing.assert_array_equal(out[0][1], out[1][1])
        assert set(np.unique(out[0][1])) <= set(range(topics)) and len(np.unique(out[0][1])) == topics
