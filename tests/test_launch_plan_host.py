"""The launch arithmetic of the fused passes (enstop_amd/csrc/plsa_launch_plan.hpp) on a CPU.

The header is free of HIP: tests/launch_plan_host.cpp calls every function of it with the arguments read from stdin.  It is
built as a stand-alone program with the address and undefined-behaviour sanitizers.  No expected value comes from the header:
the lane shapes are test_pass_matrix.lane_shape's, the two-stage switch is test_fit_driver's NORM_SWITCH, the item lengths are
the ones DESIGN.md and the code comments quote for the benchmark configurations (worked out by hand below), and the rest are
restatements written here.
"""
import os
import subprocess

import pytest

from conftest import ROOT
from test_fit_driver import NORM_SWITCH
from test_pass_matrix import lane_shape

CUS = 256
# (lpn, ch) dispatch_shape lists; the document pass adds 8 x 2, at kp = 64 only (dispatch_shape_row)
SHAPES = {(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4), (16, 2), (32, 2)}
GRID_LIMIT = 1 << 22


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_host")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1",
           "-g", os.path.join(ROOT, "tests", "launch_plan_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def call(program, name, cases, parse=int):
    """one line per case in, one line of integers (parse=float.fromhex: of hex floats) per case out"""
    text = "".join("%s %s\n" % (name, " ".join(float(v).hex() if isinstance(v, float) else str(int(v)) for v in case)) for case in cases)
    out = subprocess.run([program], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = [[parse(v) for v in line.split()] for line in out.stdout.splitlines()]
    assert len(rows) == len(cases)
    return rows


def ceil_div(a, b):
    return -(-a // b)


def test_lane_shape_for_every_k(program):
    cases = [(k, cpl, r8) for k in range(1, 1025) for cpl in (1, 2) for r8 in (0, 1)]
    for (k, cpl, r8), got in zip(cases, call(program, "lane_shape", cases)):
        kp, col, row = lane_shape(k, cpl)
        if not r8:
            row = col                        # PLSA_ROW_SHAPE=0: the document pass in the common shape
        assert got == [kp, col[0], col[1], row[0], row[1]], (k, cpl, r8)
        assert col in SHAPES and (row in SHAPES or (row == (8, 2) and kp == 64)), (k, cpl, r8)
        assert 4 * col[0] * col[1] >= kp and 4 * row[0] * row[1] >= kp          # the lanes hold the whole k-vector
    assert [lane_shape(64)[2], lane_shape(60)[2], lane_shape(68)[2]] == [(8, 2), (16, 1), (16, 2)]


def norm_blocks(chunks):
    """the clamp of the two-stage norm restated: one workgroup per 64 chunk rows, at least 64 and at most 1024 of them"""
    return 0 if chunks <= NORM_SWITCH else min(max(chunks // 64, 64), 1024)


def test_col_pass_chunks_reduce_grid_and_norm_stages(program):
    quoted = {1: 0, 2047: 0, 2048: 0, 2049: 64, 4096: 64, 4160: 65, 65536: 1024, 1000000: 1024}
    assert NORM_SWITCH == 2048 and all(norm_blocks(c) == nb for c, nb in quoted.items())
    lpns = (1, 8, 16, 64)
    cases = [(chunks * (256 // lpn), 1000, lpn, 0, 2048) for chunks in quoted for lpn in lpns]
    for (n_items, _, lpn, _, _), got in zip(cases, call(program, "col_pass", cases)):
        chunks = n_items // (256 // lpn)
        assert got[0] == chunks and got[2] == quoted[chunks], (n_items, lpn, got)
    # a chunk is 256 / lpn items: none, one, a full chunk, one more
    cases = [(n_items, 1000, lpn, 0, 2048) for lpn in lpns for n_items in (0, 1, 256 // lpn, 256 // lpn + 1)]
    got = call(program, "col_pass", cases)
    assert [g[0] for g in got] == [0, 1, 1, 2] * len(lpns) and all(g[2] == 0 for g in got)
    # per-column sums: one group per column up to the cap, plus one workgroup per heavy column on top of it
    cap = 2048
    cases = [(10, blocks * (256 // lpn) - less, lpn, heavy, cap)
             for lpn in lpns for blocks in (1, 100, cap - 1, cap, cap + 1, 5000) for less in (0, 1) for heavy in (0, 7)]
    for (_, m, lpn, heavy, _), got in zip(cases, call(program, "col_pass", cases)):
        assert got[1] == min(max(ceil_div(m, 256 // lpn), 1), cap) + heavy, (m, lpn, heavy, got)
    assert call(program, "col_pass", [(10, 0, 16, 3, cap)])[0][1] == 1 + 3


def test_grids_of_the_document_pass(program):
    cap = 2048
    assert call(program, "grid_for", [(0, 4, cap), (1, 4, cap), (4, 4, cap), (5, 4, cap), (4 * cap, 4, cap), (1 << 40, 256, cap)]) == \
        [[1], [1], [1], [2], [cap], [cap]]
    cases = [(n, n_ritems, items, row_lpn, cap, 0) for n, n_ritems in ((300, 5000), (18846, 101000), (3000000, 1))
             for items in (0, 1) for row_lpn in (1, 8, 16, 64)]
    for (n, n_ritems, items, row_lpn, _, _), got in zip(cases, call(program, "row_pass", cases)):
        gpb = 256 // row_lpn
        assert got == [min(ceil_div(n_ritems if items else n, gpb), cap), min(ceil_div(n, gpb), cap)], (n, n_ritems, items, row_lpn)
    # the XCD-contiguous document schedule: one trip, a multiple of eight workgroups, not capped
    for n in (2048, 2049, 1000000):
        (grid, reduce_grid), = call(program, "row_pass", [(n, 0, 0, 8, cap, 1)])
        assert grid % 8 == 0 and 0 <= grid - ceil_div(n, 32) < 8 and reduce_grid == min(ceil_div(n, 32), cap)


# the benchmark configurations: (documents, non-zeros, k)
CONFIG1 = (18846, 2948108, 20)
CONFIG2 = (100000, 10000000, 32)
CONFIG3 = (1000000, 100400000, 64)


def test_item_lengths_at_the_quoted_shapes(program):
    def row(config, mode=-1, override=0):
        n, nnz, k = config
        return n, nnz, CUS, lane_shape(k)[2][0], mode, override

    def col(config, override=0):
        return config[1], CUS, lane_shape(config[2])[1][0], override
    assert lane_shape(20)[2] == (8, 1) and lane_shape(32)[2] == (8, 1) and lane_shape(64)[1:] == ((16, 1), (8, 2))
    # config 1: 65 536 group slots of 8 lanes, 156 entries per document (> 128), 44 entries per slot -> items of 32; config 2:
    # 100 entries per document: whole (its 152 entries per slot would give 64); forced off / on; a given length decides for
    # itself: config 2's documents exceed twice 48 entries
    got = call(program, "row_items", [row(CONFIG1), row(CONFIG2), row(CONFIG1, mode=0), row(CONFIG2, mode=1),
                                      row(CONFIG1, override=48), row(CONFIG2, override=48), row(CONFIG2, mode=0, override=48)])
    assert got == [[1, 32], [0, 64], [0, 32], [1, 64], [1, 48], [1, 48], [0, 48]]
    # config 1: 2 948 108 / (1.25 x 65 536) = 35 entries -> 32; config 3: 32 768 slots of 16 lanes, 2451 entries -> the cap
    assert call(program, "col_item_len", [col(CONFIG1), col(CONFIG3), col(CONFIG1, 128), col(CONFIG3, 24)]) == [[32], [64], [128], [24]]
    # the ladder 16 / 32 / 64, one CU of 64-lane groups: 32 group slots (the column items: 40, a quarter more)
    per_slot = (0, 1, 31, 32, 63, 64, 127, 128, 100000)
    ladder = [16, 16, 16, 32, 32, 64, 64, 64, 64]
    assert [g[1] for g in call(program, "row_items", [(1000, 32 * p, 1, 64, -1, 0) for p in per_slot])] == ladder
    assert [g[0] for g in call(program, "col_item_len", [(40 * p, 1, 64, 0) for p in per_slot])] == ladder
    # band of the visiting order: 2 MB of P(z|d) rows from kp = 64 on, 512 KB below, at least 64 documents; the knob as given
    assert call(program, "order_band", [(64, -1), (128, -1), (32, -1), (60, -1), (1024, -1), (64, 0), (64, 777)]) == \
        [[8192], [4096], [4096], [(512 << 10) // 240], [512], [0], [777]]


def stretches(frac, n_chunks):
    """the boundaries restated: round to nearest, never before the previous one, never past the end"""
    lo = [0]
    for x in range(1, 8):
        lo.append(min(n_chunks, max(lo[-1], int(frac[x] * n_chunks + 0.5))))
    return lo + [n_chunks]


def test_xcd_stretches_and_the_column_grid(program):
    equal = [x / 8.0 for x in range(9)]
    crossing = [0.0, 0.5, 0.3, 0.9, 0.1, 1.2, -0.2, 0.8, 1.0]            # stretches that would be negative, ends past both edges
    skewed = [0.0, 0.9, 0.91, 0.92, 0.93, 0.94, 0.95, 0.96, 1.0]
    sizes = (0, 1, 7, 8, 63, 64, 100, 1000003, GRID_LIMIT, GRID_LIMIT + 5)
    cases = [(n, frac) for n in sizes for frac in (equal, crossing, skewed)]
    for (n, frac), got in zip(cases, call(program, "balance", [(n, *frac) for n, frac in cases])):
        lo, split, unsplit = got[:9], got[9], got[10]
        assert lo == stretches(frac, n), (n, frac)
        assert lo[0] == 0 and lo[8] == n and all(0 <= lo[x] <= lo[x + 1] <= n for x in range(8)), (n, frac, lo)
        if frac is equal:
            assert lo == [(2 * x * n + 8) // 16 for x in range(9)], (n, lo)      # round(x n / 8), halves up
        assert unsplit == min(max(n, 1), GRID_LIMIT), (n, got)
        if n >= 64:                          # the pass splits from 64 chunks on (xcd_split): some stretch then holds 8 or more
            longest = max(lo[x + 1] - lo[x] for x in range(8))
            assert longest >= 8 and split == min(8 * longest, GRID_LIMIT), (n, frac, got)
        assert 1 <= split <= GRID_LIMIT


def test_wide_tables_and_the_xcd_split_rule(program):
    # 4 GB of rows: 2^24 rows of 64 floats
    assert call(program, "table_is_wide", [(16777215, 64, 0), (16777216, 64, 0), (10, 64, 1), (16777215, 64, 1), (0, 4, 0)]) == \
        [[0], [1], [1], [1], [0]]
    # from 64 chunks on, and only when P(z|d) exceeds 2 MiB: 8192 rows of 64 floats are exactly 2 MiB; PLSA_XCD_SPLIT=0
    assert call(program, "xcd_split", [(1, 63, 1000000, 64), (1, 64, 1000000, 64), (1, 64, 8192, 64), (1, 64, 8193, 64),
                                       (0, 64, 1000000, 64), (1, 1000, 18846, 20)]) == [[0], [1], [0], [1], [0], [0]]


# ------------------------------------------------------------------------------------------------
# the arithmetic of the structure builders (csrc/plsa_structures.hpp): sort bits, piece lengths, the packing rule
# ------------------------------------------------------------------------------------------------
def edge_counts(limit=2 ** 31 - 2):
    """1, 2, 3 and every 2^j - 1, 2^j, 2^j + 1 up to the largest count an upload may have"""
    values = {1, 2, 3, limit}
    for j in range(1, 32):
        values.update((2 ** j - 1, 2 ** j, 2 ** j + 1))
    return sorted(v for v in values if 1 <= v <= limit)


def test_sort_bits_cover_every_key(program):
    counts = edge_counts()
    assert counts[-1] == 2 ** 31 - 2 and 2 ** 30 + 1 in counts
    for m, (bits,) in zip(counts, call(program, "sort_bits", [(m,) for m in counts])):
        assert bits == max(1, (m - 1).bit_length()), m
        assert m - 1 < 2 ** bits, m                      # the property: the largest column id fits
    cases = [(n, band) for n in counts for band in (0, 64, 8192)]
    for (n, band), (len_bits, key_bits) in zip(cases, call(program, "order_key", cases)):
        assert len_bits == max(1, n.bit_length()), (n, band)
        band_bits = next(b for b in range(1, 64) if 2 ** b >= n // band + 1) if band else 0
        assert key_bits == len_bits + band_bits, (n, band)
        # the largest key an item can get: the last band over the longest inverted length; band 0: the last document
        largest = (((n - 1) // band) << len_bits) | (2 ** len_bits - 1) if band else n - 1
        assert largest < 2 ** key_bits and key_bits <= 64, (n, band, key_bits)
        assert 2 ** len_bits - 1 - n >= 0, (n, len_bits)  # a column of n entries still has an inverted length


def test_packing_rule_and_e_step_piece_length(program):
    ids = 2 ** 24
    cases = [(0, 10, 0), (1, 10, 0), (100, ids, 0), (100, ids + 1, 0),
             (161, 10, 10), (160, 10, 10), (159, 10, 10)]        # 16 escapes: nnz - 1, nnz, nnz + 1
    assert call(program, "packed_ok", cases) == [[0], [1], [1], [0], [1], [1], [0]]
    by_lanes = {1: 16, 2: 16, 4: 16, 8: 8, 16: 64, 32: 64, 64: 64}
    cases = [(lpn, override) for lpn in by_lanes for override in (-1, 0, 48)]
    for (lpn, override), (seg,) in zip(cases, call(program, "e_item_len", cases)):
        assert seg == (by_lanes[lpn] if override < 0 else override), (lpn, override)


# ------------------------------------------------------------------------------------------------
# the balance controller of the XCD stretches: stamps -> XCD times and spread, times -> next fractions
# ------------------------------------------------------------------------------------------------
EQUAL = [x / 8.0 for x in range(9)]


def xcd_times_restated(stamps, grid):
    t0 = min(s for s in stamps if s)
    us = [max(1.0, (max(stamps[b] for b in range(grid) if b % 8 == x) - t0) / 100.0) for x in range(8)]
    return us, (max(us) - min(us)) / (sum(us) / 8.0)


def test_xcd_times_from_hand_made_stamps(program):
    start = 5_000_000_000
    # 20 workgroups: XCD x = b % 8 has b = x, x + 8 (and x + 16 for x < 4); [20] is the start stamp
    a = [start + 100 * (300 + 7 * b) for b in range(20)] + [start]
    a[3] = 0                                             # a workgroup that never stamped: XCD 3's time is 11's or 19's
    b = list(a)
    b[20] = 0                                            # no start stamp: the earliest end stamp is the origin ...
    b[0] = start + 50                                    # ... and XCD 0 ...
    b[8] = b[16] = start + 100                           # ... ends half a microsecond after it: the floor of 1 us
    c = [start + 100 * 1000] * 8 + [start]               # one workgroup per XCD, all at 1000 us: no spread
    for stamps in (a, b, c):
        grid = len(stamps) - 1
        (got,) = call(program, "xcd_times", [(grid, *stamps)], parse=float.fromhex)
        us, spread = xcd_times_restated(stamps, grid)
        assert got[:8] == us, (got, us)
        assert abs(got[8] - spread) <= 1e-12 * max(spread, 1.0), (got[8], spread)
    us, spread = xcd_times_restated(a, 20)
    assert us == [300.0 + 7 * 16, 300.0 + 7 * 17, 300.0 + 7 * 18, 300.0 + 7 * 19, 300.0 + 7 * 12, 300.0 + 7 * 13, 300.0 + 7 * 14,
                  300.0 + 7 * 15]
    assert xcd_times_restated(b, 20)[0][0] == 1.0 and xcd_times_restated(c, 8) == ([1000.0] * 8, 0.0)


def step_restated(frac, us):
    import numpy as np
    us = np.asarray(us, np.float64)
    size = np.maximum(1e-6, np.diff(np.asarray(frac, np.float64)) * (1.0 + 0.8 * (us.mean() / us - 1.0)))
    return [0.0] + list(np.cumsum(size) / size.sum())


def steps(program, cases):
    return call(program, "balance_step", [tuple(frac) + tuple(us) for frac, us in cases], parse=float.fromhex)


def check_boundaries(program, fracs):
    """every stretch list a step produced gives chunk boundaries that start at 0, end at n_chunks and never go back"""
    cases = [(n, *frac) for n in (64, 65, 4096) for frac in fracs]
    for (n, *frac), got in zip(cases, call(program, "balance", cases)):
        lo = got[:9]
        assert lo[0] == 0 and lo[8] == n and all(lo[x] <= lo[x + 1] for x in range(8)), (n, frac, lo)


def test_balance_step_keeps_equal_times_and_stays_a_partition(program):
    import numpy as np
    # (a) equal times: nothing to correct
    skewed = [0.0, 0.9, 0.91, 0.92, 0.93, 0.94, 0.95, 0.96, 1.0]
    cases = [(frac, [t] * 8) for frac in (EQUAL, skewed) for t in (1.0, 100.0, 8000.0, 1e6)]
    for (frac, _), got in zip(cases, steps(program, cases)):
        assert max(abs(g - f) for g, f in zip(got, frac)) <= 1e-15, (frac, got)
    # (b) any times, any stretches: still a partition of the list
    rs = np.random.RandomState(2024)
    cases = []
    for _ in range(1000):
        frac = [0.0] + sorted(rs.uniform(0.0, 1.0, size=7).tolist()) + [1.0]
        cases.append((frac, np.exp(rs.uniform(0.0, np.log(1e6), size=8)).tolist()))
    assert all(1.0 <= t <= 1e6 for _, us in cases for t in us)
    produced = steps(program, cases)
    for (frac, us), got in zip(cases, produced):
        assert got[0] == 0.0 and got[8] == 1.0 and all(got[x] < got[x + 1] for x in range(8)), (frac, us, got)
        assert max(abs(g - w) for g, w in zip(got, step_restated(frac, us))) <= 1e-12, (frac, us, got)
    check_boundaries(program, produced)                  # (d)


def test_balance_converges_within_the_launches_it_is_given(program):
    """Driven from equal stretches like ensure_balance drives it -- measure, stop at a spread of 2 %, else step -- the controller
    is done within the eight measurements a first structure gets (a NumPy restatement needs 2 or 3 steps for these inputs)."""
    def slowness(s):
        return lambda f: [8000.0 * (f[x + 1] - f[x]) * s[x] for x in range(8)]

    def density(a):                                      # cost density 1 + a u over the list: the integral over a stretch
        return lambda f: [8000.0 * ((f[x + 1] - f[x]) + 0.5 * a * (f[x + 1] ** 2 - f[x] ** 2)) for x in range(8)]
    models = [slowness(s) for s in ([1, 1, 1, 1, 1, 1, 1, 2], [1, 1.1, 0.9, 1, 1.2, 1, 0.8, 1], [3, 1, 1, 1, 1, 1, 1, 1])] + \
             [density(a) for a in (0.5, 1.0, 3.0)]
    fracs = [list(EQUAL) for _ in models]
    reached = [0] * len(models)
    produced = []
    for measurement in range(1, 9):
        pending = []
        for i, model in enumerate(models):
            if reached[i]:
                continue
            us = [max(1.0, t) for t in model(fracs[i])]
            if (max(us) - min(us)) / (sum(us) / 8.0) <= 0.02:
                reached[i] = measurement
            else:
                pending.append((i, us))
        if not pending or measurement == 8:
            break
        for (i, _), got in zip(pending, steps(program, [(fracs[i], us) for i, us in pending])):
            fracs[i] = got
            produced.append(got)
    assert all(reached), reached
    assert reached[0] > 1, "the first model starts out of balance"
    check_boundaries(program, produced)                  # (d)
