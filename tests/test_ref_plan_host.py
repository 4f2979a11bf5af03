"""The launch arithmetic of the reference arithmetic (enstop_amd/csrc/plsa_ref_plan.hpp) on a CPU.

The header is free of HIP: tests/ref_plan_host.cpp calls every function of it with the arguments read from stdin.  It is built
as a stand-alone program with the address and undefined-behaviour sanitizers.  No expected value comes from the header: the
lanes and topics per lane are a table written out below, the chunk geometry of the pair chain is restated here with ceiling
divisions, the block plans are test_reference_blocked.plan_for's, and one case of each is worked by hand.
"""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT
from test_reference_blocked import kp_of, plan_for


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ref_plan") / "ref_plan_host")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1",
           "-g", os.path.join(ROOT, "tests", "ref_plan_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def call(program, name, cases):
    """one line per case in, one line of integers per case out"""
    text = "".join("%s %s\n" % (name, " ".join(str(int(v)) for v in case)) for case in cases)
    out = subprocess.run([program], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = [[int(v) for v in line.split()] for line in out.stdout.splitlines()]
    assert len(rows) == len(cases)
    return rows


def ceil_div(a, b):
    return -(-a // b)


# padded topic counts from .. to -> (lanes per document or column G, topics per lane NZ): topic z = lane + G t
LANES = [(4, 8, 8, 1), (12, 16, 16, 1), (20, 32, 32, 1), (36, 64, 64, 1), (68, 128, 64, 2), (132, 256, 64, 4),
         (260, 512, 64, 8), (516, 1024, 64, 16)]
# the topic counts the reference-arithmetic tests run on a GPU (test_reference_arithmetic's parametrisations; 16 and 6: the
# goldens fit_k16_mid and refit_k6)
GPU_TESTED_K = [1, 3, 65, 128, 130, 300, 520, 1000, 8, 20, 70, 5, 64, 200, 16, 6]


def lanes_of(kp):
    (g, nz), = [(g, nz) for lo, hi, g, nz in LANES if lo <= kp <= hi]
    return g, nz


def test_lanes_and_topics_per_lane_for_every_padded_k(program):
    kps = list(range(4, 1025, 4))
    assert [lo for lo, _, _, _ in LANES] == [4] + [hi + 4 for _, hi, _, _ in LANES[:-1]] and LANES[-1][1] == 1024
    for kp, (nz, g) in zip(kps, call(program, "lanes", [(kp,) for kp in kps])):
        assert (g, nz) == lanes_of(kp), kp
        assert g * nz >= kp and (nz == 1 or g == 64), kp          # lanes times topics per lane cover the k-vector
        assert nz in (1, 2, 4, 8, 16) and g in (8, 16, 32, 64)
    assert call(program, "lanes", [(1028,), (1,)]) == [[0, 0], [1, 8]]          # unsupported; the likelihood's one "topic"
    # every (G, NZ) class is reached by a GPU test of the reference arithmetic
    assert {lanes_of(kp_of(k)) for k in GPU_TESTED_K} == {(g, nz) for _, _, g, nz in LANES}


PAIR_SC, PAIR_R = 8, 16                      # chunks per wave turn (the padding of the chunk sums), chunks per group
SPANS = (1, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 47999999, 48000000)
CHUNK_KNOBS = (0, 64, 1024, 4096, 63, 100, 8192)         # 0: unset; the last three are ignored


def chain_geometry(nnz, L):
    chunks = ceil_div(nnz, L)
    return [chunks, ceil_div(chunks, PAIR_R), ceil_div(chunks, PAIR_SC), ceil_div(chunks, PAIR_SC) * PAIR_SC]


def test_pair_chain_geometry_and_scratch_bytes(program):
    # by hand: 4097 non-zeros in chunks of 256 are 17 chunks (16 full, one of a single addend), 2 groups of 16, 3 super-chunks
    # of 8 and so 24 padded chunk sums
    assert chain_geometry(4097, 256) == [17, 2, 3, 24]
    (hand,) = call(program, "pair_chain", [(4097, 4097, 4097, 64, 1, 0)])
    assert hand[:5] == [256, 17, 2, 3, 24] and hand[9:] == [8 * 24 * 64, 16 * 17 * 64, 4 * 17 * 64, 16 * 2 * 64, 4 * 2 * 64]
    cases = [(span, span + extra, span + extra, kp, two, knob) for span in SPANS for extra in (0, 1000) for two in (0, 1)
             for knob in CHUNK_KNOBS for kp in (1, 4, 64, 68, 1024)]
    lengths = set()
    for (span, cap, corpus, kp, two, knob), got in zip(cases, call(program, "pair_chain", cases)):
        L = knob if knob in (64, 1024, 4096) else (1024 if not two and corpus >= 48000000 else 256)
        lengths.add(L)
        s, c = chain_geometry(span, L), chain_geometry(cap, L)
        # float64 chunk sums, padded; records of four 32-bit words and one word of exponents per chunk, and per group with
        # two levels (one level has no group records)
        nbytes = [8 * c[3] * kp, 16 * c[0] * kp, 4 * c[0] * kp, 16 * c[1] * kp * two, 4 * c[1] * kp * two]
        assert got == [L] + s + c + nbytes, (span, cap, kp, two, knob)
        assert s[3] >= s[0] and s[1] * PAIR_R >= s[0] and s[0] * L >= span > (s[0] - 1) * L
    assert lengths == {64, 256, 1024, 4096}
    # the longer chunks of one level follow the CORPUS, not the span (a block of documents walks the corpus' chunks)
    assert [g[0] for g in call(program, "pair_chain", [(1000, 1000, 48000000, 4, 0, 0), (1000, 1000, 47999999, 4, 0, 0),
                                                        (1000, 1000, 48000000, 4, 1, 0)])] == [1024, 256, 256]
    assert 16 * chain_geometry(48000000, 256)[0] * 1024 > 2 ** 31            # (why 64 bits)


def test_tiles_of_the_tiled_passes(program):
    cases = [(nnz, nz, kp) for nz, kp in ((1, 4), (1, 64), (2, 68), (4, 256), (8, 512), (16, 1024))
             for nnz in (0, 1, 64 // nz - 1, 64 // nz, 64 // nz + 1, 3000000000)]
    for (nnz, nz, kp), got in zip(cases, call(program, "tiles", cases)):
        # a wave's tile: 64 / nz entries; two tiles of kp + 1 floats per entry in a workgroup's LDS
        assert got == [ceil_div(nnz, 64 // nz), 4 * 2 * (64 // nz) * (kp + 1)], (nnz, nz, kp)
    assert call(program, "tiles", [(65, 1, 64)]) == [[2, 33280]]


def test_thresholds(program):
    # chain_mode 0 auto: pairs from 4096 non-zeros unless switched off; 1 pairs, 2 serial: whatever the size
    cases = [(mode, off, nnz) for mode in (0, 1, 2) for off in (0, 1) for nnz in (4095, 4096)]
    assert [g[0] for g in call(program, "pairs_now", cases)] == [0, 1, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0]
    # more than a quarter of the chunks on the slow way
    assert call(program, "walk_too_slow", [(25, 100), (26, 100), (1, 4), (2, 4), (0, 0), (1, 1)]) == [[0], [1], [0], [1], [0], [1]]
    # unset (-1): from 300 000 documents; 0 / 1 pin either
    cases = [(n, knob) for knob in (-1, 0, 1) for n in (299999, 300000)]
    assert [g[0] for g in call(program, "row_tiled", cases)] == [0, 1, 0, 0, 1, 1]


def block_case(indptr, kp, budget, with_indptr=1):
    n = len(indptr) - 1
    return (n, indptr[-1], kp, budget, with_indptr) + (tuple(indptr) if with_indptr else ())


def test_block_plan_against_the_greedy_plan(program):
    # by hand: four documents of 3 entries, kp = 4: 1120 bytes are 70 rows of 16 bytes, 64 of them slack: 6 rows, two documents
    assert call(program, "block_plan", [block_case([0, 3, 6, 9, 12], 4, 1120)]) == [[0, 6, 2, 0, 2, 4, 0, 6, 12]]
    rng = np.random.default_rng(20261019)
    cases, expected = [], []
    for k in (1, 6, 64, 130):
        for n in (1, 7, 200):
            lens = rng.integers(1, 40, n) * (rng.random(n) > 0.3)           # empty documents among them
            if n == 200:
                lens[:3] = 0; lens[-2:] = 0                                  # ... at both ends too
            indptr = [0] + [int(v) for v in np.cumsum(lens)]
            X = SimpleNamespace(indptr=np.array(indptr), nnz=indptr[-1], shape=(n, 50))
            for B in (1, 2, 3, 10, 10 ** 6):
                budget = 4 * kp_of(k) * (max(X.nnz // B, int(lens.max()), 1) + 64)
                sizes, cuts = plan_for(X, k, budget)
                cases.append(block_case(indptr, kp_of(k), budget))
                expected.append((sizes, cuts, indptr))
    several = 0
    for (sizes, cuts, indptr), got in zip(expected, call(program, "block_plan", cases)):
        status, largest, blocks = got[:3]
        doc, ent = got[3:4 + blocks], got[4 + blocks:]
        assert status == 0 and blocks == len(sizes) and largest == max(sizes), (got, sizes)
        assert doc == cuts and ent == [indptr[d] for d in cuts] and [b - a for a, b in zip(ent, ent[1:])] == sizes
        several += blocks > 2
    assert several >= 10
    kp = 8
    rows = 50                                                                # max_rows of the budget below
    budget = 4 * kp * (rows + 64)
    # a document of exactly max_rows entries is a block of its own; one more and it does not fit: document 1, its length
    assert call(program, "block_plan", [block_case([0, 5, 5 + rows, 8 + rows], kp, budget)]) == \
        [[0, rows, 3, 0, 1, 2, 3, 0, 5, 5 + rows, 8 + rows]]
    assert call(program, "block_plan", [block_case([0, 5, 6 + rows, 9 + rows], kp, budget)]) == [[2, 1, rows + 1]]
    # 65 rows (one and the slack) are the least budget; one byte less holds no row
    assert call(program, "block_plan", [block_case([0, 1, 2], kp, 65 * 4 * kp - 1), block_case([0, 1, 2], kp, 65 * 4 * kp)]) == \
        [[1], [0, 1, 2, 0, 1, 2, 0, 1, 2]]
    # everything fits: one block, and indptr is not looked at (the program passes a null pointer)
    assert call(program, "block_plan", [(7, rows, kp, budget, 0), (0, 0, kp, budget, 0)]) == [[0, rows, 1, 0, 7, 0, rows], [0, 0, 1, 0, 0, 0, 0]]
