"""The launch arithmetic of the topic combination (enstop_amd/csrc/plsa_combine_plan.hpp) on a CPU.

The header is free of HIP; tests/combine_plan_host.cpp calls its functions as the kernels and the host side (plsa_combine.hpp)
do, built as a stand-alone program with the address and undefined-behaviour sanitizers.  Pair tiles: tri_tile is the b-th pair
of `for i, for j >= i` (a bijection onto i <= j), square_tile is (b / nt, b % nt).  Vocabulary slices: what the header gives is
what test_topic_combination.host_slicing restates, the slices cut [0, m) into consecutive non-empty ranges, and every grid
stays within HIP's limits (x below 2^31, y and z at most 65535).  Co-document counts: the sets per pass and the carve of the
staging buffer.  k-NN: the carves of its two buffers.  Representatives: the member lists, under the sanitizers.  Layout: the
LDS decision, the path taken and the float32 schedule of an edge.  The expected values are restated here, not read from the
header.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_topic_combination import host_slicing

CSRC = os.path.join(ROOT, "enstop_amd", "csrc")
GIB = 1 << 30


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("combine_plan") / "combine_plan_host")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O2",
           "-g", os.path.join(ROOT, "tests", "combine_plan_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def call(program, cases):
    text = "".join(" ".join(str(v) for v in case) + "\n" for case in cases)
    out = subprocess.run([program], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = [np.array([int(v) for v in line.split()], dtype=np.int64) for line in out.stdout.splitlines()]
    assert len(rows) == len(cases)
    return rows


NTS = list(range(1, 81)) + [513, 1023, 1024]


def test_tri_tile_is_the_bth_pair_of_the_upper_triangle(program):
    for nt, row in zip(NTS, call(program, [("tri", nt) for nt in NTS])):
        i, j = np.triu_indices(nt)                    # row-major over i <= j: `for i, for j >= i`
        assert row[0] == nt * (nt + 1) // 2 == i.size, nt
        assert np.array_equal(row[1::2], i) and np.array_equal(row[2::2], j), nt


def test_square_tile_is_row_major(program):
    for nt, row in zip(NTS, call(program, [("square", nt) for nt in NTS])):
        b = np.arange(nt * nt)
        assert row[0] == nt * nt, nt
        assert np.array_equal(row[1::2], b // nt) and np.array_equal(row[2::2], b % nt), nt


def test_the_slicing_is_host_slicing_and_cuts_the_vocabulary(program):
    cases = [("slicing", which, t, m, cus) for which in (0, 1) for cus in (64, 256, 304)
             for t in (1, 63, 64, 65, 128, 129, 640, 1984, 1985, 2816, 2817, 65536)
             for m in (1, 31, 32, 33, 4037, 4099, 173762, 2 ** 20)]
    for (_, which, t, m, cus), row in zip(cases, call(program, cases)):
        nt, tiles, wanted, words, slices, last, cut_ok, finish_grid = (int(v) for v in row)
        want = host_slicing(t, m, cus, "hellinger" if which == 0 else "kl")
        tag = (which, t, m, cus)
        assert nt == -(-t // 64) and tiles == want["tiles"], tag
        assert (wanted, words, slices, last) == (want["wanted"], want["slice"], want["slices"], want["last"]), tag
        assert cut_ok == 1 and words % 32 == 0 and 1 <= last <= words, tag
        # grid (tiles, slices) of the gram kernels, (t) of k_hell_prepare, (t * t / 256) of k_hell_finish and k_sum_slices
        assert 1 <= tiles < 2 ** 31 and 1 <= slices <= 64 and t < 2 ** 31 and finish_grid == -(-t * t // 256) < 2 ** 31, tag
    row = call(program, [("slicing", 0, 64, 4037, 256)])[0]
    assert (row[3], row[4], row[5]) == (64, 64, 5)


def test_the_sets_per_pass(program):
    cases = [("sets", free, held, n, sets, cap) for free in (0, GIB, 16 * GIB) for held in (0, 3 * GIB) for n in (1, 10 ** 6)
             for sets in (1, 5, 4097, 2 ** 24) for cap in (0, 3)]
    for (_, free, held, n, sets, cap), row in zip(cases, call(program, cases)):
        chunk, mark_x, count_x = (int(v) for v in row)
        asked = cap if cap else (free + held) // 4 // (4 * n)       # a quarter of what is free, one 32-bit mask per document
        assert chunk == max(1, min(asked, sets, 4096)) and 1 <= chunk <= min(sets, 4096), (free, held, n, sets, cap)
        assert mark_x == max(1, min(64, -(-n // 4096))) and count_x == max(1, min(128, -(-n // 2048))), n
    free0, free16 = call(program, [("sets", 0, 0, 10 ** 6, 2 ** 24, 0), ("sets", 16 * GIB, 0, 10 ** 6, 2 ** 24, 0)])
    assert free0[0] == 1 and free16[0] == 1073
    big = call(program, [("sets", 0, 0, n, 1, 1) for n in (4096, 4097, 262144, 262145, 10 ** 9)])
    assert [(int(r[1]), int(r[2])) for r in big] == [(1, 2), (2, 3), (64, 128), (64, 128), (64, 128)]


def test_the_grid_of_the_representatives(program):
    """grid (m / 256, n_clusters): x stays below 2^31 for any m whose topics fit a device; y is the cluster count, which the entry
    point refuses above the 65535 the plan states"""
    ms = [1, 255, 256, 257, 173762, 2 ** 31, 2 ** 38]
    for m, row in zip(ms, call(program, [("egrid", m) for m in ms])):
        assert row[0] == -(-m // 256) < 2 ** 31 and row[1] == 65535, m
    host = code("plsa_combine.hpp")
    assert "if (n_clusters > plsa::plan::GRID_YZ_MAX)" in host
    assert host.index("if (n_clusters > plsa::plan::GRID_YZ_MAX)") < host.index("plsa::plan::member_lists(") < host.index("CHK(ensure(c, rep,")


def check_carve(starts, sizes, total, tag):
    """consecutive ranges [start, start + size): disjoint, in order, every start on 8 bytes, nothing past the total"""
    end = 0
    for start, size in zip(starts, sizes):
        assert start >= end and start % 8 == 0 and start - end < 8, tag
        end = start + size
    assert end == total, tag


def test_the_carves_are_disjoint_ordered_and_aligned(program):
    cases = [("mcarve", chunk, nw) for chunk in (1, 3, 1073, 4096) for nw in (2, 3, 20, 31, 32)]
    for (_, chunk, nw), row in zip(cases, call(program, cases)):
        co, positive, words, total = (int(v) for v in row)
        check_carve((co, positive, words), (8 * chunk * nw * nw, 8 * chunk * nw, 4 * chunk * nw), total, (chunk, nw))
        assert co == 0 and total == chunk * nw * (8 * nw + 12), (chunk, nw)       # no padding: the sizes sum to the total
    cases = [("knn", t, k) for t in (2, 3, 65, 300, 301, 65536) for k in (1, 2, 15, 1024) if k <= t]
    for (_, t, k), row in zip(cases, call(program, cases)):
        idx, done, int_total, dist, member, rho, sigma, row_sum, float_total = (4 * int(v) for v in row)
        tk = 4 * t * k
        check_carve((idx, done), (tk, 4), int_total, (t, k))
        check_carve((dist, member, rho, sigma, row_sum), (tk, tk, 4 * t, 4 * t, 4 * t), float_total, (t, k))


def member_lists(labels, n_clusters):
    first = [0] * (n_clusters + 1)
    for c in range(n_clusters):
        first[c + 1] = first[c] + sum(1 for v in labels if v == c)
    members = [i for c in range(n_clusters) for i, v in enumerate(labels) if v == c]         # row order within each cluster
    return first, members


def test_the_member_lists(program):
    ok = {"noise": (3, [0, -1, 2, 1, -1, 0, 2, 2, -7, 1]),
          "an empty cluster in the middle": (4, [3, 0, 0, -1, 2, 3, 0]),
          "all noise": (2, [-1, -1, -5]),
          "one cluster holds every row": (1, [0] * 9),
          "one cluster of many holds every row": (5, [3] * 6),
          "no rows": (2, [])}
    names = list(ok)
    cases = [("members", ok[name][0], len(ok[name][1])) + tuple(ok[name][1]) for name in names]
    for name, row in zip(names, call(program, cases)):
        n_clusters, labels = ok[name]
        first, members = member_lists(labels, n_clusters)
        nf = int(row[1])
        assert row[0] == -1 and nf == n_clusters + 1, name
        assert list(row[2:2 + nf]) == first and row[2 + nf] == len(members) and list(row[3 + nf:]) == members, name
    # a label >= n_clusters: its index, found before anything is written (the sanitizers watch both arrays)
    bad = [("members", 0, 3, -1, 0, 0), ("members", 2, 5, 1, 0, -1, 2, 1), ("members", 2, 4, 7, 1, 1, 1), ("members", 0, 2, -1, -1),
           ("members", 3, 3, 0, 1, 2 ** 31 - 1)]
    rows = call(program, bad)
    assert [int(r[0]) for r in rows] == [1, 3, 0, -1, 2]
    assert list(rows[3][1:]) == [1, 0, 0]            # n_clusters = 0 and only noise: first = [0], no members


def test_the_layout_decisions(program):
    cases = [("layout", t, dim) for t, dim in ((1024, 8), (8192, 1), (2730, 3), (1025, 8), (8193, 1), (2731, 3), (1, 1), (65536, 8))]
    for (_, t, dim), row in zip(cases, call(program, cases)):
        fits, auto, lds, per_epoch, grid = (int(v) for v in row)
        assert fits == (2 * 4 * t * dim <= 64 * 1024), (t, dim)
        assert auto == (1 if fits else 2) and lds == (1 if fits else -1) and per_epoch == 2, (t, dim)     # -1: the refusal
        assert grid == -(-t // 256), (t, dim)
    assert [int(r[0]) for r in call(program, cases[:6])] == [1, 1, 1, 0, 0, 0]


def test_the_edge_schedule_is_float32(program):
    bits = lambda v: int(np.float32(v).view(np.uint32))
    weights = [1.0, 0.75, 1e-3, 0.33333334, 3.1e-7, 0.99999994]
    cases = [("sched", bits(wmax), bits(w), bits(rate)) for wmax in (1.0, 0.75) for w in weights if w <= wmax for rate in (1, 5, 64)]
    assert any(c[1] == c[2] for c in cases)          # w == wmax: due every epoch
    for (_, wmax, w, rate), row in zip(cases, call(program, cases)):
        f = lambda u: np.array([u], np.uint32).view(np.float32)[0]
        eps = f(wmax) / f(w)
        assert eps.dtype == np.float32 and (eps / f(rate)).dtype == np.float32
        assert (int(row[0]), int(row[1])) == (bits(eps), bits(eps / f(rate))), (f(wmax), f(w), f(rate))


def code(name):
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def test_the_kernels_and_the_host_take_their_indices_from_the_plan():
    kernels = code("plsa_combine_kernels.hpp")
    assert '#include "plsa_combine_plan.hpp"' in kernels
    assert kernels.count("plan::tri_tile(blockIdx.x, plan::pair_nt(t))") == 1               # k_hell_gram
    assert kernels.count("plan::square_tile(blockIdx.x, plan::pair_nt(t))") == 1            # k_kl_gram
    assert kernels.count("plan::slice_begin(blockIdx.y, slice)") == 2 and kernels.count("plan::slice_end(blockIdx.y, slice, m)") == 2
    assert "tile_i" not in kernels and "tile_j" not in kernels and "constexpr int HELL_" not in kernels
    for name in ("k_hell_prepare", "k_hell_gram", "k_hell_finish", "kl_log2", "k_kl_gram", "k_sum_slices", "k_rep_accumulate",
                 "k_rep_normalise"):
        assert re.search(r"\b%s\(" % name, kernels), name
    for name, constants in (("plsa_metric_kernels.hpp", ("METRIC_MAX_WORDS", "METRIC_BLOCK")),
                            ("plsa_embed_kernels.hpp", ("LAYOUT_LDS_BYTES", "LAYOUT_EPOCH_BLOCK"))):
        text = code(name)
        assert '#include "plsa_combine_plan.hpp"' in text, name
        for constant in constants:
            assert "using plan::%s;" % constant in text and not re.search(r"constexpr \w+ %s\b" % constant, text), constant
    host = code("plsa_combine.hpp")
    assert host.count("plsa::plan::vocab_slicing(") == 2                   # Hellinger and KL, nowhere else
    assert "HELL_KSTEP" not in host and "HELL_TILE" not in host and "hipError_t" not in host
    for stated in ("plsa::plan::tri_tiles(", "plsa::plan::square_tiles(", "plsa::plan::member_lists(", "plsa::plan::metric_sets_per_pass(",
                   "plsa::plan::metric_carve(", "plsa::plan::metric_mark_x(", "plsa::plan::metric_count_x(", "plsa::plan::knn_carve(",
                   "plsa::plan::layout_fits_lds(", "plsa::plan::layout_path(", "plsa::plan::layout_epoch_grid(",
                   "plsa::plan::layout_edge_schedule("):
        assert stated in host, stated
    # every launch goes through the one macro (Scope, launch, launch_check), every copy through the frame
    assert host.count("hipLaunchKernelGGL(") == 1 and host.count("hipMemcpyAsync(") == 1 and host.count("hipStreamSynchronize(") == 2
    assert host.count('COMBINE_LAUNCH(call, "k_') == 12
    plan = code("plsa_combine_plan.hpp")
    assert "hip" not in plan.replace("__HIPCC__", "").lower()              # free of HIP


def test_the_core_unit_no_longer_holds_the_combination():
    old = code("plsa_kernels.hpp")
    for gone in ("k_hell_", "k_kl_gram", "k_rep_", "k_sum_slices", "kl_log2"):
        assert gone not in old, gone
    unit = open(os.path.join(CSRC, "plsa_hip.hip")).read()
    for entry in ("plsa_all_pairs_hellinger", "plsa_all_pairs_kl", "plsa_cluster_representatives", "plsa_codocument_counts",
                  "plsa_knn_membership", "plsa_layout", "plsa_host_normalize_rows", "layout_run"):
        assert not re.search(r"\b%s\(" % entry, unit), entry
    assert unit.index('#include "plsa_lda.hpp"') < unit.index('#include "plsa_combine_kernels.hpp"') < unit.index('#include "plsa_combine.hpp"')
