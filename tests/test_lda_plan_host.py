"""The launch arithmetic of the LDA kernels (enstop_amd/csrc/plsa_lda_plan.hpp) on a CPU.

The header is free of HIP and stands on plsa_smoothed_plan.hpp; tests/lda_plan_host.cpp runs the kernels' own loops for every
thread of the grid the plan gives, built as a stand-alone program with the address and undefined-behaviour sanitizers.  The
streaming kernels (k_lda_tables, k_lda_rows, k_lda_topics) visit every float4 once with the right row, quarter and pad mask --
the pads of the state and of the tables are written as 0 through that mask, and the ABI cannot read them back.  The row
kernels (k_lda_rowsum, k_lda_wordmax) give every row to one group of lanes that never leaves its wavefront and adds the row's
quarters in an order that depends on kq alone.  The slab kernels cut the rows like k_log_prior, never by the grid cap.  Topic
counts: k = 3 (one quarter, one pad), 6, 21, 130 (kq = 33, ragged), 260 (kq = 65: more quarters than lanes), 1024.  The expected
values are restated here, not read from the header.
"""
import os
import re
import subprocess

import pytest

from conftest import ROOT

BLOCK = 256
KS = [3, 6, 21, 130, 260, 1024]
ROWS = [0, 1, 480, 640, 2111]
CAPS = [1, 7, 256, 256 * 128]


def kq_of(k):
    return (k + 3) // 4


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lda_plan") / "lda_plan_host")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O2",
           "-g", os.path.join(ROOT, "tests", "lda_plan_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def call(program, cases):
    text = "".join("%s %d %d %d %d\n" % case for case in cases)
    out = subprocess.run([program], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = [[int(v) for v in line.split()] for line in out.stdout.splitlines()]
    assert len(rows) == len(cases)
    return rows


def test_the_streaming_kernels_visit_every_float4_once_with_the_right_mask(program):
    cases = [("stream", rows, kq_of(k), k, cap) for k in KS for rows in ROWS for cap in CAPS]
    wrapped = 0
    for (_, rows, kq, k, cap), (grid, threads, once, pos_ok, mask_ok) in zip(cases, call(program, cases)):
        tag = (rows, kq, k, cap)
        n4 = rows * kq
        assert grid == min(max(-(-n4 // BLOCK), 1), cap), tag
        assert threads == grid * BLOCK and once == 1 and pos_ok == 1 and mask_ok == 1, tag
        wrapped += n4 > 2 * threads and n4 % threads != 0
    assert wrapped >= len(KS)


def test_the_row_kernels_give_every_row_to_one_group_in_a_fixed_order(program):
    cases = [("rowsum", rows, kq_of(k), k, cap) for k in KS for rows in ROWS + [70001] for cap in CAPS]
    wrapped = 0
    for (_, rows, kq, k, cap), (grid, lanes, groups, once, order_ok) in zip(cases, call(program, cases)):
        tag = (rows, kq, k, cap)
        want = 1
        while want < kq and want < 64:
            want *= 2
        assert lanes == want and groups == BLOCK // lanes, tag       # the smallest power of two >= kq, one wavefront at most
        assert grid == min(max(-(-rows // groups), 1), cap), tag
        assert once == 1 and order_ok == 1, tag
        wrapped += rows > 2 * grid * groups and rows % (grid * groups) != 0
    assert wrapped >= len(KS)


def test_the_slabs_cut_the_rows_whatever_the_cap(program):
    cases = [("slabs", rows, kq_of(k), k, 0) for k in KS for rows in ROWS + [255, 256, 257, 70001]]
    for (_, rows, kq, k, _), (slabs, topic_grid, shift_slabs, cut_ok) in zip(cases, call(program, cases)):
        assert slabs == min(256, max(rows, 1)) and shift_slabs == min(4096, max(rows, 1)) and cut_ok == 1, (rows, kq)
        assert topic_grid == -(-4 * kq // 16), (rows, kq)             # 16 topics per workgroup, 16 lanes each


def test_the_kernels_take_their_indices_from_the_plan():
    text = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_lda_kernels.hpp")).read()
    assert '#include "plsa_lda_plan.hpp"' in text and '#include "plsa_lda_math.hpp"' in text
    for stated in ("plan::smooth_first(blockIdx.x, threadIdx.x)", "plan::smooth_stride(gridDim.x)", "plan::smooth_advance(",
                   "plan::smooth_pad_mask(", "plan::prior_rows_first(rows, gridDim.x, blockIdx.x)", "long long n4",
                   "plan::lda_row_first(blockIdx.x, group, lanes)", "plan::lda_row_stride(gridDim.x, lanes)"):
        assert stated in text, stated
    assert "atomic" not in re.sub(r"//[^\n]*", "", text)
    host = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_lda.hpp")).read()
    assert host.count("plsa::plan::lda_grid(n4, c->grid_cap)") == 4 and "plsa::plan::lda_bound_grid(rows)" in host and "plsa::plan::lda_shift_grid(c->n)" in host
    assert host.count("plsa::plan::lda_rowsum_grid(") == 2
    for name in ("plsa_lda_plan.hpp", "plsa_lda_math.hpp"):
        plan = open(os.path.join(ROOT, "enstop_amd", "csrc", name)).read()
        assert "hip" not in re.sub(r"//[^\n]*", "", plan).replace("__HIPCC__", "").lower(), name       # free of HIP
