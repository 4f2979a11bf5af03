"""The launch arithmetic of the smoothed-EM kernels (enstop_amd/csrc/plsa_smoothed_plan.hpp) on a CPU.

The header is free of HIP; tests/smoothed_plan_host.cpp runs the kernels' own loops (first index, stride, positions walked by
smooth_advance, pad masks) for every thread of the grid the plan gives, over a bitmap of the table's float4s, built as a
stand-alone program with the address and undefined-behaviour sanitizers.  A table is [rows, kp] float32, kp a multiple of 4:
rows * kp / 4 float4s, counted in 64 bits.  Topic counts: k = 3 (one quarter, one pad), 6, 21 (kq = 6: rows straddle
workgroups), 130 (kq = 33, ragged), 1024 (rows are whole workgroups).  Sizes: none, one row, the 640- and 480-row tables of the
test matrix, a capped grid that makes three trips and more with a ragged last one, and a table one row past 2^31 floats.  The
expected values are restated here, not read from the header.
"""
import os
import re
import subprocess

import pytest

from conftest import ROOT

BLOCK = 256
SLABS = 256
KS = [3, 6, 21, 130, 1024]
ROWS = [0, 1, 480, 640, 2111]
CAPS = [1, 7, 256, 256 * 128]                   # grid_cap of a context: CUs x PLSA_GRID_MULT (256 x 128 by default)


def kq_of(k):
    return (k + 3) // 4


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("smoothed_plan") / "smoothed_plan_host")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O2",
           "-g", os.path.join(ROOT, "tests", "smoothed_plan_host.cpp"), "-o", exe]
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


def test_the_stride_loops_visit_every_float4_once_at_the_right_row_quarter_and_mask(program):
    cases = [("smooth", rows, kq_of(k), k, cap) for k in KS for rows in ROWS for cap in CAPS]
    # a table of 2^31 floats and one row more, k = 6 (kq = 2, pads in the second quarter): one walk of 2^29 places
    big_rows = 2 ** 31 // 8 + 1
    cases.append(("smooth", big_rows, 2, 6, CAPS[-1]))
    wrapped = 0
    for (_, rows, kq, k, cap), (grid, threads, stride, starts_ok, walked, pos_ok, mask_ok) in zip(cases, call(program, cases)):
        tag = (rows, kq, k, cap)
        n4 = rows * kq
        assert grid == min(max(-(-n4 // BLOCK), 1), cap), tag        # one workgroup per 256 float4s, one at least, the cap at most
        assert threads == grid * BLOCK and stride == threads, tag
        assert starts_ok == 1 and walked == 1 and pos_ok == 1 and mask_ok == 1, tag
        wrapped += n4 > 2 * threads and n4 % threads != 0             # three trips at least, the last one ragged
    assert wrapped >= len(KS)                                         # the capped grids of the list really wrap
    assert big_rows * 2 * 4 > 2 ** 31


def test_the_prior_slabs_cut_the_rows_and_cover_every_float4_once(program):
    cases = [("prior", rows, kq_of(k), k, 0) for k in KS for rows in ROWS + [255, 256, 257, 70001]]
    # (the positions past 2^31 floats are walked by the test above: both loops advance through the same two functions)
    for (_, rows, kq, k, _), (slabs, threads, block, cut_ok, walked, pos_ok, mask_ok) in zip(cases, call(program, cases)):
        tag = (rows, kq, k)
        assert slabs == min(SLABS, max(rows, 1)), tag                 # never a function of the grid cap
        assert threads == slabs * BLOCK and block == BLOCK, tag
        assert cut_ok == 1 and walked == 1 and pos_ok == 1 and mask_ok == 1, tag


def test_the_kernels_take_their_indices_from_the_plan():
    text = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_smoothed_kernels.hpp")).read()
    assert '#include "plsa_smoothed_plan.hpp"' in text
    for stated in ("plan::smooth_first(blockIdx.x, threadIdx.x)", "plan::smooth_stride(gridDim.x)", "plan::smooth_advance(",
                   "plan::smooth_pad_mask(", "plan::prior_rows_first(rows, gridDim.x, blockIdx.x)", "long long n4"):
        assert stated in text, stated
    assert "atomic" not in re.sub(r"//[^\n]*", "", text)
    host = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_smoothed.hpp")).read()
    assert host.count("plsa::plan::smooth_grid(n4, c->grid_cap)") == 2 and "plsa::plan::prior_grid(rows)" in host
    plan = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_smoothed_plan.hpp")).read()
    assert "hip" not in re.sub(r"//[^\n]*", "", plan).replace("__HIPCC__", "").lower()       # free of HIP
