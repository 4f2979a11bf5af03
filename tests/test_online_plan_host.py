"""The launch arithmetic of k_online_blend (enstop_amd/csrc/plsa_online_plan.hpp) on a CPU.

The header is free of HIP; tests/online_plan_host.cpp runs the kernel's own loop (first index, stride, bound) for every thread
of every workgroup of the grid the plan gives, over a bitmap of the table's float4s, built as a stand-alone program with the
address and undefined-behaviour sanitizers.  A table is [m, kp] float32, kp a multiple of 4: m * kp / 4 float4s, counted in 64
bits.  The float4 counts: none, one, the [480, 16] table of the test matrix, and one float4 past 2^31 / 4 -- the first table
whose float count no longer fits 32 bits with a sign -- as [178956971, 12]; beside them every number of column sweeps
(kp up to 1024) and row counts around the 256 slabs.  The expected values are restated here, not read from the header.
"""
import os
import subprocess

import pytest

from conftest import ROOT

SLABS = 256
BIG = (178956971, 12)
assert BIG[0] * BIG[1] // 4 == 2 ** 31 // 4 + 1
# (m, kp): the four sizes above first
CASES = [(0, 16), (1, 4), (480, 16), BIG,
         (480, 4), (480, 24), (480, 64), (480, 132), (480, 256), (480, 260), (480, 304), (640, 516), (300, 1024), (77, 1020),
         (255, 64), (256, 64), (257, 64), (511, 12), (513, 12), (100003, 64)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("online_plan") / "online_plan_host")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O2",
           "-g", os.path.join(ROOT, "tests", "online_plan_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def call(program, cases):
    text = "".join("blend %d %d\n" % case for case in cases)
    out = subprocess.run([program], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = [[int(v) for v in line.split()] for line in out.stdout.splitlines()]
    assert len(rows) == len(cases)
    return rows


def lanes_of(kp):
    """active lanes of a workgroup: per sweep of up to 256 columns, (span / 4) float4 columns x (256 // span) strands"""
    total = 0
    for zb in range(0, kp, 256):
        span = min(256, kp - zb)
        total += span // 4 * (256 // span)
    return total


def test_the_grid_covers_every_float4_of_a_table_once(program):
    for (m, kp), (grid, n4, lanes, counted, walked, strands_ok) in zip(CASES, call(program, CASES)):
        tag = (m, kp)
        assert grid == min(max(m, 1), SLABS), tag                    # one workgroup per slab of k_colsum_partial, one at least
        assert n4 == m * kp // 4, tag                                # 64-bit: BIG's float count is 2^31 + 4
        assert lanes == lanes_of(kp) and 0 < lanes <= 256, tag
        assert counted == n4, tag
        assert walked == 1, tag
        assert strands_ok == 1, tag


def test_the_kernel_takes_its_indices_from_the_plan():
    text = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_online_kernels.hpp")).read()
    assert '#include "plsa_online_plan.hpp"' in text
    for used in ("plan::blend_lane(kp, threadIdx.x)", "plan::blend_rows_first(m, gridDim.x, blockIdx.x)",
                 "plan::blend_rows_last(m, gridDim.x, blockIdx.x)", "plan::blend_stride(kq, lane)", "plan::blend_first(",
                 "plan::blend_end("):
        assert used in text, used
    assert "long long m" in text and "long long i" in text           # 64-bit counts: a table of 2^31 floats and more is legal
    host = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_online.hpp")).read()
    assert "plsa::plan::blend_grid(st->m)" in host and "plsa::plan::BLEND_BLOCK" in host
    plan = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_online_plan.hpp")).read()
    assert "hip" not in plan.lower().replace("__hipcc__", "").replace("free of hip", "")     # the header is free of HIP
