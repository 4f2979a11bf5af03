"""The launch arithmetic of k_temper (enstop_amd/csrc/plsa_tempered_plan.hpp) on a CPU.

The header is free of HIP; tests/tempered_plan_host.cpp runs the kernel's own loop (first index, stride, bound) for every thread
of the grid the plan gives, over a bitmap of the table's float4s, built as a stand-alone program with the address and
undefined-behaviour sanitizers.  A table is [rows, kp] float32, kp a multiple of 4: rows * kp / 4 float4s, counted in 64 bits.
The sizes: none, one, the [640, 16] table of the test matrix, and one float4 past 2^31 / 4 -- the first table whose float
count no longer fits 32 bits with a sign.  The expected values are restated here, not read from the header.
"""
import os
import subprocess

import pytest

from conftest import ROOT

BLOCK = 256
SIZES = [0, 1, 640 * 4, 2 ** 31 // 4 + 1]
CAPS = [1, 7, 2048, 256 * 128]                  # grid_cap of a context: CUs x PLSA_GRID_MULT (256 x 128 by default)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tempered_plan") / "tempered_plan_host")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O2",
           "-g", os.path.join(ROOT, "tests", "tempered_plan_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def call(program, cases):
    text = "".join("temper %d %d\n" % case for case in cases)
    out = subprocess.run([program], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = [[int(v) for v in line.split()] for line in out.stdout.splitlines()]
    assert len(rows) == len(cases)
    return rows


def test_the_grid_covers_every_float4_of_a_table_once(program):
    cases = [(n4, cap) for n4 in SIZES for cap in CAPS if not (n4 > 2 ** 24 and cap != CAPS[-1])]   # (one walk of 2^29 places)
    assert {n4 for n4, _ in cases} == set(SIZES)
    for (n4, cap), (grid, threads, stride, starts_ok, counted, walked) in zip(cases, call(program, cases)):
        tag = (n4, cap)
        assert grid == min(max(-(-n4 // BLOCK), 1), cap), tag        # one workgroup per 256 float4s, one at least, the cap at most
        assert threads == grid * BLOCK and stride == threads, tag    # the threads' index sets are the residues modulo `threads`
        assert starts_ok == 1, tag
        assert counted == n4, tag
        assert walked == 1, tag


def test_the_kernel_takes_its_indices_from_the_plan():
    text = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_tempered_kernels.hpp")).read()
    assert '#include "plsa_tempered_plan.hpp"' in text
    assert "plan::temper_first(blockIdx.x, threadIdx.x)" in text and "plan::temper_stride(gridDim.x)" in text
    host = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_tempered.hpp")).read()
    assert "plsa::plan::temper_grid(n4, c->grid_cap)" in host and "plsa::plan::TEMPER_BLOCK" in host
    assert "long long n4" in text                                    # 64-bit count: a table of 2^31 floats and more is legal
