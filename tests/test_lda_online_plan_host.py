"""The launch arithmetic of k_lda_online_blend (enstop_amd/csrc/plsa_lda_online_kernels.hpp) on a CPU.

The kernel blends the block's counts into lambda in place and leaves the float64 slab sums of the result where
k_lda_topic_partial would have left them, so that kernel's sweep is never launched.  It takes its geometry from
plsa_online_plan.hpp (k_online_blend's) and its pad mask from plsa_smoothed_plan.hpp; k_lda_topic_partial takes its slabs from
plan::prior_rows_* of plsa_lda_plan.hpp.  tests/lda_online_plan_host.cpp, built as a stand-alone program with the address and
undefined-behaviour sanitizers, runs the kernel's own loops for every thread of every workgroup over a bitmap of the table's
float4s and walks k_lda_topic_partial's loops beside them: every float4 once and by one lane, the same slabs, the same rows in
the same order per (column, strand), the strand sums left where the second half reads them, the pads masked.
"""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SLABS = 256
KP = [4, 8, 24, 64, 132, 300, 1024]
M = [0, 1, 2, 255, 256, 257, 480, 2111]


def topic_counts(kp):
    """k: no pads, one pad, three pads, and a whole quarter and more of pads where the row has one"""
    return sorted({kp, kp - 1, kp - 3, max(1, kp - 5), 1} - {0, -1, -2})


CASES = [(m, kp, k) for kp in KP for m in M for k in topic_counts(kp) if k >= 1]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lda_online_plan") / "lda_online_plan_host")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O2",
           "-g", os.path.join(ROOT, "tests", "lda_online_plan_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def test_the_blend_walks_the_table_once_in_the_slabs_and_strands_of_the_topic_partials(program):
    text = "".join("blend %d %d %d\n" % case for case in CASES)
    out = subprocess.run([program], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = [[int(v) for v in line.split()] for line in out.stdout.splitlines()]
    assert len(rows) == len(CASES)
    for (m, kp, k), (grid, n4, walked, slabs_same, strands_same, mask_ok) in zip(CASES, rows):
        tag = (m, kp, k)
        assert grid == min(max(m, 1), SLABS), tag            # one workgroup per slab of k_lda_topic_partial, one at least
        assert n4 == m * kp // 4, tag
        assert walked == 1, tag                              # every float4 of the table once, by one lane
        assert slabs_same == 1, tag                          # blend_grid == lda_bound_grid, blend_rows_* == prior_rows_*
        assert strands_same == 1, tag                        # per (column, strand): the same rows in the same order
        assert mask_ok == 1, tag


def _code(name):
    return re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "enstop_amd", "csrc", name)).read())


def test_the_kernel_takes_its_indices_from_the_plan():
    text = _code("plsa_lda_online_kernels.hpp")
    assert '#include "plsa_online_plan.hpp"' in text and '#include "plsa_lda_plan.hpp"' in text
    for used in ("plan::blend_lane(kp, threadIdx.x)", "plan::blend_rows_first(m, gridDim.x, blockIdx.x)",
                 "plan::blend_rows_last(m, gridDim.x, blockIdx.x)", "plan::blend_stride(kq, lane)", "plan::blend_first(",
                 "plan::blend_end(", "plan::smooth_pad_mask(lane.q, k)",
                 # the strand sums and the partials: where the walker says they are
                 "&sred[lane.sweep][lane.strand * lane.span + 4 * (lane.q - lane.sweep * 64)]",
                 "tot += sred[sweep][r * span + z - zb]", "partials[(long long)blockIdx.x * kp + z] = tot"):
        assert used in text, used
    assert "long long m" in text and "long long i" in text           # 64-bit counts
    assert "float4 sum" not in text and text.count("double") >= 4    # float64 strands, where k_online_blend has float32
    # k_lda_topic_partial's half of the comparison is the source the walker restates
    topic = _code("plsa_lda_kernels.hpp")
    for used in ("plan::prior_rows_first(rows, gridDim.x, blockIdx.x)", "plan::prior_rows_last(rows, gridDim.x, blockIdx.x)",
                 "for (long long w = r0 + ro; w < r1; w += rpp) s += (double)T[w * kp + z]",
                 "tot += sred[r * span + threadIdx.x]", "partials[(long long)blockIdx.x * kp + zb + threadIdx.x] = tot"):
        assert used in topic, used
    host = _code("plsa_lda_online.hpp")
    assert "dim3(plsa::plan::blend_grid(st->m)), dim3(plsa::plan::BLEND_BLOCK)" in host
    # the topic-side chain is plsa_lda.hpp's, on the side it is handed: the slab count of the state's m
    shared = _code("plsa_lda.hpp")
    chain = shared[shared.index("int run_lda_topic_tables("):shared.index("int run_lda_table_v(")]
    assert "plsa::plan::lda_bound_grid(t.m)" in chain and "st->m, st->k, st->kp}" in host
    # the sweep of k_lda_topic_partial is launched for a lambda the host set, never behind the blend
    assert chain.index("if (sweep) {") < chain.index("plsa::k_lda_topic_partial") < chain.index("plsa::k_lda_topic_sums")
    update = host[host.index("int lda_online_global_update("):host.index("struct LdaOnlineTopicSide")]
    assert "run_lda_topic_tables(c, lda_online_side(st), false, true)" in update and "k_lda_topic_partial" not in update
    set_lambda = host[host.index("int plsa_lda_online_set_lambda("):host.index("int plsa_lda_online_get_lambda(")]
    assert "run_lda_topic_tables(h, lda_online_side(st), true, true)" in set_lambda
