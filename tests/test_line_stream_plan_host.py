"""The line layout of the packed entry streams (enstop_amd/csrc/plsa_launch_plan.hpp: line_*) on a CPU.

tests/line_stream_plan_host.cpp calls the header's functions with the arguments read from stdin; it is built as a stand-alone
program with the address and undefined-behaviour sanitizers.  The expected values are the layout as DESIGN.md section 3 states
it, restated here: a block is 4 * LPN words, the word at 4 * li + c of a block holds entry c * LPN + li of that block, owners
start on whole blocks.
"""
import os
import subprocess

import pytest

from conftest import ROOT

LANES = (1, 2, 4, 8, 16, 32, 64)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("line_stream_plan") / "line_stream_plan_host")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1",
           "-g", os.path.join(ROOT, "tests", "line_stream_plan_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def call(program, name, cases):
    text = "".join("%s %s\n" % (name, " ".join(str(int(v)) for v in case)) for case in cases)
    out = subprocess.run([program], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = [[int(v) for v in line.split()] for line in out.stdout.splitlines()]
    assert len(rows) == len(cases)
    return rows


def ceil_div(a, b):
    return -(-a // b)


def row_lengths(lpn):
    return [0, 1, lpn - 1, lpn, lpn + 1, 4 * lpn - 1, 4 * lpn, 4 * lpn + 1, 8 * lpn + 3]


def col_lengths(seg):
    return [0, 1, seg - 1, seg, seg + 1, 2 * seg + 5]


def test_block_and_slot_sizes(program):
    segs = (1, 8, 15, 16, 17, 32, 48, 64, 128, 255, 256, 257)
    cases = [(lpn, seg) for lpn in LANES for seg in segs]
    for (lpn, seg), (block, slot) in zip(cases, call(program, "sizes", cases)):
        assert block == 4 * lpn
        assert slot % block == 0 and slot >= seg and slot - seg < block, (lpn, seg, slot)
    # the benchmark's flagship shape: 64-entry column items in 16-lane groups are one block, one load per lane; the document
    # pass' 8-lane block is one 128-byte line
    assert call(program, "sizes", [(16, 64), (8, 64), (8, 32)]) == [[64, 64], [32, 64], [32, 32]]


def test_documents_start_on_whole_blocks(program):
    for lpn in LANES:
        lengths = row_lengths(lpn) + col_lengths(16) + [5000]
        blocks = [b for (b,) in call(program, "blocks", [(length, lpn) for length in lengths])]
        assert blocks == [ceil_div(length, 4 * lpn) for length in lengths]
        assert blocks[0] == 0                            # an empty document takes no block and shares its successor's start
        start = 0
        for length, b in zip(lengths, blocks):           # the exclusive sum: starts in blocks, padding below one block each
            assert 0 <= b * 4 * lpn - length < 4 * lpn
            start += b
        assert start * 4 * lpn < sum(lengths) + len(lengths) * 4 * lpn


def test_every_entry_to_block_lane_component_and_back(program):
    for lpn in LANES:
        block = 4 * lpn
        longest = max(row_lengths(lpn) + col_lengths(64) + [2 * 64 + 5])
        cases = [(rel, lpn) for rel in range(longest)]
        seen = set()
        for (rel, _), got in zip(cases, call(program, "pos", cases)):
            b, lane, comp, word, rel_back, b2, lane2, comp2 = got
            # batch `comp` of block b, lane `lane`: the entry that lane takes with one word per load (batch = rel // lpn)
            assert (b, comp, lane) == (rel // block, rel // lpn % 4, rel % lpn), (rel, lpn, got)
            assert word == b * block + 4 * lane + comp and 0 <= lane < lpn and 0 <= comp < 4
            assert rel_back == rel and (b2, lane2, comp2) == (b, lane, comp)
            seen.add(word)
        assert len(seen) == longest                      # no two entries share a word
        # whole blocks are filled completely: the words of the first longest // block blocks are all taken
        full = longest // block * block
        assert set(range(full)) <= seen and max(seen) < ceil_div(longest, block) * block


def test_the_two_to_the_31_edge_of_the_offsets(program):
    limit = 2 ** 31 - 1
    assert call(program, "fits", [(0,), (limit - 1,), (limit,), (limit + 1,), (2 ** 33,)]) == [[1], [1], [1], [0], [0]]
    # a document stream before its offsets are summed: every document wastes less than one block
    cases = [(100_400_000, 1_000_000, 8), (100_400_000, 1_000_000, 16), (2 ** 31 - 2, 1, 64), (2 ** 31 - 2, 2 ** 31 - 2, 64)]
    for (nnz, n, lpn), (bound,) in zip(cases, call(program, "doc_bound", cases)):
        assert bound == nnz + n * (4 * lpn - 1)
    # the largest benchmark corpus (config 5: 5 M documents, 500 M entries, 16-lane blocks) stays below half the edge in words;
    # in blocks, as the offsets are stored, below 2^24
    (bound,), = call(program, "doc_bound", [(500_000_000, 5_000_000, 16)])
    assert bound < limit // 2 and ceil_div(bound, 64) < 2 ** 24
    cases = [(0, 64, 16), (1, 64, 16), (1_700_000, 64, 16), (2 ** 25, 64, 16), (2 ** 25 - 1, 64, 16), (2 ** 31 - 2, 256, 64)]
    for (n_items, seg, lpn), (words,) in zip(cases, call(program, "item_words", cases)):
        assert words == n_items * ceil_div(seg, 4 * lpn) * 4 * lpn
    words = [w for (w,) in call(program, "item_words", cases)]
    assert call(program, "fits", [(w,) for w in words]) == [[1], [1], [1], [0], [1], [0]]
