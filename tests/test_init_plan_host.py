"""The arithmetic of factor initialisation with the MT19937 stream (enstop_amd/csrc/plsa_init_plan.hpp) on a CPU.

The header is free of HIP: tests/init_plan_host.cpp calls every function of it with the arguments read from stdin.  It is built
as a stand-alone program with the address and undefined-behaviour sanitizers.  No expected value comes from the header: the
stream plan is restated here and held to the properties the device code relies on, the jump tree is simulated in Python and
its keys are compared with a numpy.random.RandomState advanced the long way, the scratch layout is compared with the
expressions mt_init used before the plan existed, written out as literal formulas, and one case of each is worked by hand.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("init_plan") / "init_plan_host")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1",
           "-g", os.path.join(ROOT, "tests", "init_plan_host.cpp"), "-o", exe]
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


def pow2_at_least(v):
    p = 1
    while p < v:
        p *= 2
    return p


# (n, m, k, draw_topics): the shapes of the GPU tests of the stream (test_hip_parity.py; the last of them the refit
# initialisation, which draws no topics), the smallest corpus, one whose words end inside the generator's current block
# (48 words), and the 1 M x 100 k, k = 64 corpus of BASELINE.md
SHAPES = [(40, 50, 6, 1), (333, 1000, 20, 1), (5000, 3000, 64, 1), (17, 9, 33, 1), (20000, 5000, 33, 1), (3000, 700, 33, 0),
          (2, 1, 3, 1), (5, 7, 2, 1), (1000000, 100000, 64, 1)]
POSITIONS = (0, 1, 3, 623, 624)
STREAMS = (1, 2, 5, 16, 128, 256, 4096)
MIN_BLOCKS = (1, 4096)
STREAM_FIELDS = ("v_doubles", "n_doubles", "n_words", "first", "total_blocks", "per_stream", "log2_per", "n_streams",
                 "streams_p2", "levels", "words_bytes")


def parse_stream(row):
    assert row[0] == 1, row
    s = dict(zip(STREAM_FIELDS, row[1:]))
    rest = row[1 + len(STREAM_FIELDS):]
    assert len(rest) == 3 * s["levels"]
    s["exponent"], s["step"], s["sources"] = rest[0::3], rest[1::3], rest[2::3]
    return s


def stream_rule(n, m, k, draw_topics, pos0, mt_streams, mt_min_blocks):
    """the cut of the stream, restated: rand(k, m) then rand(n, k), two words per double; pieces of the least power of two of
    blocks with which mt_streams pieces cover the whole blocks, once there are mt_min_blocks of them"""
    n_doubles = (k * m if draw_topics else 0) + n * k
    n_words = 2 * n_doubles
    first = min(624 - pos0, n_words)
    total_blocks = ceil_div(n_words - first, 624)
    if mt_streams > 1 and total_blocks >= mt_min_blocks:
        per_stream = pow2_at_least(ceil_div(total_blocks, mt_streams))
        n_streams = ceil_div(total_blocks, per_stream)
    else:
        per_stream, n_streams = max(total_blocks, 1), 1
    return dict(n_doubles=n_doubles, n_words=n_words, first=first, total_blocks=total_blocks, per_stream=per_stream,
                n_streams=n_streams)


def jump_tree(s):
    """the levels of the tree as k_mt_jump runs them: {stream: blocks from the key given}; no stream is made twice"""
    offset = {0: 0}
    for l in range(s["levels"]):
        step = s["step"][l]
        for i in range(s["sources"][l]):
            q = 2 * step * i
            if q + step < s["n_streams"]:
                assert q in offset and q + step not in offset, (q, step, offset)
                offset[q + step] = offset[q] + 2 ** s["exponent"][l]
    return offset


def test_stream_plan_over_the_grid(program):
    # by hand: 40 documents, 50 words, 6 topics: 300 + 240 doubles, 1080 words; a fresh block (position 0) gives 624 of them,
    # the other 456 are one block: one stream whatever is allowed.  The same with 2030 documents: 12 480 doubles, 24 960
    # words, 39 blocks behind the first 624 words; five streams take 8 blocks each (4 x 5 < 39 <= 8 x 5), five of them are
    # needed, the tree has 8 slots and 3 levels, which jump by 2^5, 2^4, 2^3 blocks over 4, 2, 1 slots from 1, 2, 4 sources
    (a, b) = call(program, "stream", [(40, 50, 6, 1, 0, 5, 1), (2030, 50, 6, 1, 0, 5, 1)])
    assert a == [1, 300, 540, 1080, 624, 1, 1, 0, 1, 1, 0, 4320]
    assert b == [1, 300, 12480, 24960, 624, 39, 8, 3, 5, 8, 3, 99840, 5, 4, 1, 4, 2, 2, 3, 1, 4]
    assert jump_tree(parse_stream(b)) == {0: 0, 4: 32, 2: 16, 1: 8, 3: 24}

    cases = [shape + (pos0, streams, min_blocks) for shape in SHAPES for pos0 in POSITIONS for streams in STREAMS
             for min_blocks in MIN_BLOCKS]
    several = ended_inside = 0
    for case, row in zip(cases, call(program, "stream", cases)):
        n, m, k, draw_topics, pos0, mt_streams, mt_min_blocks = case
        s = parse_stream(row)
        want = stream_rule(*case)
        assert {key: s[key] for key in want} == want, case
        assert s["v_doubles"] == (k * m if draw_topics else 0) and s["words_bytes"] == 4 * s["n_words"]
        # k_mt19937_fill states these two on the device:
        #     const i64 first = min((i64)(624 - pos0), n_words);
        #     const i64 total_blocks = (n_words - first + 623) / 624;
        assert s["n_words"] == 2 * s["n_doubles"]
        assert s["first"] == min(624 - pos0, s["n_words"])
        assert s["total_blocks"] == (s["n_words"] - s["first"] + 623) // 624
        if s["n_streams"] > 1:
            assert s["per_stream"] == 2 ** s["log2_per"]
        assert 1 <= s["n_streams"] <= mt_streams
        assert s["n_streams"] * s["per_stream"] >= s["total_blocks"]
        if s["total_blocks"] > 0:         # the last stream owns a block: the state it leaves is the stream's
            assert (s["n_streams"] - 1) * s["per_stream"] < s["total_blocks"]
        assert s["streams_p2"] == pow2_at_least(s["n_streams"]) and 2 ** s["levels"] == s["streams_p2"]
        if mt_streams == 1 or s["total_blocks"] < mt_min_blocks:
            assert s["n_streams"] == 1
        # the tree puts stream r exactly r pieces behind the key
        assert s["exponent"] == [s["log2_per"] + s["levels"] - 1 - l for l in range(s["levels"])]
        assert s["step"] == [s["streams_p2"] >> (l + 1) for l in range(s["levels"])]
        assert s["sources"] == [2 ** l for l in range(s["levels"])]
        assert jump_tree(s) == {r: r * s["per_stream"] for r in range(s["n_streams"])}, case
        several += s["n_streams"] > 1
        ended_inside += s["n_words"] < 624 - pos0
    assert several >= 100 and ended_inside >= 20
    # a position beyond the block is refused
    assert call(program, "stream", [(40, 50, 6, 1, 625, 5, 1), (40, 50, 6, 1, -1, 5, 1), (40, 50, 6, 1, 624, 5, 1)])[:2] == [[0], [0]]


@pytest.mark.parametrize("advance", [1, 700])
def test_jump_tree_keys_are_numpy_keys(program, advance):
    """The planned jumps applied on the host (csrc/mt_jump.hpp) to a RandomState key: stream r's key is the key of a generator
    that produced r * per_stream * 624 more words."""
    rs = np.random.RandomState(20261019)
    rs.bytes(4 * advance)
    state = rs.get_state()
    assert state[2] == advance % 624
    n, m, k = (2030, 50, 6) if advance == 1 else (1990, 77, 6)     # 40 and 39 blocks behind the current one
    case = (n, m, k, 1, state[2], 5, 1)
    (row,) = call(program, "jump_tree", [case + tuple(int(v) for v in state[1])])
    n_streams, per_stream = row[:2]
    assert (n_streams, per_stream) == (5, 8) and len(row) == 2 + 624 * n_streams
    plan = stream_rule(*case)
    assert plan["total_blocks"] == (40 if advance == 1 else 39) and (plan["n_streams"], plan["per_stream"]) == (5, 8)
    for r in range(n_streams):
        key = np.array(row[2 + 624 * r:2 + 624 * (r + 1)], dtype=np.uint32)
        after = rs.get_state()
        assert after[2] == state[2]
        want = np.array(after[1], dtype=np.uint32)
        np.testing.assert_array_equal(key[1:], want[1:])
        assert (int(key[0]) ^ int(want[0])) & 0x80000000 == 0          # only the top bit of word 0 is generator state
        rs.bytes(4 * per_stream * 624)


SCRATCH_FIELDS = ("state_bytes", "fin_bytes", "poly_bytes", "marg_word", "nch", "tiles", "csum_off", "pairs_off", "tsum_off",
                  "guess_off", "seq_bytes", "grid_x", "grid_y")


def test_scratch_layout(program):
    # by hand: 6 topics over 4097 words: 65 chunks of 64 draws (the last of one), 2 tiles of 64 chunks, 390 chunks in all:
    # 3120 bytes of sums, 6240 of pairs, 3120 of room for the 12 tile sums, 1560 of guesses: 14 040; a tree of 8 slots and 3
    # levels: 8 and 3 blocks of 2496 bytes; the state handed back is 625 words, the marginals start at word 632 = byte 2528
    assert call(program, "scratch", [(6, 4097, 8, 3, 0)]) == [[19968, 10752, 7488, 632, 65, 2, 0, 3120, 9360, 12480, 14040, 2, 6]]
    cases = [(k, m, p2, levels, chain) for k in (1, 6, 33, 64, 1024) for m in (1, 63, 64, 65, 4097, 173762, 4500001)
             for p2, levels in ((1, 0), (8, 3), (4096, 12)) for chain in (0, 1)]
    for (k, m, p2, levels, chain), row in zip(cases, call(program, "scratch", cases)):
        s = dict(zip(SCRATCH_FIELDS, row))
        assert s["nch"] == ceil_div(m, 64) and s["tiles"] == ceil_div(s["nch"], 64)
        assert (s["grid_x"], s["grid_y"]) == (s["tiles"], k)
        # what mt_init computed in place:
        #     ensure(st, sizeof(unsigned) * 624 * streams_p2); ensure(fin, sizeof(unsigned) * 640 + sizeof(double) * 1024);
        #     ensure(gp, sizeof(unsigned) * polys.size()), polys of levels * 624 words; marg = (double *)(fin + 632 words)
        assert s["state_bytes"] == 4 * 624 * p2 and s["fin_bytes"] == 4 * 640 + 8 * 1024 and s["poly_bytes"] == 4 * levels * 624
        assert s["marg_word"] == 632
        #     ensure(mt_seq, k * ((m + 64 - 1) / 64) * (3 * sizeof(u64) + sizeof(int) + sizeof(double)))   [not with the chain]
        #     per = k * nch; csum = (u64 *)mt_seq; pairs = csum + per; tsum = (double *)(pairs + 2 * per); guess = (int *)(tsum + per)
        per = k * ((m + 64 - 1) // 64)
        assert s["seq_bytes"] == (0 if chain else per * (3 * 8 + 4 + 8))
        assert [s["csum_off"], s["pairs_off"], s["tsum_off"], s["guess_off"]] == [0, 8 * per, 8 * per + 16 * per, 8 * per + 16 * per + 8 * per]
        # disjoint, in order, aligned for what they hold, and the total is the end of the last; the tile sums fit their room
        regions = [(s["csum_off"], 8 * per, 8), (s["pairs_off"], 16 * per, 8), (s["tsum_off"], 8 * k * s["tiles"], 8),
                   (s["guess_off"], 4 * per, 4)]
        end = 0
        for off, size, align in regions:
            assert off >= end and off % align == 0
            end = off + size
        assert s["tsum_off"] + 8 * per == s["guess_off"] and k * s["tiles"] <= per
        if not chain:
            assert s["seq_bytes"] == end
        # the marginals lie behind the 625 words of the state, on an 8-byte boundary, with room for 1024 doubles
        marg = 4 * s["marg_word"]
        assert marg % 8 == 0 and marg >= 625 * 4 and marg + 8 * 1024 <= s["fin_bytes"]
    assert 1024 * ceil_div(4500001, 64) * 36 > 2 ** 31                       # (why 64 bits)


def test_host_side_grids(program):
    # by hand: 70 words and 36 padded topics are 3 x 2 tiles of 32 x 32; 130 documents are 3 waves of 64
    assert call(program, "grids", [(130, 70, 36)]) == [[3, 2, 3]]
    cases = [(n, m, kp) for n in (1, 63, 64, 65, 1000000) for m in (1, 31, 32, 33, 173762) for kp in (4, 32, 36, 1024)]
    for (n, m, kp), got in zip(cases, call(program, "grids", cases)):
        assert got == [ceil_div(m, 32), ceil_div(kp, 32), ceil_div(n, 64)], (n, m, kp)
