"""CPU-only checks of the scoring boundary (include/plsa_hip_score.h): the header declares exactly plsa_score_rows and is
plain C99, the built library exports it, enstop_amd/_lib.py binds it in a table of its own, the drop-in tables and headers
are untouched, and INTEGRATION.md documents it with what it stands for."""
import os
import re
import subprocess

from conftest import ROOT

HEADER = "plsa_hip_score.h"
ENTRIES = ["plsa_score_rows"]
OTHER_HEADERS = ("plsa_hip.h", "plsa_hip_diag.h", "plsa_hip_members.h", "plsa_hip_metrics.h", "plsa_hip_blocked.h",
                 "plsa_hip_embed.h", "plsa_hip_nmf.h")


def _symbols(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(plsa_[a-z0-9_]+)\s*\(", text)))


def test_score_header_declares_exactly_the_entry_point():
    assert _symbols(HEADER) == ENTRIES


def test_score_header_is_plain_c99():
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c",
                          os.path.join(ROOT, "include", HEADER)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_score_symbol_exported_and_bound_in_its_own_table_only():
    from enstop_amd import _lib
    lib = _lib.load()
    assert sorted(_lib.SCORE_SIGNATURES) == ENTRIES
    for name, (res, args) in _lib.SCORE_SIGNATURES.items():
        assert hasattr(lib, name), "libplsa_hip.so does not export %s" % name
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res            # applied by load()
    assert len(_lib.SCORE_SIGNATURES["plsa_score_rows"][1]) == 9
    for table in (_lib.SIGNATURES, _lib.MEMBER_SIGNATURES, _lib.METRIC_SIGNATURES, _lib.BLOCKED_SIGNATURES,
                  _lib.EMBED_SIGNATURES, _lib.NMF_SIGNATURES):
        assert not set(ENTRIES) & set(table)
    for other in OTHER_HEADERS:
        assert not set(ENTRIES) & set(_symbols(other)), other


def test_drop_in_table_still_equals_the_two_drop_in_headers():
    from enstop_amd import _lib
    assert sorted(_lib.SIGNATURES) == sorted(set(_symbols("plsa_hip.h")) | set(_symbols("plsa_hip_diag.h")))


def test_score_entry_point_is_documented_with_what_it_stands_for():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert HEADER in doc
    assert "plsa_score_rows" in doc
    assert "plsa.py:329-386" in doc                                 # the reference function it is the per-document form of
    header = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "plsa.py:329-386" in header
    for stated in ("Stored zeros contribute nothing", "plsa_set_arithmetic does NOT affect"):
        assert stated in header, stated


def test_score_sources_are_build_dependencies_and_part_of_the_translation_unit():
    from enstop_amd import build
    deps = {os.path.relpath(d, ROOT) for d in build.DEPS}
    assert {"include/plsa_hip_score.h", "enstop_amd/csrc/plsa_score_kernels.hpp", "enstop_amd/csrc/plsa_score.hpp"} <= deps
    unit = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_hip.hip")).read()
    tail = unit[unit.index('#include "plsa_nmf.hpp"'):]
    assert '#include "plsa_score_kernels.hpp"' in tail and '#include "plsa_score.hpp"' in tail
    data = open(os.path.join(ROOT, "enstop_amd", "libplsa_hip.so"), "rb").read()
    assert b"k_score_rows" in data
