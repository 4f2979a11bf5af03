"""CPU-only checks of the tempered-EM boundary (include/plsa_hip_tempered.h): the header declares exactly the three entry
points and is plain C99, the built library exports them, enstop_amd/_lib.py binds them in a table of its own, the drop-in
table still equals the two drop-in headers (plsa_temper_factors, the diagnostic read-back, is declared in plsa_hip_diag.h and
bound there), the other tables and headers do not know them, and INTEGRATION.md documents them."""
import os
import re
import subprocess

from conftest import ROOT

HEADER = "plsa_hip_tempered.h"
ENTRIES = ["plsa_factors_restore", "plsa_factors_snapshot", "plsa_fit_tempered"]
OTHER_HEADERS = ("plsa_hip.h", "plsa_hip_diag.h", "plsa_hip_members.h", "plsa_hip_metrics.h", "plsa_hip_blocked.h",
                 "plsa_hip_embed.h", "plsa_hip_nmf.h", "plsa_hip_score.h")


def _symbols(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(plsa_[a-z0-9_]+)\s*\(", text)))


def test_tempered_header_declares_exactly_the_three_entry_points():
    assert _symbols(HEADER) == ENTRIES


def test_tempered_header_is_plain_c99():
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c",
                          os.path.join(ROOT, "include", HEADER)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_tempered_symbols_exported_and_bound_in_their_own_table_only():
    import ctypes as C
    from enstop_amd import _lib
    lib = _lib.load()
    assert sorted(_lib.TEMPERED_SIGNATURES) == ENTRIES
    for name, (res, args) in _lib.TEMPERED_SIGNATURES.items():
        assert hasattr(lib, name), "libplsa_hip.so does not export %s" % name
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res            # applied by load()
    fit, tempered = _lib.SIGNATURES["plsa_fit"][1], _lib.TEMPERED_SIGNATURES["plsa_fit_tempered"][1]
    assert len(tempered) == 11 and tempered[2] is C.c_double        # plsa_fit's arguments with beta after sw
    assert tempered[:2] + tempered[3:] == fit
    for table in (_lib.SIGNATURES, _lib.MEMBER_SIGNATURES, _lib.METRIC_SIGNATURES, _lib.BLOCKED_SIGNATURES,
                  _lib.EMBED_SIGNATURES, _lib.NMF_SIGNATURES, _lib.SCORE_SIGNATURES):
        assert not set(ENTRIES) & set(table)
    for other in OTHER_HEADERS:
        assert not set(ENTRIES) & set(_symbols(other)), other


def test_drop_in_table_still_equals_the_two_drop_in_headers():
    from enstop_amd import _lib
    assert sorted(_lib.SIGNATURES) == sorted(set(_symbols("plsa_hip.h")) | set(_symbols("plsa_hip_diag.h")))
    assert "plsa_temper_factors" in _symbols("plsa_hip_diag.h") and "plsa_temper_factors" not in _symbols("plsa_hip.h")
    # plsa_hip.h itself is as it was: no temperature in any drop-in entry point
    assert "beta" not in re.sub(r"beta_loss", "", open(os.path.join(ROOT, "include", "plsa_hip.h")).read())


def test_tempered_entry_points_are_documented_with_what_they_stand_for():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert HEADER in doc
    for name in ENTRIES + ["plsa_temper_factors"]:
        assert name in doc, name
    header = open(os.path.join(ROOT, "include", HEADER)).read()
    for stated in ("Hofmann 1999 / 2001", "beta == 1.0 calls plsa_fit", "One stream, no look-ahead buffer set, no hipGraph",
                   "likelihood of the TRUE factors", "launches nothing", "plsa_release_scratch"):
        assert stated in header, stated
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 16." in design and "k_temper" in design


def test_tempered_sources_are_build_dependencies_and_part_of_the_translation_unit():
    from enstop_amd import build
    deps = {os.path.relpath(d, ROOT) for d in build.DEPS}
    assert {"include/plsa_hip_tempered.h", "enstop_amd/csrc/plsa_tempered_kernels.hpp", "enstop_amd/csrc/plsa_tempered.hpp",
            "enstop_amd/csrc/plsa_tempered_plan.hpp"} <= deps
    unit = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_hip.hip")).read()
    tail = unit[unit.index('#include "plsa_score.hpp"'):]
    assert '#include "plsa_tempered_kernels.hpp"' in tail and '#include "plsa_tempered.hpp"' in tail
    data = open(os.path.join(ROOT, "enstop_amd", "libplsa_hip.so"), "rb").read()
    assert b"k_temper" in data


def test_hot_kernels_are_not_touched_by_the_tempered_sources():
    """the tempered iteration runs the passes of plsa_fit through their wrappers: no pass kernel is named in its sources"""
    for name in ("plsa_tempered.hpp", "plsa_tempered_kernels.hpp", "plsa_tempered_plan.hpp"):
        text = open(os.path.join(ROOT, "enstop_amd", "csrc", name)).read()
        code = re.sub(r"//[^\n]*", "", text)
        for kernel in ("k_row_pass<", "k_col_pass<", "k_col_reduce_norm<", "k_loglik<"):
            assert kernel not in code, (name, kernel)
