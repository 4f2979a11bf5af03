"""CPU-only checks of the NMF boundary (include/plsa_hip_nmf.h): the header declares exactly the six entry points, the built
library exports them, enstop_amd/_lib.py binds them in a table of its own, INTEGRATION.md documents them with the
scikit-learn functions they stand for, the other headers and tables are untouched, and the header is plain C99."""
import os
import re
import subprocess

from conftest import ROOT

HEADER = "plsa_hip_nmf.h"
ENTRIES = ["plsa_nmf_divergence", "plsa_nmf_fit", "plsa_nmf_get_factors", "plsa_nmf_set_factors", "plsa_nmf_update_h",
           "plsa_nmf_update_w"]
OTHER_HEADERS = ("plsa_hip.h", "plsa_hip_diag.h", "plsa_hip_members.h", "plsa_hip_metrics.h", "plsa_hip_blocked.h",
                 "plsa_hip_embed.h")


def _symbols(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(plsa_[a-z0-9_]+)\s*\(", text)))


def test_nmf_header_declares_exactly_the_entry_points():
    assert _symbols(HEADER) == ENTRIES


def test_nmf_symbols_exported_and_bound_in_their_own_table():
    from enstop_amd import _lib
    lib = _lib.load()
    assert sorted(_lib.NMF_SIGNATURES) == ENTRIES
    for name, (res, args) in _lib.NMF_SIGNATURES.items():
        assert hasattr(lib, name), "libplsa_hip.so does not export %s" % name
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res            # applied by load()
    assert len(_lib.NMF_SIGNATURES["plsa_nmf_fit"][1]) == 7 and len(_lib.NMF_SIGNATURES["plsa_nmf_set_factors"][1]) == 6


def test_nmf_symbols_stay_out_of_the_existing_headers_and_tables():
    from enstop_amd import _lib
    names = set(ENTRIES)
    for other in OTHER_HEADERS:
        assert not names & set(_symbols(other)), other
    for table in (_lib.SIGNATURES, _lib.MEMBER_SIGNATURES, _lib.METRIC_SIGNATURES, _lib.BLOCKED_SIGNATURES, _lib.EMBED_SIGNATURES):
        assert not names & set(table)
    assert sorted(_lib.SIGNATURES) == sorted(set(_symbols("plsa_hip.h")) | set(_symbols("plsa_hip_diag.h")))


def test_nmf_entry_points_are_documented_with_the_functions_they_stand_for():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert HEADER in doc
    for name in ENTRIES:
        assert name in doc, name
    for cited in ("_multiplicative_update_w", "_multiplicative_update_h", "_beta_divergence", "_fit_multiplicative_update"):
        assert cited in doc, cited
        assert cited in open(os.path.join(ROOT, "include", HEADER)).read(), cited


def test_nmf_header_is_plain_c99():
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c",
                          os.path.join(ROOT, "include", HEADER)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_nmf_sources_are_build_dependencies():
    from enstop_amd import build
    deps = {os.path.relpath(d, ROOT) for d in build.DEPS}
    assert {"include/plsa_hip_nmf.h", "enstop_amd/csrc/plsa_nmf_kernels.hpp", "enstop_amd/csrc/plsa_nmf.hpp"} <= deps
