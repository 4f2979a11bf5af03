"""CPU-only checks of the batched-members boundary (include/plsa_hip_members.h): every plsa_members_* entry point the
header declares is exported by the built library, bound in the member table of enstop_amd/_lib.py and documented in
INTEGRATION.md; the drop-in header and its binding table are untouched by it.  No device computation here."""
import os
import re

import pytest

from conftest import ROOT


def _symbols(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(plsa_[a-z0-9_]+)\s*\(", text)))


def test_member_header_declares_only_member_entry_points():
    names = _symbols("plsa_hip_members.h")
    assert len(names) >= 5
    assert all(n.startswith("plsa_members_") for n in names), names
    for needed in ("plsa_members_create", "plsa_members_prepare", "plsa_members_fit", "plsa_members_copy_components",
                   "plsa_members_destroy"):
        assert needed in names, needed


def test_member_symbols_exported_and_bound_in_their_own_table():
    from enstop_amd import _lib
    lib = _lib.load()
    names = _symbols("plsa_hip_members.h")
    for name in names:
        assert hasattr(lib, name), "libplsa_hip.so does not export %s" % name
        assert name in _lib.MEMBER_SIGNATURES, "member table lacks %s" % name
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.MEMBER_SIGNATURES[name][1]      # applied by load()
    assert sorted(_lib.MEMBER_SIGNATURES) == names


def test_member_symbols_stay_out_of_the_existing_headers_and_table():
    from enstop_amd import _lib
    names = set(_symbols("plsa_hip_members.h"))
    main, diag = _symbols("plsa_hip.h"), _symbols("plsa_hip_diag.h")
    assert len(main) <= 40, len(main)
    assert not names & set(main) and not names & set(diag)
    assert not names & set(_lib.SIGNATURES)
    assert not [s for s in _lib.SIGNATURES if s.startswith("plsa_members_")]
    assert sorted(_lib.SIGNATURES) == sorted(set(main) | set(diag))


def test_member_entry_points_are_documented_with_the_interface_they_stand_for():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    missing = [s for s in _symbols("plsa_hip_members.h") if s not in doc]
    assert not missing, missing
    assert "plsa_hip_members.h" in doc and "enstop_.py:164-231" in doc


def test_batched_is_a_recognised_parallelism():
    from enstop_amd import enstop_
    assert enstop_.PARALLELISM == ("dask", "joblib", "none", "batched")
    assert enstop_._batched_requested("batched") and not enstop_._batched_requested("none")
    assert "batched" in enstop_._ensemble_of_plsa_topics.__doc__


def test_environment_switch_and_batch_cap(monkeypatch):
    from enstop_amd import enstop_
    monkeypatch.delenv("ENSTOP_AMD_ENSEMBLE", raising=False)
    assert not enstop_._batched_requested("dask")
    monkeypatch.setenv("ENSTOP_AMD_ENSEMBLE", "batched")
    assert enstop_._batched_requested("dask") and enstop_._batched_requested("joblib") and not enstop_._batched_requested("none")
    monkeypatch.delenv("ENSTOP_AMD_BATCH_MEMBERS", raising=False)
    assert enstop_.batch_members_cap() == 32
    for given, want in (("5", 5), ("1", 1), ("64", 64), ("500", 64), ("0", 1)):
        monkeypatch.setenv("ENSTOP_AMD_BATCH_MEMBERS", given)
        assert enstop_.batch_members_cap() == want
