"""CPU-only checks of the memory-plumbing boundary include/plsa_hip_blocked.h (the reference arithmetic under a P(z|w,d)
budget): the header declares exactly plsa_set_p_budget and plsa_p_block_info, the built library exports them,
enstop_amd/_lib.py binds them in a table of its own, the drop-in headers and their table do not know them, INTEGRATION.md
names them, and `p_budget=` is a keyword of the fit functions and the estimator.  No device computation here."""
import inspect
import os
import re
import subprocess

from conftest import ROOT

HEADER = "plsa_hip_blocked.h"
NAMES = ["plsa_p_block_info", "plsa_set_p_budget"]


def _symbols(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(plsa_[a-z0-9_]+)\s*\(", text)))


def test_blocked_header_declares_exactly_the_two_entry_points():
    assert _symbols(HEADER) == NAMES


def test_blocked_symbols_exported_and_bound_in_their_own_table():
    from enstop_amd import _lib
    lib = _lib.load()
    assert sorted(_lib.BLOCKED_SIGNATURES) == NAMES
    for name, (res, args) in _lib.BLOCKED_SIGNATURES.items():
        assert hasattr(lib, name), "libplsa_hip.so does not export %s" % name
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res            # applied by load()
    assert len(_lib.BLOCKED_SIGNATURES["plsa_set_p_budget"][1]) == 2
    assert len(_lib.BLOCKED_SIGNATURES["plsa_p_block_info"][1]) == 5


def test_blocked_symbols_stay_out_of_the_other_headers_and_tables():
    from enstop_amd import _lib
    names = set(NAMES)
    for other in ("plsa_hip.h", "plsa_hip_diag.h", "plsa_hip_members.h", "plsa_hip_metrics.h"):
        assert not names & set(_symbols(other)), other
    assert not names & (set(_lib.SIGNATURES) | set(_lib.MEMBER_SIGNATURES) | set(_lib.METRIC_SIGNATURES))


def test_blocked_entry_points_are_documented_as_memory_plumbing():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in doc for name in NAMES) and HEADER in doc
    # the flag's comment in the drop-in header no longer says that the mode needs the whole array
    assert "plsa_set_p_budget" in open(os.path.join(ROOT, "include", "plsa_hip.h")).read()


def test_blocked_header_is_plain_c():
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c",
                          os.path.join(ROOT, "include", HEADER)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_p_budget_is_a_keyword_of_the_fit_functions_and_the_estimator():
    import enstop_amd
    from enstop_amd import plsa
    for fn in (plsa.plsa_fit, plsa.plsa_refit):
        p = inspect.signature(fn).parameters["p_budget"]
        assert p.default is None and p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
        assert list(inspect.signature(fn).parameters)[-1] == "p_budget"        # appended: positional compatibility unchanged
    est = enstop_amd.PLSA(arithmetic="reference", p_budget=1 << 20)
    assert est.get_params()["p_budget"] == 1 << 20 and enstop_amd.PLSA().p_budget is None
    for name in ("set_p_budget", "p_block_info"):
        assert callable(getattr(enstop_amd.Engine, name))
