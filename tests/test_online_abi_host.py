"""CPU-only checks of the online-EM boundary (include/plsa_hip_online.h): the header declares exactly the eight entry points
and is plain C99, the built library exports them, enstop_amd/_lib.py binds them in a table of its own, the other tables and
headers do not know them, the drop-in header is as small as it was, and INTEGRATION.md and DESIGN.md document them."""
import os
import re
import subprocess

from conftest import ROOT

HEADER = "plsa_hip_online.h"
ENTRIES = ["plsa_online_create", "plsa_online_destroy", "plsa_online_fold", "plsa_online_get_topics", "plsa_online_set_topics",
           "plsa_online_statistic_get", "plsa_online_statistic_set", "plsa_online_step"]
OTHER_HEADERS = ("plsa_hip.h", "plsa_hip_diag.h", "plsa_hip_members.h", "plsa_hip_metrics.h", "plsa_hip_blocked.h",
                 "plsa_hip_embed.h", "plsa_hip_nmf.h", "plsa_hip_score.h", "plsa_hip_tempered.h")


def _symbols(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(plsa_[a-z0-9_]+)\s*\(", text)))


def test_online_header_declares_exactly_the_eight_entry_points():
    assert _symbols(HEADER) == ENTRIES
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == sorted(OTHER_HEADERS + (HEADER,))


def test_online_header_is_plain_c99():
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c",
                          os.path.join(ROOT, "include", HEADER)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_online_symbols_exported_and_bound_in_their_own_table_only():
    import ctypes as C
    from enstop_amd import _lib
    lib = _lib.load()
    assert sorted(_lib.ONLINE_SIGNATURES) == ENTRIES
    for name, (res, args) in _lib.ONLINE_SIGNATURES.items():
        assert hasattr(lib, name), "libplsa_hip.so does not export %s" % name
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res            # applied by load()
    step = _lib.ONLINE_SIGNATURES["plsa_online_step"][1]
    # (state, block context, sw, inner_iter, thresh, rho, scale, flags, ll_partial): the step size and the scale are doubles
    assert len(step) == 9 and step[5] is C.c_double and step[6] is C.c_double and step[4] is C.c_float
    assert len(_lib.ONLINE_SIGNATURES["plsa_online_fold"][1]) == 6
    for table in (_lib.SIGNATURES, _lib.MEMBER_SIGNATURES, _lib.METRIC_SIGNATURES, _lib.BLOCKED_SIGNATURES,
                  _lib.EMBED_SIGNATURES, _lib.NMF_SIGNATURES, _lib.SCORE_SIGNATURES, _lib.TEMPERED_SIGNATURES):
        assert not set(ENTRIES) & set(table)
    for other in OTHER_HEADERS:
        assert not set(ENTRIES) & set(_symbols(other)), other


def test_the_drop_in_header_is_as_it_was():
    from enstop_amd import _lib
    assert sorted(_lib.SIGNATURES) == sorted(set(_symbols("plsa_hip.h")) | set(_symbols("plsa_hip_diag.h")))
    assert len(_symbols("plsa_hip.h")) <= 40
    assert "online" not in open(os.path.join(ROOT, "include", "plsa_hip.h")).read()


def test_online_entry_points_are_documented_with_what_they_stand_for():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert HEADER in doc
    for name in ENTRIES:
        assert name in doc, name
    header = open(os.path.join(ROOT, "include", HEADER)).read()
    for stated in ("Cappe & Moulines 2009", "fmaf(b, Vacc, a * S)", "(float)(1 - rho)", "(float)(rho * scale)",
                   "One stream, no look-ahead buffer set, no hipGraph", "launches nothing", "plsa_release_scratch",
                   "no host wait unless ll_partial"):
        assert stated in header, stated
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 17." in design and "k_online_blend" in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "plsa_fit_online" in readme and "partial_fit" in readme


def test_online_sources_are_build_dependencies_and_part_of_the_translation_unit():
    from enstop_amd import build
    deps = {os.path.relpath(d, ROOT) for d in build.DEPS}
    assert {"include/plsa_hip_online.h", "enstop_amd/csrc/plsa_online_kernels.hpp", "enstop_amd/csrc/plsa_online.hpp",
            "enstop_amd/csrc/plsa_online_plan.hpp"} <= deps
    unit = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_hip.hip")).read()
    tail = unit[unit.index('#include "plsa_tempered.hpp"'):]
    assert '#include "plsa_online_kernels.hpp"' in tail and '#include "plsa_online.hpp"' in tail
    data = open(os.path.join(ROOT, "enstop_amd", "libplsa_hip.so"), "rb").read()
    assert b"k_online_blend" in data


def test_the_step_runs_the_existing_passes_and_normalisation_through_their_wrappers():
    """no pass kernel is named in the online sources; the norm and the division are the existing kernels, launched unchanged"""
    for name in ("plsa_online.hpp", "plsa_online_kernels.hpp", "plsa_online_plan.hpp"):
        text = open(os.path.join(ROOT, "enstop_amd", "csrc", name)).read()
        code = re.sub(r"//[^\n]*", "", text)
        for kernel in ("k_row_pass<", "k_col_pass<", "k_col_reduce_norm<", "k_loglik<", "hipStreamCreate", "hipGraph"):
            assert kernel not in code, (name, kernel)
    host = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_online.hpp")).read())
    assert "plsa::k_colsum_final" in host and "plsa::k_v_normalise" in host and "plsa::k_online_blend" in host
    # the state frame (shared with online LDA) lives here: the event wait and record on the block's stream, once each in the tree
    folder = os.path.join(ROOT, "enstop_amd", "csrc")
    tree = "".join(open(os.path.join(folder, name)).read() for name in sorted(os.listdir(folder)))
    for once in ("hipStreamWaitEvent(c->stream, st->ev, 0)", "hipEventRecord(st->ev, c->stream)", "struct OnlineFrame {"):
        assert once in host and tree.count(once) == 1, once
    assert "struct plsa_online : OnlineFrame {" in host


def test_the_package_exports_the_online_module():
    import enstop_amd
    for name in ("OnlinePLSA", "OnlineSchedule", "OnlineState", "plsa_fit_online"):
        assert name in enstop_amd.__all__ and hasattr(enstop_amd, name)
    assert issubclass(enstop_amd.OnlinePLSA, enstop_amd.PLSA)
    params = enstop_amd.OnlinePLSA().get_params()
    assert params["n_batches"] == 64 and params["n_epochs"] == 5 and params["inner_iter"] == 3
    assert params["kappa"] == 0.7 and params["tau0"] == 10.0 and params["rho"] is None and "tempering" not in params
