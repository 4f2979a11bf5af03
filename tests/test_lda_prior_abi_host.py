"""CPU-only checks of the boundary of LDA's vector and learned priors: the four entry points are declared in
enstop_amd/include/plsa_hip_lda_priors.h and in no header of include/, the header is plain C99, the built library exports them,
enstop_amd/_lib.py binds them in a table of their own with the argument lists the header declares, the sources are build
dependencies and part of the translation unit and run the passes through their wrappers only, the scratch is released, and the
documents name them."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

HEADER = os.path.join(ROOT, "enstop_amd", "include", "plsa_hip_lda_priors.h")
ENTRIES = ["plsa_lda_prior_bound", "plsa_lda_prior_fit", "plsa_lda_prior_refit", "plsa_lda_prior_stats"]
COUNTS = {"plsa_lda_prior_fit": 15, "plsa_lda_prior_refit": 11, "plsa_lda_prior_bound": 5, "plsa_lda_prior_stats": 3}
SOURCES = ("plsa_lda_priors.hpp", "plsa_lda_prior_kernels.hpp", "plsa_lda_prior_plan.hpp", "plsa_lda_prior_math.hpp")
KERNELS = ("k_lda_logmean", "k_lda_logmean_sums", "k_lda_rows_v", "k_lda_bound_v")


def _strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _symbols(path):
    return sorted(set(re.findall(r"\b(plsa_[a-z0-9_]+)\s*\(", _strip(open(path).read()))))


def test_the_header_declares_exactly_the_four_entry_points_and_is_plain_c99():
    assert _symbols(HEADER) == ENTRIES
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    include = os.path.join(ROOT, "include")
    for header in os.listdir(include):
        assert not set(ENTRIES) & set(_symbols(os.path.join(include, header))), header
    text = open(HEADER).read()
    for stated in ("gamma_dz = alpha_z + sum_w x_dw phi_dwz", "F(alpha) = n [lgamma(sum_z alpha_z) - sum_z lgamma(alpha_z)] + sum_z alpha_z T_z",
                   "launches nothing", "One stream, no look-ahead buffer set, no hipGraph", "plsa_release_scratch", "1e-6",
                   "prior_start is the burn-in", "cannot stop the loop before", "no sample weights"):
        assert stated in text, stated


def test_the_library_exports_them_and_their_own_table_binds_them():
    from enstop_amd import _lib
    lib = _lib.load()
    assert sorted(_lib.LDA_PRIOR_SIGNATURES) == ENTRIES
    for name, (res, args) in _lib.LDA_PRIOR_SIGNATURES.items():
        assert hasattr(lib, name), "libplsa_hip.so does not export %s" % name
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res            # applied by load()
    for table in (_lib.SIGNATURES, _lib.MEMBER_SIGNATURES, _lib.METRIC_SIGNATURES, _lib.BLOCKED_SIGNATURES, _lib.EMBED_SIGNATURES,
                  _lib.NMF_SIGNATURES, _lib.SCORE_SIGNATURES, _lib.TEMPERED_SIGNATURES, _lib.ONLINE_SIGNATURES):
        assert not set(ENTRIES) & set(table)
    text = _strip(open(HEADER).read())
    for name, count in COUNTS.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(decl.split(",")) == count == len(_lib.LDA_PRIOR_SIGNATURES[name][1]), name
    fit, refit = _lib.LDA_PRIOR_SIGNATURES["plsa_lda_prior_fit"][1], _lib.LDA_PRIOR_SIGNATURES["plsa_lda_prior_refit"][1]
    scalar = _lib.SIGNATURES["plsa_lda_fit"][1]
    # (ctx, alpha [k], &eta, learn, prior_start, prior_every) and then the scalar fit's arguments behind its two priors
    assert fit[2] == C.POINTER(C.c_double) and fit[3:6] == [C.c_int32] * 3 and fit[6:] == scalar[3:]
    assert refit[2:] == _lib.SIGNATURES["plsa_lda_refit"][1][2:]
    bound = _lib.LDA_PRIOR_SIGNATURES["plsa_lda_prior_bound"][1]
    assert bound[2] is C.c_double and bound[4] == C.POINTER(C.c_double)


def test_the_sources_are_build_dependencies_and_part_of_the_translation_unit():
    from enstop_amd import build
    deps = {os.path.relpath(d, ROOT) for d in build.DEPS}
    assert {"enstop_amd/csrc/" + name for name in SOURCES} | {os.path.relpath(HEADER, ROOT)} <= deps
    unit = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_hip.hip")).read()
    assert '#include "../include/plsa_hip_lda_priors.h"' in unit
    tail = unit[unit.index('#include "plsa_lda.hpp"'):]
    for name in ("plsa_lda_prior_math.hpp", "plsa_lda_prior_kernels.hpp", "plsa_lda_priors.hpp"):
        assert '#include "%s"' % name in tail, name
    data = open(os.path.join(ROOT, "enstop_amd", "libplsa_hip.so"), "rb").read()
    for kernel in KERNELS:
        assert kernel.encode() in data, kernel
    release = unit[unit.index("int plsa_release_scratch("):unit.index("int plsa_timing_enable(")]
    for buffer in ("&c->lda_prior.alpha", "&c->lda_prior.partials", "&c->lda_prior.t", "c->lda_prior.h.reset()"):
        assert buffer in release, buffer


def test_the_passes_run_through_their_wrappers():
    """no pass kernel, no stream creation, no graph call and no atomic is named in the new sources; the math and the plan are
    free of HIP"""
    for name in SOURCES:
        code = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "enstop_amd", "csrc", name)).read())
        for word in ("k_row_pass<", "k_col_pass<", "k_col_reduce_norm<", "k_loglik<", "hipStreamCreate", "hipGraph", "atomic"):
            assert word not in code, (name, word)
        if name in ("plsa_lda_prior_plan.hpp", "plsa_lda_prior_math.hpp"):
            assert "hip" not in code.replace("__HIPCC__", "").lower(), name
    host = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_lda_priors.hpp")).read())
    for used in ("plsa::k_ll_final", "plsa::fit::REFIT", "lda_context_ok(", "lda_eligible(", "fit_open(", "fit_run(", "run_lda_table_u(",
                 "run_lda_table_v(", "plsa::lda::maximise_alpha(", "plsa::lda::maximise_eta(", "plsa::plan::prior_due(",
                 # the round and the bound are plsa_lda.hpp's, entered with the vector forms of the rows step and of gamma's part
                 "lda_rounds(c, thresh, [this] { return run_lda_rows_v(c); }", "lda_bound_send(c, \"plsa_lda_prior_bound\", [c] { return run_lda_dirichlet_v(c); }",
                 "lda_bound_finish(c, lgamma(sum) - each,"):
        assert used in host, used
    assert "int round(" not in host and "int iteration()" in host
    scalar = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_lda.hpp")).read())
    for used in ("run_row_pass(", "run_col_pass(c, false, nullptr, thresh, 3)", "run_loglik(", "StandIn u(", "run_lda_table_u(",
                 "run_lda_table_v(", "CHK(rows());", "CHK(gamma_part());"):
        assert used in scalar, used
    # the scalar entry points' host side names none of the new kernels: each is launched from one place, this feature's
    folder = os.path.join(ROOT, "enstop_amd", "csrc")
    for kernel in KERNELS:
        assert kernel not in scalar, kernel
        sites = [name for name in sorted(os.listdir(folder))
                 for _ in range(re.sub(r"//[^\n]*", "", open(os.path.join(folder, name)).read()).count("plsa::" + kernel))]
        assert set(sites) == {"plsa_lda_priors.hpp"}, (kernel, sites)
        assert len(sites) == 1 or kernel == "k_lda_logmean", (kernel, sites)          # (a prefix of k_lda_logmean_sums)


def test_the_documents_and_the_package_name_them():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "plsa_hip_lda_priors.h" in doc
    for name in ENTRIES:
        assert name in doc, name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 20." in design
    for kernel in KERNELS:
        assert kernel in design, kernel
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert '"auto"' in readme and '"asymmetric"' in readme and "prior_start" in readme and "lda_prior_timing" in readme
    import enstop_amd
    for method in ("lda_prior_fit", "lda_prior_refit", "lda_prior_bound", "lda_prior_stats"):
        assert hasattr(enstop_amd.Engine, method)
