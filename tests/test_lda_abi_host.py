"""CPU-only checks of the LDA boundary: the four entry points are declared in include/plsa_hip_diag.h (a section of their own
behind smoothed EM's, for the reason INTEGRATION.md gives there) and nowhere else, the built library exports them,
enstop_amd/_lib.py binds them in SIGNATURES with the argument lists the header declares, the sources are build dependencies and
part of the translation unit and run the passes through their wrappers only, and the documents name them."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

HEADER = "plsa_hip_diag.h"
ENTRIES = ["plsa_lda_bound", "plsa_lda_fit", "plsa_lda_refit", "plsa_lda_tables"]
SOURCES = ("plsa_lda.hpp", "plsa_lda_kernels.hpp", "plsa_lda_plan.hpp", "plsa_lda_math.hpp")
KERNELS = ("k_lda_tables", "k_lda_rows", "k_lda_topics", "k_lda_bound", "k_lda_rowsum", "k_lda_wordmax", "k_lda_topic_partial",
           "k_lda_topic_sums", "k_lda_shift_sum")


def _symbols(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(plsa_[a-z0-9_]+)\s*\(", text)))


def test_the_four_symbols_are_declared_in_the_diagnostics_header_and_nowhere_else():
    assert set(ENTRIES) <= set(_symbols(HEADER))
    assert [name for name in _symbols(HEADER) if name.startswith("plsa_lda")] == ENTRIES
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", HEADER)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    for header in os.listdir(os.path.join(ROOT, "include")):
        if header != HEADER:
            assert not set(ENTRIES) & set(_symbols(header)), header
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    section = text[text.index("variational Bayes LDA"):]
    for stated in ("gamma_dz = alpha + sum_w x_dw phi_dwz", "lambda_zw = eta + sum_d x_dw phi_dwz", "launches nothing",
                   "One stream, no look-ahead buffer set, no hipGraph", "plsa_release_scratch", "the bound never decreases",
                   "largest entry of every such row is 1", "no sample weights"):
        assert stated in section, stated
    assert len(_symbols("plsa_hip.h")) <= 40


def test_the_library_exports_them_and_signatures_binds_them():
    from enstop_amd import _lib
    lib = _lib.load()
    for name in ENTRIES:
        assert hasattr(lib, name), "libplsa_hip.so does not export %s" % name
        res, args = _lib.SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res            # applied by load()
    for table in (_lib.MEMBER_SIGNATURES, _lib.METRIC_SIGNATURES, _lib.BLOCKED_SIGNATURES, _lib.EMBED_SIGNATURES,
                  _lib.NMF_SIGNATURES, _lib.SCORE_SIGNATURES, _lib.TEMPERED_SIGNATURES, _lib.ONLINE_SIGNATURES):
        assert not set(ENTRIES) & set(table)
    fit, refit = _lib.SIGNATURES["plsa_lda_fit"][1], _lib.SIGNATURES["plsa_lda_refit"][1]
    plain = _lib.SIGNATURES["plsa_fit"][1]
    # plsa_fit's arguments without sw: (ctx, alpha, eta, n_iter, n_iter_per_test, tolerance, doc_iter, thresh, flags, ...)
    assert fit == plain[:1] + [C.c_double, C.c_double] + plain[2:5] + [C.c_int32] + plain[5:]
    assert refit == fit[:2] + fit[3:]                               # the same without eta
    bound, tables = _lib.SIGNATURES["plsa_lda_bound"][1], _lib.SIGNATURES["plsa_lda_tables"][1]
    assert len(bound) == 5 and bound[1] is C.c_double and bound[2] is C.c_double and len(tables) == 3
    # the declarations say the same
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    for name, count in (("plsa_lda_fit", 12), ("plsa_lda_refit", 11), ("plsa_lda_bound", 5), ("plsa_lda_tables", 3)):
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(decl.split(",")) == count == len(_lib.SIGNATURES[name][1]), name


def test_the_sources_are_build_dependencies_and_part_of_the_translation_unit():
    from enstop_amd import build
    deps = {os.path.relpath(d, ROOT) for d in build.DEPS}
    assert {"enstop_amd/csrc/" + name for name in SOURCES} | {"include/" + HEADER} <= deps
    unit = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_hip.hip")).read()
    tail = unit[unit.index('#include "plsa_smoothed.hpp"'):]
    assert '#include "plsa_lda_kernels.hpp"' in tail and '#include "plsa_lda.hpp"' in tail
    data = open(os.path.join(ROOT, "enstop_amd", "libplsa_hip.so"), "rb").read()
    for kernel in KERNELS:
        assert kernel.encode() in data, kernel
    release = unit[unit.index("int plsa_release_scratch("):unit.index("int plsa_timing_enable(")]
    for buffer in ("&c->lda.A", "&c->lda.B", "&c->lda.sums", "&c->lda.norm_pdz", "&c->lda.partials", "&c->lda.out", "c->lda.h_out.reset()"):
        assert buffer in release, buffer


def test_the_passes_run_through_their_wrappers():
    """no pass kernel, no stream creation, no graph call and no atomic is named in the LDA sources"""
    for name in SOURCES:
        code = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "enstop_amd", "csrc", name)).read())
        for word in ("k_row_pass<", "k_col_pass<", "k_col_reduce_norm<", "k_loglik<", "hipStreamCreate", "hipGraph", "atomic"):
            assert word not in code, (name, word)
    host = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_lda.hpp")).read())
    for used in ("run_row_pass(", "run_col_pass(c, false, nullptr, thresh, 3)", "run_loglik(", "plsa::k_ll_final", "StandIn u(",
                 "plsa::fit::run_materialised(", "plsa::fit::REFIT", "if (c->comm)", "plain_fused_refusal(", "fit_open(", "fit_run("):
        assert used in host, used


def test_the_documents_and_the_package_name_them():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in doc, name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 19." in design
    for kernel in KERNELS:
        assert kernel in design, kernel
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "doc_topic_prior" in readme and "lda_fit" in readme and "lda_timing" in readme
    import enstop_amd
    for name in ("LDA", "lda_fit", "lda_transform"):
        assert name in enstop_amd.__all__ and hasattr(enstop_amd, name)
    for method in ("lda_fit", "lda_refit", "lda_bound", "lda_tables"):
        assert hasattr(enstop_amd.Engine, method)
    from sklearn.base import clone
    model = enstop_amd.LDA(n_components=7, doc_topic_prior=0.1)
    assert clone(model).get_params() == model.get_params()
    assert list(model.get_params()) == sorted(["n_components", "doc_topic_prior", "topic_word_prior", "n_iter", "n_iter_per_test",
                                               "tolerance", "doc_iter", "random_state"])
