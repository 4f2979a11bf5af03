"""CPU-only checks of the smoothed-EM boundary: the three entry points are declared in include/plsa_hip_diag.h (a section of
its own) and nowhere else, the built library exports them, enstop_amd/_lib.py binds them in SIGNATURES, the sources are build
dependencies and part of the translation unit and run the passes through their wrappers only, the documents name them, and the
Python layer keeps PLSA's parameter list, carries set values through clone and pickle and refuses what has no smoothed form
before an engine is touched."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT

ENTRIES = ["plsa_fit_smoothed", "plsa_log_posterior", "plsa_refit_smoothed"]
SOURCES = ("plsa_smoothed.hpp", "plsa_smoothed_kernels.hpp", "plsa_smoothed_plan.hpp")


def _symbols(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(plsa_[a-z0-9_]+)\s*\(", text)))


def test_the_three_symbols_are_declared_in_the_diagnostics_header_and_nowhere_else():
    assert set(ENTRIES) <= set(_symbols("plsa_hip_diag.h"))
    for header in os.listdir(os.path.join(ROOT, "include")):
        if header != "plsa_hip_diag.h":
            assert not set(ENTRIES) & set(_symbols(header)), header
    text = open(os.path.join(ROOT, "include", "plsa_hip_diag.h")).read()
    section = text[text.index("smoothed (MAP) EM"):]
    for stated in ("P(z|d) = (n_dz + a) / (N_d + k a)", "P(w|z) = (n_wz + b) / (N_z + m b)", "launches nothing",
                   "One stream, no look-ahead buffer set, no hipGraph", "plsa_release_scratch", "bits of plsa_log_likelihood",
                   "A factor entry equal to 0 adds"):
        assert stated in section, stated
    assert len(_symbols("plsa_hip.h")) <= 40


def test_the_library_exports_them_and_signatures_binds_them():
    from enstop_amd import _lib
    lib = _lib.load()
    for name in ENTRIES:
        assert hasattr(lib, name), "libplsa_hip.so does not export %s" % name
        res, args = _lib.SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res
    for table in (_lib.MEMBER_SIGNATURES, _lib.METRIC_SIGNATURES, _lib.BLOCKED_SIGNATURES, _lib.EMBED_SIGNATURES,
                  _lib.NMF_SIGNATURES, _lib.SCORE_SIGNATURES, _lib.TEMPERED_SIGNATURES, _lib.ONLINE_SIGNATURES):
        assert not set(ENTRIES) & set(table)
    fit, refit, post = (_lib.SIGNATURES[name][1] for name in ("plsa_fit_smoothed", "plsa_refit_smoothed", "plsa_log_posterior"))
    plain = _lib.SIGNATURES["plsa_fit"][1]
    # plsa_fit's arguments with `double a, double b` after sw; plsa_refit's with `double a`; (ctx, sw, a, b, double *out)
    assert fit == plain[:2] + [C.c_double, C.c_double] + plain[2:]
    assert refit == _lib.SIGNATURES["plsa_refit"][1][:2] + [C.c_double] + _lib.SIGNATURES["plsa_refit"][1][2:]
    assert len(post) == 5 and post[2] is C.c_double and post[3] is C.c_double


def test_the_sources_are_build_dependencies_and_part_of_the_translation_unit():
    from enstop_amd import build
    deps = {os.path.relpath(d, ROOT) for d in build.DEPS}
    assert {"enstop_amd/csrc/" + name for name in SOURCES} <= deps
    unit = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_hip.hip")).read()
    tail = unit[unit.index('#include "plsa_online.hpp"'):]
    assert '#include "plsa_smoothed_kernels.hpp"' in tail and '#include "plsa_smoothed.hpp"' in tail
    data = open(os.path.join(ROOT, "enstop_amd", "libplsa_hip.so"), "rb").read()
    for kernel in (b"k_smooth_rows", b"k_smooth_topics", b"k_log_prior"):
        assert kernel in data, kernel


def test_the_passes_run_through_their_wrappers():
    """no pass kernel, no stream creation and no graph call is named in the smoothed sources; the norm is the existing kernels'"""
    for name in SOURCES:
        code = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "enstop_amd", "csrc", name)).read())
        for word in ("k_row_pass<", "k_col_pass<", "k_col_reduce_norm<", "k_loglik<", "hipStreamCreate", "hipGraph", "atomic"):
            assert word not in code, (name, word)
    host = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_smoothed.hpp")).read())
    for used in ("run_row_pass(", "run_col_pass(", "run_col_tail(", "run_vacc_norm(", "run_loglik(", "plsa::k_ll_final",
                 "plsa::fit::run_materialised(", "plsa::fit::REFIT", "if (c->comm)"):
        assert used in host, used
    # the helper split out of run_v_normalise keeps that path's launches, in order, under the same timing names
    unit = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_hip.hip")).read()
    helper = unit[unit.index("int run_vacc_norm("):unit.index("int run_v_normalise(")]
    assert helper.index('"k_colsum_partial"') < helper.index('"k_colsum_final"')
    body = unit[unit.index("int run_v_normalise("):unit.index("int run_col_tail(")]
    assert body.index("rccl_allreduce_accumulator") < body.index("run_vacc_norm(c)") < body.index('"k_v_normalise"')
    release = unit[unit.index("int plsa_release_scratch("):unit.index("int plsa_timing_enable(")]
    assert "&c->smoothed.norm_pdz" in release and "&c->smoothed.partials" in release


def test_the_documents_name_them():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in doc, name
    assert "stretches the purpose of that header" in doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 18." in design and "k_smooth_rows" in design and "k_smooth_topics" in design and "k_log_prior" in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "doc_topic_smoothing" in readme and "topic_word_smoothing" in readme and "plsa_fit_smoothed" in readme


def test_the_estimator_keeps_its_parameter_list_and_carries_set_values():
    import enstop_amd
    from sklearn.base import clone
    for name in ("plsa_fit_smoothed", "plsa_refit_smoothed"):
        assert name in enstop_amd.__all__ and hasattr(enstop_amd, name)
    plain = enstop_amd.PLSA().get_params()
    assert "doc_topic_smoothing" not in plain and "topic_word_smoothing" not in plain and "tempering" not in plain
    assert sorted(plain) == sorted(["n_components", "init", "n_iter", "n_iter_per_test", "tolerance", "e_step_thresh",
                                    "transform_random_seed", "random_state", "device", "arithmetic", "p_budget"])
    import inspect
    assert list(inspect.signature(enstop_amd.PLSA.__init__).parameters)[-3:] == ["tempering", "doc_topic_smoothing",
                                                                                 "topic_word_smoothing"]
    model = enstop_amd.PLSA(n_components=5, doc_topic_smoothing=0.1, topic_word_smoothing=0.01)
    params = model.get_params()
    assert params["doc_topic_smoothing"] == 0.1 and params["topic_word_smoothing"] == 0.01 and "tempering" not in params
    for copy in (clone(model), pickle.loads(pickle.dumps(model))):
        assert copy.get_params() == params and copy.n_components == 5
    one = enstop_amd.PLSA(topic_word_smoothing=0.5)
    assert "doc_topic_smoothing" not in one.get_params() and clone(one).topic_word_smoothing == 0.5
    assert enstop_amd.PLSA().set_params(doc_topic_smoothing=0.2).doc_topic_smoothing == 0.2
    assert model._smoothing() == (0.1, 0.01) and enstop_amd.PLSA()._smoothing() == (0.0, 0.0)
    assert "doc_topic_smoothing" in inspect.signature(enstop_amd.held_out_scores).parameters
    assert list(inspect.signature(enstop_amd.held_out_scores).parameters)[-1] == "doc_topic_smoothing"


def test_the_python_refusals_come_before_any_engine(monkeypatch):
    import enstop_amd
    from enstop_amd import engine, plsa, scoring, smoothed

    def no_engine(*args, **kwargs):
        raise AssertionError("an engine was asked for")
    for module in (engine, plsa, scoring, smoothed):
        monkeypatch.setattr(module, "get_engine", no_engine)
    X = sp.random(12, 9, density=0.5, format="csr", random_state=0, dtype=np.float32)
    nan = float("nan")
    for kw in (dict(doc_topic_smoothing=-0.1), dict(topic_word_smoothing=-1), dict(doc_topic_smoothing=nan),
               dict(topic_word_smoothing=float("inf")), dict(doc_topic_smoothing="a lot"), dict(topic_word_smoothing=True),
               dict(doc_topic_smoothing=0.1, tempering="auto"), dict(topic_word_smoothing=0.1, tempering=0.9),
               dict(doc_topic_smoothing=0.1, arithmetic="reference"), dict(topic_word_smoothing=0.1, arithmetic="reference_source")):
        with pytest.raises(ValueError):
            enstop_amd.PLSA(n_components=3, **kw).fit(X)
    for cls in (enstop_amd.StreamedPLSA, enstop_amd.BlockParallelPLSA, enstop_amd.GPUPLSA, enstop_amd.DistributedPLSA,
                enstop_amd.OnlinePLSA):
        est = cls(n_components=3)
        assert "doc_topic_smoothing" not in est.get_params()
        est.doc_topic_smoothing = 0.1
        with pytest.raises(ValueError, match="PLSA only"):
            est.fit(X)
    for kw in (dict(doc_topic_smoothing=-1.0), dict(topic_word_smoothing=nan), dict(doc_topic_smoothing=0.1, flags=0),
               dict(doc_topic_smoothing=0.1, flags=1 | 256), dict(topic_word_smoothing=0.1, flags=1 | 512)):
        with pytest.raises(ValueError):
            enstop_amd.plsa_fit_smoothed(X, 3, None, **kw)
    with pytest.raises(ValueError):
        enstop_amd.plsa_refit_smoothed(X, np.full((3, 9), 1 / 9, np.float32), None, -0.5)
    with pytest.raises(ValueError):
        enstop_amd.held_out_scores(X, np.full((3, 9), 1 / 9, np.float32), doc_topic_smoothing=-0.5)
    for flags in (0, 1 | 256, 1 | 512):          # the fold-in of a smoothed model: flags without a smoothed form
        with pytest.raises(ValueError):
            enstop_amd.held_out_scores(X, np.full((3, 9), 1 / 9, np.float32), doc_topic_smoothing=0.1, flags=flags)
        with pytest.raises(ValueError):
            enstop_amd.plsa_refit_smoothed(X, np.full((3, 9), 1 / 9, np.float32), None, 0.1, flags=flags)

    class Untouchable:                           # _refit_on_engine itself refuses before its first call on the engine
        def __getattr__(self, name):
            raise AssertionError("the engine was touched: %s" % name)
    with pytest.raises(ValueError):
        plsa._refit_on_engine(Untouchable(), X, np.full((3, 9), 1 / 9, np.float32), None, 5, 5, 0.0, 1e-32,
                              np.random.RandomState(0), 0, doc_topic_smoothing=0.1)
    # a fitted smoothed model refuses a bad value at transform time as well
    model = enstop_amd.PLSA(n_components=3, doc_topic_smoothing=0.1)
    model.components_ = np.full((3, 9), 1 / 9, np.float32)
    model.doc_topic_smoothing = -2
    with pytest.raises(ValueError):
        model.transform(X)
