"""CPU-only checks of the boundary of online variational Bayes LDA: the six entry points are declared in
enstop_amd/include/plsa_hip_lda_online.h and in no header of include/, the header is plain C99, the built library exports them,
enstop_amd/_lib.py binds them in a table of their own with the argument lists the header declares, the sources are build
dependencies and part of the translation unit and run the passes through their wrappers only, the documents and the package
name everything, and the estimator's parameters are the stated ones while LDA's stay as they were."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

HEADER = os.path.join(ROOT, "enstop_amd", "include", "plsa_hip_lda_online.h")
ENTRIES = ["plsa_lda_online_create", "plsa_lda_online_destroy", "plsa_lda_online_fold", "plsa_lda_online_get_lambda",
           "plsa_lda_online_set_lambda", "plsa_lda_online_step"]
COUNTS = {"plsa_lda_online_create": 4, "plsa_lda_online_destroy": 1, "plsa_lda_online_set_lambda": 2,
          "plsa_lda_online_get_lambda": 3, "plsa_lda_online_step": 10, "plsa_lda_online_fold": 6}
SOURCES = ("plsa_lda_online.hpp", "plsa_lda_online_kernels.hpp")
KERNEL = "k_lda_online_blend"


def _strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _symbols(path):
    return sorted(set(re.findall(r"\b(plsa_[a-z0-9_]+)\s*\(", _strip(open(path).read()))))


def test_the_header_declares_exactly_the_six_entry_points_and_is_plain_c99():
    assert _symbols(HEADER) == ENTRIES
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    include = os.path.join(ROOT, "include")
    for header in os.listdir(include):
        assert not set(ENTRIES) & set(_symbols(os.path.join(include, header))), header
    text = open(HEADER).read()
    for stated in ("fmaf(b, n_wz[w, z], fmaf(a, lambda[w, z], c))", "a = (float)(1 - rho), b = (float)(rho scale), c = (float)(rho eta)",
                   "exact 0 at the pads", "scale = D / n_b", "launches nothing", "no second stream", "no hipGraph", "no atomics",
                   "WITHOUT the topic part", "the lambda the step started from", "the only host wait of a step",
                   "plsa_release_scratch", "rho outside (0, 1]", "doc_iter < 1", "There are no sample"):
        assert stated in text, stated


def test_the_library_exports_them_and_their_own_table_binds_them():
    from enstop_amd import _lib
    lib = _lib.load()
    assert sorted(_lib.LDA_ONLINE_SIGNATURES) == ENTRIES
    for name, (res, args) in _lib.LDA_ONLINE_SIGNATURES.items():
        assert hasattr(lib, name), "libplsa_hip.so does not export %s" % name
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype == res            # applied by load()
    for table in (_lib.SIGNATURES, _lib.MEMBER_SIGNATURES, _lib.METRIC_SIGNATURES, _lib.BLOCKED_SIGNATURES, _lib.EMBED_SIGNATURES,
                  _lib.NMF_SIGNATURES, _lib.SCORE_SIGNATURES, _lib.TEMPERED_SIGNATURES, _lib.ONLINE_SIGNATURES,
                  _lib.LDA_PRIOR_SIGNATURES):
        assert not set(ENTRIES) & set(table)
    text = _strip(open(HEADER).read())
    for name, count in COUNTS.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(decl.split(",")) == count == len(_lib.LDA_ONLINE_SIGNATURES[name][1]), name
    step = _lib.LDA_ONLINE_SIGNATURES["plsa_lda_online_step"][1]
    # (state, block, alpha, eta, doc_iter, thresh, rho, scale, flags, &bound_partial): the priors, rho and scale are doubles
    assert step[2:4] == [C.c_double] * 2 and step[4] is C.c_int32 and step[5] is C.c_float and step[6:8] == [C.c_double] * 2
    assert step[9] == C.POINTER(C.c_double)
    assert _lib.LDA_ONLINE_SIGNATURES["plsa_lda_online_destroy"][0] is None
    assert _lib.LDA_ONLINE_SIGNATURES["plsa_lda_online_get_lambda"][1][2] == C.POINTER(C.c_int64)


def test_the_sources_are_build_dependencies_and_part_of_the_translation_unit():
    from enstop_amd import build
    deps = {os.path.relpath(d, ROOT) for d in build.DEPS}
    assert {"enstop_amd/csrc/" + name for name in SOURCES} | {os.path.relpath(HEADER, ROOT)} <= deps
    unit = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_hip.hip")).read()
    assert '#include "../include/plsa_hip_lda_online.h"' in unit
    tail = unit[unit.index('#include "plsa_lda_priors.hpp"'):]          # behind the priors
    for name in ("plsa_lda_online_kernels.hpp", "plsa_lda_online.hpp"):
        assert '#include "%s"' % name in tail, name
    data = open(os.path.join(ROOT, "enstop_amd", "libplsa_hip.so"), "rb").read()
    assert KERNEL.encode() in data
    # the state's buffers are the state's: a block context's release names none of them
    release = unit[unit.index("int plsa_release_scratch("):unit.index("int plsa_timing_enable(")]
    assert "online" not in release


def _csrc(name):
    return re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "enstop_amd", "csrc", name)).read())


def _all_csrc():
    folder = os.path.join(ROOT, "enstop_amd", "csrc")
    return {name: _csrc(name) for name in sorted(os.listdir(folder)) if name.endswith((".hpp", ".hip"))}


def test_the_passes_run_through_their_wrappers():
    """no pass kernel, no stream creation, no graph call and no atomic is named in the online LDA sources or in the two host
    sides they share code with; the round, the tables and the bound are plsa_lda.hpp's, the state frame with its event
    discipline is plsa_online.hpp's, and each is named by the file that holds it"""
    for name in SOURCES + ("plsa_lda.hpp", "plsa_lda_priors.hpp", "plsa_online.hpp"):
        code = _csrc(name)
        for word in ("k_row_pass<", "k_col_pass<", "k_col_reduce_norm<", "k_loglik<", "hipStreamCreate", "hipGraph", "atomic"):
            assert word not in code, (name, word)
    host, lda, frame = _csrc("plsa_lda_online.hpp"), _csrc("plsa_lda.hpp"), _csrc("plsa_online.hpp")
    for used in ("run_row_pass(", "run_col_pass(c, false, nullptr, thresh, 3)", "run_loglik(c, nullptr, nullptr)", "wait_ll(",
                 "StandIn u(", "run_lda_table_u(", "run_lda_table_v(", "run_lda_rows(c, alpha)", "run_lda_dirichlet<true>(",
                 "run_lda_shift_sum(", "lda_prior_ok(", "plsa::k_lda_topic_sums", "plsa::k_lda_wordmax", "plsa::k_lda_tables<false>"):
        assert used in lda, used
    for used in ("plain_fused_refusal(", "need_factors(", "hipStreamWaitEvent(c->stream, st->ev, 0)", "hipEventRecord(st->ev, c->stream)"):
        assert used in frame, used
    # ... and the online side reaches every one of them through the shared pieces
    for used in ("lda_rounds(", "lda_scalar_rows(c, alpha)", "lda_bound_send(", "lda_gamma_part(c, alpha)", "lda_bound_finish(",
                 "run_lda_topic_tables(", "online_frame_eligible(", "online_wait(st, c)", "online_record(st, c)", "online_host_wait(st)",
                 "lda_prior_ok(", "plsa::k_lda_online_blend"):
        assert used in host, used
    # the block's own topic table stays: the online path never asks a round for the topics.  The step leaves the counts in
    # Vacc, the fold runs no column pass; the one round writes and flips Vt under LdaColumns::TOPICS only
    assert "run_lda_topics(" not in host and "c->cv ^= 1" not in host and "LdaColumns::TOPICS" not in host
    step = host[host.index("int plsa_lda_online_step("):host.index("int plsa_lda_online_fold(")]
    fold = host[host.index("int plsa_lda_online_fold("):]
    assert step.count("LdaColumns::") == 1 and "LdaColumns::COUNTS, eta).iteration(doc_iter)" in step
    assert fold.count("LdaColumns::") == 1 and "LdaColumns::NONE" in fold and "rounds.round(false)" in fold
    assert "const bool topics = with_columns && columns == LdaColumns::TOPICS;" in lda
    assert "if (topics) CHK(run_lda_topics(c, eta));" in lda and "if (topics) { c->cv ^= 1; l.b_valid = false; }" in lda
    assert lda.count("c->cv ^= 1") == 1 and lda.count("run_lda_topics(") == 2          # (its definition and the round)
    # the send precedes the global update, the wait follows it
    assert step.index("lda_bound_send(") < step.index("lda_online_global_update(") < step.index("online_record(") \
        < step.index("lda_bound_finish(")
    # one site each in the tree: the event wait and record on the block's stream, the round, the topic-side chain, and the
    # launches of the kernels that belong to one feature
    tree = _all_csrc()
    for once in ("hipStreamWaitEvent(c->stream, st->ev, 0)", "hipEventRecord(st->ev, c->stream)", "int round(bool",
                 "plsa::k_lda_topic_sums,", "plsa::k_lda_topic_partial,", "plsa::k_lda_wordmax,", "plsa::k_lda_tables<false>,",
                 "plsa::" + KERNEL + ",", "plsa::k_lda_rows_v,", "plsa::k_lda_bound_v,"):
        assert sum(code.count(once) for code in tree.values()) == 1, once
    assert "int round(bool" in lda and "plsa::" + KERNEL + "," in host
    assert "plsa::k_lda_rows_v," in tree["plsa_lda_priors.hpp"] and "plsa::k_lda_bound_v," in tree["plsa_lda_priors.hpp"]


def test_the_documents_and_the_package_name_them():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "plsa_hip_lda_online.h" in doc
    for name in ENTRIES:
        assert name in doc, name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 21." in design
    section = design[design.index("## 21."):]
    for word in (KERNEL, "k_lda_topic_partial", "doc_iter", "tau0", "held-out perplexity"):
        assert word in section, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    for word in ("OnlineLDA", "lda_fit_online", "partial_fit", "lda_online_timing"):
        assert word in readme, word
    import enstop_amd
    for name in ("OnlineLDA", "lda_fit_online", "LdaOnlineState"):
        assert name in enstop_amd.__all__ and hasattr(enstop_amd, name), name
    for method in ("set_lambda", "get_lambda", "steps", "step", "fold", "close", "__enter__", "__exit__"):
        assert hasattr(enstop_amd.LdaOnlineState, method), method


def test_the_parameters_of_the_estimators():
    import enstop_amd
    assert enstop_amd.OnlineLDA().get_params() == dict(
        n_components=10, doc_topic_prior=None, topic_word_prior=None, n_iter=100, n_iter_per_test=10, tolerance=0.001, doc_iter=3,
        random_state=None, n_batches=64, n_epochs=5, kappa=0.7, tau0=10.0, rho=None, shuffle_documents=True, total_samples=1e6)
    assert enstop_amd.LDA().get_params() == dict(
        n_components=10, doc_topic_prior=None, topic_word_prior=None, n_iter=100, n_iter_per_test=10, tolerance=0.001, doc_iter=1,
        random_state=None)
    assert issubclass(enstop_amd.OnlineLDA, enstop_amd.LDA)
    for method in ("transform", "score", "perplexity", "held_out_perplexity", "coherence", "log_lift"):
        assert getattr(enstop_amd.OnlineLDA, method) is getattr(enstop_amd.LDA, method), method
