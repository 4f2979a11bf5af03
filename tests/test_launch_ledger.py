"""Launch ledger of the LDA and online entry points: which kernels each call launches, and how often.

The host sides of variational LDA, LDA with vector priors, online LDA and online EM share one round, one bound, one topic-side
table routine and one online state frame (DESIGN.md sections 17, 19 and 21).  What a call launches must not depend on how that
host code is folded, so every entry point is run once with timing on and its per-kernel launch counts (plsa_timing_report)
are held to tests/golden/launch_ledger_lda_online.json: kernel names and integer counts, recorded with these same calls
before the host sides were folded -- independent of compiler and machine.

The corpus has n = 40 documents, m = 30 words and about 300 non-zeros; k in {6, 64}: kq = 2 with pads, and the 8 x 2 document
shape.  Launches are counted on the context they are timed on: the home engine for plsa_lda_online_set_lambda, the block engine
for steps and folds.
"""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN

K = [6, 64]
N, M = 40, 30
ALPHA, ETA = 0.5, 0.1
THRESH = 1e-32
LEDGER = os.path.join(GOLDEN, "launch_ledger_lda_online.json")


def corpus():
    rs = np.random.RandomState(2024)
    X = sp.random(N, M, density=0.25, format="csr", random_state=rs, dtype=np.float64)
    X.data = np.ceil(X.data * 4)
    return X.astype(np.float32).tocsr()


def start(k):
    rs = np.random.RandomState(77 + k)
    gamma = rs.gamma(100.0, 0.01, (N, k)).astype(np.float32)
    lam = rs.gamma(100.0, 0.01, (k, M)).astype(np.float32)
    topics = (lam / lam.sum(axis=1, keepdims=True)).astype(np.float32)
    docs = (gamma / gamma.sum(axis=1, keepdims=True)).astype(np.float32)
    return gamma, lam, docs, topics


def readings(amd, k):
    """{call: {kernel: launches}} of every entry point of the ledger, each run once from the same start"""
    X = corpus()
    gamma, lam, docs, topics = start(k)
    vec = np.linspace(0.3, 0.7, k)
    out = {}

    def counted(eng, name, call):
        eng.timing_reset()
        call()
        out[name] = {kernel: cnt for kernel, (cnt, _) in sorted(eng.timing_report().items())}

    with amd.Engine() as home, amd.Engine() as eng:
        home.timing(True)
        eng.timing(True)
        eng.upload_csr(X)

        def fresh(u=gamma, v=lam):
            eng.set_factors(u, v)

        fresh()
        counted(eng, "plsa_lda_fit", lambda: eng.lda_fit(ALPHA, ETA, n_iter=2, n_iter_per_test=1, tolerance=0.0, doc_iter=2,
                                                         e_step_thresh=THRESH))
        fresh()
        counted(eng, "plsa_lda_refit", lambda: eng.lda_refit(ALPHA, n_iter=2, n_iter_per_test=1, tolerance=0.0, doc_iter=2,
                                                             e_step_thresh=THRESH))
        fresh()
        counted(eng, "plsa_lda_prior_fit", lambda: eng.lda_prior_fit(vec, ETA, learn=3, prior_start=2, prior_every=1, n_iter=2,
                                                                     n_iter_per_test=1, tolerance=0.0, doc_iter=2,
                                                                     e_step_thresh=THRESH))
        fresh()
        counted(eng, "plsa_lda_bound", lambda: eng.lda_bound(ALPHA))
        counted(eng, "plsa_lda_bound topics", lambda: eng.lda_bound(ALPHA, ETA))
        counted(eng, "plsa_lda_prior_bound", lambda: eng.lda_prior_bound(vec))
        counted(eng, "plsa_lda_prior_bound topics", lambda: eng.lda_prior_bound(vec, ETA))

        with amd.LdaOnlineState(home, M, k) as state:
            counted(home, "plsa_lda_online_set_lambda", lambda: state.set_lambda(lam))
            fresh()
            counted(eng, "plsa_lda_online_step", lambda: state.step(eng, ALPHA, ETA, 0.5, 2.0, doc_iter=2, e_step_thresh=THRESH))
            fresh()
            counted(eng, "plsa_lda_online_step bound", lambda: state.step(eng, ALPHA, ETA, 0.5, 2.0, doc_iter=2,
                                                                          e_step_thresh=THRESH, want_bound=True))
            fresh()
            counted(eng, "plsa_lda_online_fold", lambda: state.fold(eng, ALPHA, 2, e_step_thresh=THRESH))
            assert state.steps == 2

        with amd.OnlineState(home, M, k) as state:
            state.set_topics(topics)
            fresh(docs, topics)
            counted(eng, "plsa_online_step", lambda: state.step(eng, 0.5, 1.0 / float(X.sum()), inner_iter=2,
                                                                e_step_thresh=THRESH))
            fresh(docs, topics)
            counted(eng, "plsa_online_step ll", lambda: state.step(eng, 0.5, 1.0 / float(X.sum()), inner_iter=2,
                                                                   e_step_thresh=THRESH, want_ll=True))
            fresh(docs, topics)
            counted(eng, "plsa_online_fold", lambda: state.fold(eng, 2, e_step_thresh=THRESH))
            assert state.steps == 2
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_every_entry_point_launches_what_it_launched_before_the_fold(k):
    import enstop_amd
    with open(LEDGER) as f:
        golden = json.load(f)["k=%d" % k]
    got = readings(enstop_amd, k)
    assert sorted(got) == sorted(golden)
    for call in golden:
        assert got[call] == golden[call], (call, got[call], golden[call])
    # the ledger is not vacuous: the calls that must differ do
    assert got["plsa_lda_fit"]["k_lda_topics"] == 2 and "k_lda_topics" not in got["plsa_lda_refit"]
    assert "k_lda_topics" not in got["plsa_lda_online_step"] and got["plsa_lda_online_step"]["k_lda_online_blend"] == 1
    assert "k_lda_bound_v" in got["plsa_lda_prior_bound"] and "k_lda_bound_v" not in got["plsa_lda_bound"]
