"""The call around the loop of the five fit entry points (enstop_amd/csrc/plsa_drivers.hpp: fit_open, fit_run): which refusal
wins when two reasons hold at once, and what a refused call leaves behind.

plsa_fit, plsa_refit, plsa_fit_tempered, plsa_fit_smoothed and plsa_refit_smoothed refuse in this order: the variant's own
eligibility (its parameter, flags without PLSA_FUSED, a flag without a form, a context in reference arithmetic), the
delegation at the neutral parameter, the device, the factors, the counts; then fit_info is reset; then plsa_fit alone refuses
PLSA_SHARDED in the reference arithmetic.  Every text and every state below was read off the entry points as they stood
before they shared a frame, and the file passes against that library as well.

A 33 x 17 corpus of about 150 entries, k = 3; apart from one three-iteration fit per module nothing is launched.
"""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

FUSED, SHARDED, GRAPH, SUMS, LL = 1, 64, 128, 256, 512             # include/plsa_hip.h
N, M, K = 33, 17, 3
NO_FACTORS = "factors not set (call plsa_set_factors)"
FORMLESS = "%s: PLSA_SHARDED, PLSA_GRAPH, PLSA_REFERENCE_SUMS and PLSA_REFERENCE_LL have no %s form (flags=%d)"
NOT_FUSED = "%s: %s EM runs the fused passes only (flags without PLSA_FUSED)"
REFERENCE = "%s: the context is in reference arithmetic (plsa_set_arithmetic), which has no %s form"
COUNTS = "%s: bad n_iter / n_iter_per_test"
SHARDED_REFERENCE = ("plsa_fit: PLSA_REFERENCE_SUMS / PLSA_REFERENCE_LL have no doc-sharded form (the reference's sums are "
                     "single chains over all non-zeros)")
# entry point -> (Engine method, eligible parameters, neutral parameters, whom the neutral call delegates to, the form's word,
#                 an ineligible parameter, its refusal)
VARIANTS = {
    "plsa_fit_tempered": ("fit_tempered", dict(beta=0.5), dict(beta=1.0), "plsa_fit", "tempered", dict(beta=1.5),
                          "plsa_fit_tempered: beta=1.5 outside (0, 1]"),
    "plsa_fit_smoothed": ("fit_smoothed", dict(doc_topic_smoothing=0.1, topic_word_smoothing=0.01),
                          dict(doc_topic_smoothing=0.0, topic_word_smoothing=0.0), "plsa_fit", "smoothed",
                          dict(doc_topic_smoothing=0.1, topic_word_smoothing=-1.0),
                          "plsa_fit_smoothed: pseudo-count b=-1 is not a finite number >= 0"),
    "plsa_refit_smoothed": ("refit_smoothed", dict(doc_topic_smoothing=0.1), dict(doc_topic_smoothing=0.0), "plsa_refit",
                            "smoothed", dict(doc_topic_smoothing=-1.0),
                            "plsa_refit_smoothed: pseudo-count a=-1 is not a finite number >= 0"),
}
PLAIN = {"plsa_fit": "fit", "plsa_refit": "refit"}
GOOD = dict(n_iter=3, n_iter_per_test=2, tolerance=0.0, flags=FUSED)


def corpus():
    rs = np.random.RandomState(7)
    cells = rs.choice(N * M, 150, replace=False)
    X = sp.csr_matrix((rs.randint(1, 6, 150).astype(np.float32), (cells // M, cells % M)), shape=(N, M))
    U = rs.rand(N, K).astype(np.float32) + 0.1
    V = rs.rand(K, M).astype(np.float32) + 0.1
    return X, U / U.sum(1, keepdims=True), V / V.sum(1, keepdims=True)


@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


@pytest.fixture(scope="module")
def bare(amd):
    """a context with a corpus and no factors"""
    eng = amd.Engine()
    eng.upload_csr(corpus()[0])
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def fitted(amd):
    """a context after a fused fit, with what that fit left: (engine, fit_info, U, V)"""
    X, U, V = corpus()
    eng = amd.Engine()
    eng.upload_csr(X)
    eng.set_factors(U, V)
    eng.fit(**GOOD)
    info = eng.fit_info()
    assert info["fused"]
    yield (eng, info) + tuple(eng.get_factors())
    eng.close()


def refused(amd, eng, method, text, **kw):
    with pytest.raises(amd.engine.DeviceError) as e:
        getattr(eng, method)(**dict(GOOD, **kw))
    assert str(e.value) == text, (method, kw)


def unchanged(fitted):
    eng, info, U, V = fitted
    assert eng.fit_info() == info
    U1, V1 = eng.get_factors()
    assert np.array_equal(U1.view(np.uint32), U.view(np.uint32)) and np.array_equal(V1.view(np.uint32), V.view(np.uint32))


@pytest.mark.parametrize("entry", sorted(PLAIN))
def test_plain_entry_points_refuse_factors_before_counts(amd, bare, fitted, entry):
    refused(amd, bare, PLAIN[entry], NO_FACTORS, n_iter=-1)
    refused(amd, bare, PLAIN[entry], NO_FACTORS, n_iter_per_test=0, flags=FUSED | SHARDED | SUMS)
    refused(amd, fitted[0], PLAIN[entry], COUNTS % entry, n_iter=-1)
    refused(amd, fitted[0], PLAIN[entry], COUNTS % entry, n_iter_per_test=0)
    unchanged(fitted)


def test_fit_refuses_counts_before_sharded_reference(amd, fitted):
    for flags in (SHARDED | SUMS, FUSED | SHARDED | LL):
        refused(amd, fitted[0], "fit", COUNTS % "plsa_fit", n_iter_per_test=0, flags=flags)
        unchanged(fitted)


@pytest.mark.parametrize("entry", sorted(VARIANTS))
def test_variants_refuse_eligibility_first_in_its_own_order(amd, bare, fitted, entry):
    method, ok, neutral, _, word, bad, bad_text = VARIANTS[entry]
    for eng in (bare, fitted[0]):                                   # eligibility looks at neither factors nor counts
        refused(amd, eng, method, bad_text, flags=0, n_iter=-1, **bad)
        refused(amd, eng, method, bad_text, flags=GRAPH, **bad)
        refused(amd, eng, method, NOT_FUSED % (entry, word), flags=GRAPH | SUMS, n_iter=-1, **ok)
        refused(amd, eng, method, NOT_FUSED % (entry, word), flags=0, **neutral)
        for formless in (SHARDED, GRAPH, SUMS, LL, SHARDED | SUMS):
            refused(amd, eng, method, FORMLESS % (entry, word, FUSED | formless), flags=FUSED | formless, n_iter_per_test=0, **ok)
        refused(amd, eng, method, FORMLESS % (entry, word, FUSED | GRAPH), flags=FUSED | GRAPH, **neutral)
    unchanged(fitted)


@pytest.mark.parametrize("entry", sorted(VARIANTS))
def test_variants_refuse_the_reference_context_after_the_flags(amd, bare, entry):
    method, ok, neutral, _, word, bad, bad_text = VARIANTS[entry]
    bare.set_arithmetic("reference")
    try:
        refused(amd, bare, method, bad_text, **bad)
        refused(amd, bare, method, NOT_FUSED % (entry, word), flags=0, **ok)
        refused(amd, bare, method, FORMLESS % (entry, word, FUSED | SHARDED), flags=FUSED | SHARDED, **ok)
        refused(amd, bare, method, REFERENCE % (entry, word), n_iter=-1, **ok)
        refused(amd, bare, method, REFERENCE % (entry, word), **neutral)
    finally:
        bare.set_arithmetic(None)


@pytest.mark.parametrize("entry", sorted(VARIANTS))
def test_variants_then_refuse_factors_then_counts_under_the_name_that_runs(amd, bare, fitted, entry):
    method, ok, neutral, delegate, _, _, _ = VARIANTS[entry]
    refused(amd, bare, method, NO_FACTORS, n_iter=-1, **ok)
    refused(amd, bare, method, NO_FACTORS, n_iter_per_test=0, **neutral)
    refused(amd, fitted[0], method, COUNTS % entry, n_iter=-1, **ok)
    refused(amd, fitted[0], method, COUNTS % entry, n_iter_per_test=0, **ok)
    refused(amd, fitted[0], method, COUNTS % delegate, n_iter=-1, **neutral)      # the neutral parameter IS the plain entry point
    unchanged(fitted)


def test_the_refusal_of_fit_that_follows_the_reset(amd):
    """PLSA_SHARDED in the reference arithmetic is refused after fit_info was reset: the record of the earlier fit is gone,
    the factors stay, and the arithmetic the flags asked for ends with the call (the next fused fit runs fused)"""
    X, U, V = corpus()
    eng = amd.Engine()
    try:
        eng.upload_csr(X)
        eng.set_factors(U, V)
        eng.fit(**GOOD)
        before = eng.fit_info()
        U1, V1 = eng.get_factors()
        assert before["fused"] and before["col_tail"] is not None
        blank = dict(fused=False, pipelined=False, speculated=False, graph_launches=0, col_tail=None, two_stage_norm=False,
                     xcd_split=False)
        for flags in (FUSED | SHARDED | SUMS, SHARDED | LL):
            refused(amd, eng, "fit", SHARDED_REFERENCE, flags=flags)
            assert eng.fit_info() == blank
            U2, V2 = eng.get_factors()
            assert np.array_equal(U2.view(np.uint32), U1.view(np.uint32)) and np.array_equal(V2.view(np.uint32), V1.view(np.uint32))
        eng.set_factors(U, V)
        eng.fit(**GOOD)
        assert eng.fit_info() == before
        U3, V3 = eng.get_factors()
        assert np.array_equal(U3.view(np.uint32), U1.view(np.uint32)) and np.array_equal(V3.view(np.uint32), V1.view(np.uint32))
    finally:
        eng.close()
