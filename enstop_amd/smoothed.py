"""Smoothed pLSA: MAP EM with Dirichlet pseudo-counts, on the device.

Maximum-likelihood pLSA gives a word that a topic never saw P(w|z) = 0 exactly, and exact zeros are absorbing under EM: a
held-out document with one word the training set did not contain has no probability at all (scoring: `unscored`).  The
standard remedy is MAP estimation under Dirichlet priors (scikit-learn's LDA: doc_topic_prior / topic_word_prior, gensim:
alpha / eta): a pseudo-count is added to every expected count before it is normalised,

    P(z|d) = (n_dz + a) / (N_d + k a)        P(w|z) = (n_wz + b) / (N_z + m b)

with a = doc_topic_smoothing >= 0 and b = topic_word_smoothing >= 0, the Dirichlet concentrations minus one.  This is EM on
the log posterior

    F = sum sw_d x_dw log sum_z P(w|z) P(z|d)  +  a sum_d sw_d sum_z log P(z|d)  +  b sum_z sum_w log P(w|z)

which never decreases; F stands in the trace and in the stop test where plsa_fit has the log-likelihood.  A pseudo-count of 0
leaves its side the ordinary update, bit for bit; both 0 is plsa_fit.  The fused default arithmetic on one GPU only
(include/plsa_hip_diag.h: plsa_fit_smoothed, plsa_refit_smoothed, plsa_log_posterior).
"""
from scipy.sparse import csr_matrix, issparse
from sklearn.utils import check_random_state

from ._driver import effective_weights, init_factors, resolve_smoothing, smoothed_flags
from .engine import get_engine
from .plsa import _locked, _refit_on_engine


@_locked
def _fit(X, k, sample_weight, a, b, init, n_iter, n_iter_per_test, tolerance, e_step_thresh, random_state, device, flags,
         return_info):
    eng = get_engine(device)
    eng.upload_csr(X)
    init_factors(eng, k, init, check_random_state(random_state), X)
    iters, trace = eng.fit_smoothed(a, b, effective_weights(sample_weight), n_iter, n_iter_per_test, tolerance, e_step_thresh,
                                    flags, trace=return_info)
    U, V = eng.get_factors()
    if return_info:
        return U, V, dict(n_iter=iters, log_posterior_trace=trace)
    return U, V


def plsa_fit_smoothed(X, k, sample_weight=None, doc_topic_smoothing=0.0, topic_word_smoothing=0.0, init="random", n_iter=100,
                      n_iter_per_test=10, tolerance=0.001, e_step_thresh=1e-32, random_state=None, device=None, flags=None,
                      return_info=False):
    """plsa_fit with the pseudo-counts doc_topic_smoothing and topic_word_smoothing; returns (P(z|d) [n, k], P(w|z) [k, m]),
    with return_info also dict(n_iter, log_posterior_trace).  The factors are initialised exactly as plsa_fit initialises
    them.  A pseudo-count that is not a finite number >= 0, flags without PLSA_FUSED and the reference arithmetic are a
    ValueError raised before an engine is touched."""
    a = resolve_smoothing("doc_topic_smoothing", doc_topic_smoothing)
    b = resolve_smoothing("topic_word_smoothing", topic_word_smoothing)
    flags = smoothed_flags(flags)
    X = X.tocsr() if issparse(X) else csr_matrix(X)
    return _fit(X, k, sample_weight, a, b, init, n_iter, n_iter_per_test, tolerance, e_step_thresh, random_state, device, flags,
                return_info)


@_locked
def _refit(X, topics, sample_weight, a, n_iter, n_iter_per_test, tolerance, e_step_thresh, random_state, device, flags,
           return_info):
    eng = get_engine(device)
    iters, trace = _refit_on_engine(eng, X, topics, sample_weight, n_iter, n_iter_per_test, tolerance, e_step_thresh,
                                    check_random_state(random_state), flags, trace=return_info, doc_topic_smoothing=a)
    U, _ = eng.get_factors(want_v=False)
    if return_info:
        return U, dict(n_iter=iters, log_posterior_trace=trace)
    return U


def plsa_refit_smoothed(X, topics, sample_weight=None, doc_topic_smoothing=0.0, n_iter=50, n_iter_per_test=10, tolerance=0.005,
                        e_step_thresh=1e-32, random_state=None, device=None, flags=None, return_info=False):
    """plsa_refit with the document-side pseudo-count: P(z|d) [n, k] for X against the fixed `topics`, which stay as they
    are; a document without tokens gets 1 / k.  0 is plsa_refit.  Refusals as in plsa_fit_smoothed."""
    a = resolve_smoothing("doc_topic_smoothing", doc_topic_smoothing)
    flags = smoothed_flags(flags)
    X = X.tocsr() if issparse(X) else csr_matrix(X)
    return _refit(X, topics, sample_weight, a, n_iter, n_iter_per_test, tolerance, e_step_thresh, random_state, device, flags,
                  return_info)
