"""Latent Dirichlet allocation by variational Bayes, on the device.

Smoothed pLSA (smoothed.py) is MAP estimation under Dirichlet priors and can only ADD pseudo-counts: concentrations >= 1.
The regime LDA exists for is sparse document mixtures, doc_topic_prior < 1 (scikit-learn's default is 1 / k), which needs the
variational treatment (Blei, Ng, Jordan 2003; the batch form of Hoffman, Blei, Bach 2010, which scikit-learn's
LatentDirichletAllocation follows).  The state is gamma [n, k] and lambda [k, m], the Dirichlet parameters of the document
mixtures and of the topics; with

    A_dz = exp(psi(gamma_dz) - psi(sum_z gamma_dz))        B_zw = exp(psi(lambda_zw) - psi(sum_w lambda_zw))

the optimal responsibilities are phi_dwz ~ A_dz B_zw, and an iteration is

    gamma_dz = alpha + sum_w x_dw phi_dwz                  lambda_zw = eta + sum_d x_dw phi_dwz

both from the same tables, which is exact coordinate ascent: the variational bound never decreases.  The two sums are what the
fused passes of plsa_fit compute from any pair of non-negative tables, so the passes run unchanged on the exp-digamma tables
and the priors are added behind them (include/plsa_hip_diag.h).  The fused default arithmetic on one GPU
only; no sample weights.

An entry at a prior below about 0.012 is below the float32 normal range (psi(0.01) = -100.6), so the passes run on scaled
tables: every document's row of A and every word's row of B is divided by its largest entry, which the responsibilities do
not see, and the bound gets the logarithms back.
"""
import numbers

import numpy as np
from scipy.sparse import csr_matrix, issparse
from sklearn.base import BaseEstimator, TransformerMixin
from sklearn.utils import check_array, check_random_state

from .engine import get_engine
from .plsa import _TopicMetricsMixin, _locked


def resolve_prior(name, value, k):
    """None -> 1 / k (scikit-learn's default); otherwise a finite real number > 0, or a ValueError"""
    if value is None:
        return 1.0 / k
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or not np.isfinite(value) or not value > 0:
        raise ValueError("%s=%r: expected None or a finite number > 0" % (name, value))
    return float(value)


def _resolve_count(name, value, least):
    if isinstance(value, bool) or not isinstance(value, numbers.Integral) or value < least:
        raise ValueError("%s=%r: expected an integer >= %d" % (name, value, least))
    return int(value)


def _resolve_loop(k, n_iter, n_iter_per_test, doc_iter, tolerance):
    k = _resolve_count("k", k, 1)
    if k > 1024:
        raise ValueError("k=%d: at most 1024 topics" % k)
    if isinstance(tolerance, bool) or not isinstance(tolerance, numbers.Real) or not tolerance >= 0:
        raise ValueError("tolerance=%r: expected a number >= 0" % (tolerance,))
    return (k, _resolve_count("n_iter", n_iter, 0), _resolve_count("n_iter_per_test", n_iter_per_test, 1),
            _resolve_count("doc_iter", doc_iter, 1))


def _counts(X):
    X = check_array(X, accept_sparse="csr")
    X = X.tocsr() if issparse(X) else csr_matrix(X)
    if np.any(X.data < 0):
        raise ValueError("LDA is only valid for matrices with non-negative entries")
    return X


def lda_init(X, k, init="random", rng=None):
    """(gamma0 [n, k], lambda0 [k, m]) float32.  "random": rng.gamma(100., 0.01, (k, m)) and then (n, k) from the RandomState,
    scikit-learn's draws; a (gamma0, lambda0) tuple is taken as given (positive, of the right shapes)."""
    n, m = X.shape
    if isinstance(init, str):
        if init != "random":
            raise ValueError("Unrecognized init %r: expected \"random\" or a (gamma0, lambda0) tuple" % (init,))
        rng = check_random_state(rng)
        lam = rng.gamma(100.0, 0.01, (k, m))
        gamma = rng.gamma(100.0, 0.01, (n, k))
    else:
        try:
            gamma, lam = init
        except (TypeError, ValueError):
            raise ValueError("init: expected \"random\" or a (gamma0, lambda0) tuple") from None
        gamma, lam = np.asarray(gamma), np.asarray(lam)
        if gamma.shape != (n, k) or lam.shape != (k, m):
            raise ValueError("init has shapes %s and %s, expected %s and %s" % (gamma.shape, lam.shape, (n, k), (k, m)))
    gamma, lam = np.ascontiguousarray(gamma, np.float32), np.ascontiguousarray(lam, np.float32)
    if not (np.isfinite(gamma).all() and np.isfinite(lam).all() and (gamma > 0).all() and (lam > 0).all()):
        raise ValueError("init: gamma0 and lambda0 must be finite and > 0")
    return gamma, lam


@_locked
def _fit(X, gamma0, lam0, alpha, eta, n_iter, n_iter_per_test, tolerance, doc_iter, e_step_thresh, device, return_info):
    eng = get_engine(device)
    eng.upload_csr(X)
    eng.set_factors(gamma0, lam0)
    iters, trace = eng.lda_fit(alpha, eta, n_iter, n_iter_per_test, tolerance, doc_iter, e_step_thresh, trace=return_info)
    gamma, lam = eng.get_factors()
    if return_info:
        return gamma, lam, dict(n_iter=iters, bound_trace=trace)
    return gamma, lam


def lda_fit(X, k, doc_topic_prior=None, topic_word_prior=None, init="random", n_iter=100, n_iter_per_test=10, tolerance=0.001,
            doc_iter=1, e_step_thresh=1e-32, random_state=None, device=None, return_info=False):
    """Batch variational Bayes LDA of the count matrix X [n, m] with k topics: returns (gamma [n, k], lambda [k, m]), with
    return_info also dict(n_iter, bound_trace).  Priors of None mean 1 / k.  The bound is evaluated before the first iteration
    and after every n_iter_per_test-th; the loop stops when its relative change falls below `tolerance` (0 never stops).
    doc_iter - 1 extra rounds per iteration update gamma alone.  Bad arguments are a ValueError raised before an engine is
    touched."""
    k, n_iter, n_iter_per_test, doc_iter = _resolve_loop(k, n_iter, n_iter_per_test, doc_iter, tolerance)
    alpha = resolve_prior("doc_topic_prior", doc_topic_prior, k)
    eta = resolve_prior("topic_word_prior", topic_word_prior, k)
    X = _counts(X)
    gamma0, lam0 = lda_init(X, k, init, random_state)
    return _fit(X, gamma0, lam0, alpha, eta, n_iter, n_iter_per_test, float(tolerance), doc_iter, e_step_thresh, device,
                return_info)


@_locked
def _transform(X, gamma0, lam, alpha, eta, n_iter, n_iter_per_test, tolerance, doc_iter, e_step_thresh, device, return_info):
    eng = get_engine(device)
    eng.upload_csr(X)
    eng.set_factors(gamma0, lam)
    iters, trace = eng.lda_refit(alpha, n_iter, n_iter_per_test, tolerance, doc_iter, e_step_thresh, trace=return_info)
    gamma, _ = eng.get_factors(want_v=False)
    if return_info:
        bound = eng.lda_bound(alpha, eta)
        return gamma, dict(n_iter=iters, bound_trace=trace, bound=bound)
    return gamma


def lda_transform(X, lam, doc_topic_prior, n_iter=50, n_iter_per_test=10, tolerance=0.001, doc_iter=1, e_step_thresh=1e-32,
                  random_state=None, device=None, return_info=False, topic_word_prior=None):
    """The fold-in of X against the fixed lambda [k, m]: gamma [n, k], started at rng.gamma(100., 0.01, (n, k)); lambda stays as
    it is.  With return_info also dict(n_iter, bound_trace, bound): the trace holds the likelihood and document parts of the
    bound (float32), `bound` is the bound at the returned gamma in float64 -- with the topic part when topic_word_prior is
    given, which is scikit-learn's score."""
    lam = np.asarray(lam)
    if lam.ndim != 2:
        raise ValueError("lam has shape %s, expected (k, m)" % (lam.shape,))
    k, n_iter, n_iter_per_test, doc_iter = _resolve_loop(lam.shape[0], n_iter, n_iter_per_test, doc_iter, tolerance)
    alpha = resolve_prior("doc_topic_prior", doc_topic_prior, k)
    eta = None if topic_word_prior is None else resolve_prior("topic_word_prior", topic_word_prior, k)
    X = _counts(X)
    if X.shape[1] != lam.shape[1]:
        raise ValueError("X has %d columns, lam %d" % (X.shape[1], lam.shape[1]))
    gamma0 = check_random_state(random_state).gamma(100.0, 0.01, (X.shape[0], k))
    gamma0, lam = lda_init(X, k, (gamma0, lam))
    return _transform(X, gamma0, lam, alpha, eta, n_iter, n_iter_per_test, float(tolerance), doc_iter, e_step_thresh, device,
                      return_info)


class LDA(_TopicMetricsMixin, BaseEstimator, TransformerMixin):
    """Latent Dirichlet allocation by batch variational Bayes.  `components_` is lambda [k, m], unnormalised, as scikit-learn
    has it; `topic_word_` its rows normalised; `embedding_` gamma with rows normalised; `bound_` the variational bound of the
    training matrix at the end of the fit, `bound_trace_` its trace, `n_iter_` the iterations run.  transform(X) is the
    normalised gamma of the fold-in (50 iterations at most, seeded by transform_random_seed = 42), score(X) the bound of X
    under its fold-in, perplexity(X) = exp(-score / tokens), scikit-learn's definition.
    held_out_perplexity splits every document and scores the held-out part under pLSA's fold-in of `topic_word_`;
    coherence() and log_lift() score `topic_word_` against `training_data_`."""

    transform_random_seed = 42

    def __init__(self, n_components=10, doc_topic_prior=None, topic_word_prior=None, n_iter=100, n_iter_per_test=10,
                 tolerance=0.001, doc_iter=1, random_state=None):
        self.n_components = n_components
        self.doc_topic_prior = doc_topic_prior
        self.topic_word_prior = topic_word_prior
        self.n_iter = n_iter
        self.n_iter_per_test = n_iter_per_test
        self.tolerance = tolerance
        self.doc_iter = doc_iter
        self.random_state = random_state

    def _metric_topics(self):
        """coherence() and log_lift() score `topic_word_`: `components_` is lambda, whose rows do not sum to 1"""
        return self.topic_word_

    def _priors(self):
        k = _resolve_count("n_components", self.n_components, 1)
        return (resolve_prior("doc_topic_prior", self.doc_topic_prior, k),
                resolve_prior("topic_word_prior", self.topic_word_prior, k))

    def fit(self, X, y=None):
        self.fit_transform(X)
        return self

    def fit_transform(self, X, y=None):
        self._priors()
        X = _counts(X)
        gamma, lam, info = lda_fit(X, self.n_components, self.doc_topic_prior, self.topic_word_prior, n_iter=self.n_iter,
                                   n_iter_per_test=self.n_iter_per_test, tolerance=self.tolerance, doc_iter=self.doc_iter,
                                   random_state=self.random_state, return_info=True)
        self.components_ = lam
        self.topic_word_ = lam / lam.sum(axis=1, keepdims=True)
        self.embedding_ = gamma / gamma.sum(axis=1, keepdims=True)
        self.training_data_ = X
        self.n_iter_ = info["n_iter"]
        self.bound_trace_ = info["bound_trace"]
        self.bound_ = float(info["bound_trace"][-1])
        return self.embedding_

    def _fold_in(self, X, return_info=False):
        alpha, eta = self._priors()
        return lda_transform(X, self.components_, alpha, doc_iter=self.doc_iter, random_state=self.transform_random_seed,
                             return_info=return_info, topic_word_prior=eta)

    def transform(self, X, y=None):
        gamma = self._fold_in(X)
        return gamma / gamma.sum(axis=1, keepdims=True)

    def score(self, X, y=None):
        """the variational bound of X under its fold-in against `components_` (all three parts: scikit-learn's score)"""
        return self._fold_in(X, return_info=True)[1]["bound"]

    def perplexity(self, X):
        """exp(-score(X) / tokens of X)"""
        X = _counts(X)
        return float(np.exp(-self.score(X) / X.sum()))

    def held_out_perplexity(self, X, fraction=0.5, on_zero="inf"):
        """document completion under the normalised topics: scoring.held_out_scores(X, topic_word_, method="completion")"""
        from .scoring import held_out_scores
        return held_out_scores(_counts(X), self.topic_word_, method="completion", fraction=fraction,
                               random_state=self.transform_random_seed, on_zero=on_zero)["perplexity"]
