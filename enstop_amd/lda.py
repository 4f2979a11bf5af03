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


def resolve_doc_topic_prior(value, k):
    """(alpha, learn): alpha a float (None or a number: the scalar forms) or a float64 vector [k]; learn whether alpha is
    re-estimated during the fit.  "auto": learned, from 1 / k; "asymmetric": the fixed vector 1 / (z + sqrt(k)), z = 1 .. k,
    normalised to sum 1 (gensim's); an array-like of k finite numbers > 0: that vector.  Anything else is a ValueError."""
    if isinstance(value, str):
        if value == "auto":
            return np.full(k, 1.0 / k), True
        if value == "asymmetric":
            alpha = 1.0 / (np.arange(1, k + 1, dtype=np.float64) + np.sqrt(k))
            return alpha / alpha.sum(), False
        raise ValueError("doc_topic_prior=%r: expected None, a number > 0, \"auto\", \"asymmetric\" or %d numbers > 0" % (value, k))
    if value is None or isinstance(value, (bool, numbers.Real)) or np.ndim(value) == 0:
        return resolve_prior("doc_topic_prior", value, k), False
    try:
        alpha = np.array(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("doc_topic_prior=%r: expected None, a number > 0, \"auto\", \"asymmetric\" or %d numbers > 0"
                         % (value, k)) from None
    if alpha.shape != (k,) or not np.isfinite(alpha).all() or not (alpha > 0).all():
        raise ValueError("doc_topic_prior: expected %d finite numbers > 0, got %r" % (k, value))
    return alpha, False


def resolve_topic_word_prior(value, k):
    """(eta, learn): None or a number as resolve_prior has them; "auto": learned, from 1 / k"""
    if isinstance(value, str) and value == "auto":
        return 1.0 / k, True
    return resolve_prior("topic_word_prior", value, k), False


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
def _fit(X, gamma0, lam0, alpha, eta, learn, prior_start, prior_every, n_iter, n_iter_per_test, tolerance, doc_iter, e_step_thresh,
         device, return_info):
    eng = get_engine(device)
    eng.upload_csr(X)
    eng.set_factors(gamma0, lam0)
    k = gamma0.shape[1]
    if learn or np.ndim(alpha):
        iters, trace, alpha, eta = eng.lda_prior_fit(np.broadcast_to(alpha, (k,)), eta, learn, prior_start, prior_every, n_iter,
                                                     n_iter_per_test, tolerance, doc_iter, e_step_thresh, trace=return_info)
    else:               # two fixed scalars: the scalar entry point, as before
        iters, trace = eng.lda_fit(alpha, eta, n_iter, n_iter_per_test, tolerance, doc_iter, e_step_thresh, trace=return_info)
    gamma, lam = eng.get_factors()
    if return_info:
        return gamma, lam, dict(n_iter=iters, bound_trace=trace, doc_topic_prior_=np.array(np.broadcast_to(alpha, (k,)), np.float64),
                                topic_word_prior_=float(eta))
    return gamma, lam


def lda_fit(X, k, doc_topic_prior=None, topic_word_prior=None, init="random", n_iter=100, n_iter_per_test=10, tolerance=0.001,
            doc_iter=1, e_step_thresh=1e-32, random_state=None, device=None, return_info=False, prior_start=20, prior_every=1):
    """Batch variational Bayes LDA of the count matrix X [n, m] with k topics: returns (gamma [n, k], lambda [k, m]), with
    return_info also dict(n_iter, bound_trace).  Priors of None mean 1 / k.  The bound is evaluated before the first iteration
    and after every n_iter_per_test-th; the loop stops when its relative change falls below `tolerance` (0 never stops).
    doc_iter - 1 extra rounds per iteration update gamma alone.  doc_topic_prior may also be a vector of k numbers > 0,
    "asymmetric" (the fixed vector 1 / (z + sqrt(k)) normalised to sum 1) or "auto"; topic_word_prior may be "auto".  An "auto"
    prior starts at 1 / k and is re-estimated behind the iterations prior_start, prior_start + prior_every, ... by maximising
    the bound over it (alpha one number per topic, eta one number); a test of the bound cannot stop the loop before the first
    update.  prior_start is a burn-in: from a random start the maximising alpha runs away.  With return_info the dict also
    holds doc_topic_prior_ [k] and topic_word_prior_, the priors in force at the end.  Bad arguments are a ValueError raised
    before an engine is touched."""
    k, n_iter, n_iter_per_test, doc_iter = _resolve_loop(k, n_iter, n_iter_per_test, doc_iter, tolerance)
    alpha, learn_alpha = resolve_doc_topic_prior(doc_topic_prior, k)
    eta, learn_eta = resolve_topic_word_prior(topic_word_prior, k)
    prior_start, prior_every = _resolve_count("prior_start", prior_start, 1), _resolve_count("prior_every", prior_every, 1)
    X = _counts(X)
    gamma0, lam0 = lda_init(X, k, init, random_state)
    return _fit(X, gamma0, lam0, alpha, eta, int(learn_alpha) + 2 * int(learn_eta), prior_start, prior_every, n_iter,
                n_iter_per_test, float(tolerance), doc_iter, e_step_thresh, device, return_info)


@_locked
def _transform(X, gamma0, lam, alpha, eta, n_iter, n_iter_per_test, tolerance, doc_iter, e_step_thresh, device, return_info):
    eng = get_engine(device)
    eng.upload_csr(X)
    eng.set_factors(gamma0, lam)
    vector = np.ndim(alpha) > 0
    refit, bound_of = (eng.lda_prior_refit, eng.lda_prior_bound) if vector else (eng.lda_refit, eng.lda_bound)
    iters, trace = refit(alpha, n_iter, n_iter_per_test, tolerance, doc_iter, e_step_thresh, trace=return_info)
    gamma, _ = eng.get_factors(want_v=False)
    if return_info:
        bound = bound_of(alpha, eta)
        return gamma, dict(n_iter=iters, bound_trace=trace, bound=bound)
    return gamma


def lda_transform(X, lam, doc_topic_prior, n_iter=50, n_iter_per_test=10, tolerance=0.001, doc_iter=1, e_step_thresh=1e-32,
                  random_state=None, device=None, return_info=False, topic_word_prior=None):
    """The fold-in of X against the fixed lambda [k, m]: gamma [n, k], started at rng.gamma(100., 0.01, (n, k)); lambda stays as
    it is.  With return_info also dict(n_iter, bound_trace, bound): the trace holds the likelihood and document parts of the
    bound (float32), `bound` is the bound at the returned gamma in float64 -- with the topic part when topic_word_prior is
    given, which is scikit-learn's score.  doc_topic_prior: a number or a vector of k numbers > 0."""
    lam = np.asarray(lam)
    if lam.ndim != 2:
        raise ValueError("lam has shape %s, expected (k, m)" % (lam.shape,))
    k, n_iter, n_iter_per_test, doc_iter = _resolve_loop(lam.shape[0], n_iter, n_iter_per_test, doc_iter, tolerance)
    if isinstance(doc_topic_prior, str):
        raise ValueError("doc_topic_prior=%r: the fold-in takes a number or %d numbers > 0" % (doc_topic_prior, k))
    alpha, _ = resolve_doc_topic_prior(doc_topic_prior, k)
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
    doc_topic_prior: None (1 / k), a number, k numbers, "asymmetric" or "auto"; topic_word_prior: None, a number or "auto"
    (lda_fit).  `doc_topic_prior_` [k] and `topic_word_prior_` are the priors in force at the end of the fit, learned or not;
    transform, score and perplexity use them.  The class attributes prior_start and prior_every are lda_fit's.
    held_out_perplexity splits every document and scores the held-out part under pLSA's fold-in of `topic_word_`;
    coherence() and log_lift() score `topic_word_` against `training_data_`."""

    transform_random_seed = 42
    prior_start = 20
    prior_every = 1

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
        _resolve_count("prior_start", self.prior_start, 1)
        _resolve_count("prior_every", self.prior_every, 1)
        return resolve_doc_topic_prior(self.doc_topic_prior, k), resolve_topic_word_prior(self.topic_word_prior, k)

    def fit(self, X, y=None):
        self.fit_transform(X)
        return self

    def fit_transform(self, X, y=None):
        self._priors()
        X = _counts(X)
        gamma, lam, info = lda_fit(X, self.n_components, self.doc_topic_prior, self.topic_word_prior, n_iter=self.n_iter,
                                   n_iter_per_test=self.n_iter_per_test, tolerance=self.tolerance, doc_iter=self.doc_iter,
                                   random_state=self.random_state, return_info=True, prior_start=self.prior_start,
                                   prior_every=self.prior_every)
        self.doc_topic_prior_ = info["doc_topic_prior_"]
        self.topic_word_prior_ = info["topic_word_prior_"]
        self.components_ = lam
        self.topic_word_ = lam / lam.sum(axis=1, keepdims=True)
        self.embedding_ = gamma / gamma.sum(axis=1, keepdims=True)
        self.training_data_ = X
        self.n_iter_ = info["n_iter"]
        self.bound_trace_ = info["bound_trace"]
        self.bound_ = float(info["bound_trace"][-1])
        return self.embedding_

    def _fold_in(self, X, return_info=False):
        (alpha, learned), _ = self._priors()
        if learned or np.ndim(alpha):                     # a vector in force; two scalars fold in as they always did
            alpha = self.doc_topic_prior_
        return lda_transform(X, self.components_, alpha, doc_iter=self.doc_iter, random_state=self.transform_random_seed,
                             return_info=return_info, topic_word_prior=self.topic_word_prior_)

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
