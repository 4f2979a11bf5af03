"""Online variational Bayes LDA on the device (Hoffman, Blei, Bach 2010, algorithm 2 -- what scikit-learn's
LatentDirichletAllocation(learning_method="online") and gensim's LdaModel run, and the only form of LDA that takes documents in
pieces).

Batch LDA (lda.py) updates lambda once per pass over the corpus, from tables that are one whole pass old.  The online form cuts
the documents into blocks and updates lambda after every block, with a decaying step size:

    one step on block b of n_b documents, step counter t (enstop_amd/include/plsa_hip_lda_online.h):
      1. doc_iter - 1 gamma-only rounds and one full round over the block under the tables B of the current lambda:
         gamma_b = alpha + the block's expected counts per document;  n_wz = the block's expected counts per word
      2. lambda <- (1 - rho_t) lambda + rho_t (eta + scale_b n_wz),   B and its sums re-formed from the new lambda
    rho_t = (tau0 + t)^(-kappa) for t = 0, 1, ... (a fixed `rho` overrides it);  scale_b = D / n_b, D the number of documents of
    the corpus (lda_fit_online) or the promised `total_samples` (partial_fit).  At rho = 1 and scale = 1 a step is one
    iteration of lda_fit on the block, to the bit.

  LdaOnlineState    the device-side state (lambda, its tables, t) behind the C ABI (online.DeviceState's frame); steps and folds
                    are driven through it
  lda_fit_online    cuts X into blocks of whole documents, one context each (online.cut_blocks), and drives
                    online.OnlineSchedule through online.drive_blocks
  OnlineLDA         the estimator: fit / fit_transform through lda_fit_online, and partial_fit for documents in pieces

alpha and eta are fixed scalars here; vectors, "asymmetric" and "auto" (lda.py) have no online form yet, nor have sample weights.

Every default below (n_batches, n_epochs, doc_iter, kappa, tau0) is this package's choice from a float64 NumPy model of the
algorithm on a planted corpus (tests/lda_online_model.py); none of them was tuned on a device.  doc_iter
is 3, not the batch fit's 1: a block meets tables that have moved 63 times since it last saw them, and one round from its stale
gamma does not catch up (the model: five epochs at doc_iter = 1 end above batch LDA's perplexity, two at doc_iter = 3 below it).
"""
import ctypes as C
import numbers

import numpy as np
from sklearn.utils import check_random_state

from . import _lib
from ._driver import resolve_flags
from ._lib import ptr
from .engine import Engine, get_engine
from .lda import LDA, _counts, _resolve_count, lda_init, resolve_prior
from .online import (_ABI_FLAGS, MAX_BATCHES, DeviceState, OnlineSchedule, PartialFitMixin, block_tokens, cut_blocks, drive_blocks,
                     plain_fused_flags)
from .plsa import _locked


class LdaOnlineState(DeviceState):
    """lambda, the tables formed from it and the step counter on the device of `home` (an Engine, which must outlive the
    state: the host copies of lambda go through its stream).  One ABI call per method."""
    _prefix = "plsa_lda_online"
    _counter = "plsa_lda_online_get_lambda"

    def set_lambda(self, lam):
        """lambda := lam [k, m], the tables formed from it, t := 0"""
        self.home._ok(self._L.plsa_lda_online_set_lambda(self._h, self._table(lam)))
        return self

    def get_lambda(self):
        lam = np.empty((self.k, self.m), np.float32)
        self.home._ok(self._L.plsa_lda_online_get_lambda(self._h, ptr(lam), None))
        return lam

    def step(self, eng, doc_topic_prior, topic_word_prior, rho, scale, doc_iter=3, e_step_thresh=1e-32, want_bound=False,
             flags=None):
        """One step on the block resident on `eng` (module docstring); -> with want_bound the block's bound without the topic
        part, at the gamma the step leaves and the lambda it started from, else None.  Without want_bound nothing waits."""
        bound = C.c_double(0.0)
        eng._ok(self._L.plsa_lda_online_step(self._h, eng._h, float(doc_topic_prior), float(topic_word_prior), int(doc_iter),
                                             np.float32(e_step_thresh), float(rho), float(scale), resolve_flags(flags) & _ABI_FLAGS,
                                             C.byref(bound) if want_bound else None))
        return bound.value if want_bound else None

    def fold(self, eng, doc_topic_prior, n_rounds, e_step_thresh=1e-32, flags=None):
        """n_rounds gamma-only rounds over the block resident on `eng` under the state's tables, nothing else"""
        eng._ok(self._L.plsa_lda_online_fold(self._h, eng._h, float(doc_topic_prior), int(n_rounds), np.float32(e_step_thresh),
                                             resolve_flags(flags) & _ABI_FLAGS))


def resolve_online_prior(name, value, k):
    """None -> 1 / k; a finite real number > 0; everything lda_fit takes beyond that (a vector, "asymmetric", "auto") is a
    ValueError: the online fit has fixed scalar priors"""
    if isinstance(value, str) or (value is not None and np.ndim(value) > 0):
        raise ValueError("%s=%r: the online fit takes None or one finite number > 0 (vectors, \"asymmetric\" and \"auto\" have no "
                         "online form yet)" % (name, value))
    return resolve_prior(name, value, k)


def _resolve_online(k, doc_topic_prior, topic_word_prior, n_batches, n_epochs, doc_iter, tolerance):
    k = _resolve_count("k", k, 1)
    if k > 1024:
        raise ValueError("k=%d: at most 1024 topics" % k)
    alpha = resolve_online_prior("doc_topic_prior", doc_topic_prior, k)
    eta = resolve_online_prior("topic_word_prior", topic_word_prior, k)
    n_batches = _resolve_count("n_batches", n_batches, 1)
    if n_batches > MAX_BATCHES:
        raise ValueError("n_batches must be in [1, %d], not %r" % (MAX_BATCHES, n_batches))
    if isinstance(tolerance, bool) or not isinstance(tolerance, numbers.Real) or not tolerance >= 0:
        raise ValueError("tolerance=%r: expected a number >= 0" % (tolerance,))
    return k, alpha, eta, n_batches, _resolve_count("n_epochs", n_epochs, 0), _resolve_count("doc_iter", doc_iter, 1)


@_locked
def _drive_locked(device, pieces):
    """drive_blocks under the lock of the device's engine, with the home engine handed to the pieces"""
    return drive_blocks(**pieces(get_engine(device)))


def lda_fit_online(X, k, doc_topic_prior=None, topic_word_prior=None, init="random", n_batches=64, n_epochs=5, doc_iter=3,
                   kappa=0.7, tau0=10.0, rho=None, tolerance=0.001, shuffle_documents=True, e_step_thresh=1e-32,
                   random_state=None, device=None, return_info=False, callback=None):
    """LDA with k topics by online variational Bayes; -> (gamma [n, k], lambda [k, m]) as float32, with return_info an `info`
    dict too.  Priors: None (1 / k) or a finite number > 0.

    1. The start is lda_fit's for the same seed (lda_init): lambda0, then gamma0, drawn from `random_state` first; rows of
       gamma stay with their documents.
    2. shuffle_documents: ONE permutation of the documents, drawn from `random_state` after the factors.  The (permuted)
       documents are cut into min(n_batches, n) blocks of whole documents with about equal non-zeros (row_ranges_by_nnz);
       every block gets a context of its own on the device: its rows, its gamma, and three [m, kp] tables (n_batches is
       capped at 256; the bytes are in info["bytes_per_block_context"]).
    3. Epochs of one step per block, in block order, with scale = n / n_b (online.OnlineSchedule: rho_t, the cap n_epochs,
       the stop on the relative change of L_e).  L_e is the sum over the blocks of epoch e of the block's bound without the
       topic part, taken at the gamma its step left and the lambda its step started from: a progressive bound.
    4. After the last epoch every block runs max(doc_iter, 1) gamma-only rounds under the final tables; those rows are the
       returned gamma, in the caller's order.

    The bounds are read (one host wait per step) only when the tolerance is positive or return_info is set.
    info: `n_epochs`, `n_steps`, `rho` (one per step), `bounds` (L_e per epoch), `block_ranges` (row ranges of the permuted
    documents), `permutation` (None without shuffling), `tokens` (per block), `bytes_per_block_context`.
    callback(info_so_far, state) is called after every epoch.  Bad arguments are a ValueError raised before an engine is
    touched.  Default arithmetic, fused schedule only; no sample weights."""
    k, alpha, eta, n_batches, n_epochs, doc_iter = _resolve_online(k, doc_topic_prior, topic_word_prior, n_batches, n_epochs,
                                                                   doc_iter, tolerance)
    flags = plain_fused_flags("online LDA")
    X = _counts(X)
    n, m = X.shape
    n_blocks = min(n_batches, n)
    if n_blocks < 1:
        raise ValueError("lda_fit_online: no documents")
    schedule = OnlineSchedule(n_blocks, n_epochs, kappa, tau0, rho, tolerance)
    rng = check_random_state(random_state)
    gamma0, lam0 = lda_init(X, k, init, rng)
    X, (gamma0,), perm, ranges, undo = cut_blocks("lda_fit_online", X, n_blocks, rng, shuffle_documents, gamma0)

    def setup(eng, i, a, b):
        eng.upload_csr(X[a:b])
        eng.set_factors(gamma0[a:b], lam0)
        return block_tokens(X[a:b]), float(n) / float(b - a)

    def pieces(home):
        return dict(
            n=n, k=k, ranges=ranges, perm=perm, schedule=schedule, want=bool(return_info) or schedule.tolerance > 0.0,
            series="bounds", new_engine=lambda: Engine(home.device), setup=setup,
            make_state=lambda: LdaOnlineState(home, m, k).set_lambda(lam0),
            step=lambda state, eng, rho_t, scale, want: state.step(eng, alpha, eta, rho_t, scale, doc_iter, e_step_thresh, want, flags),
            fold=lambda state, eng: state.fold(eng, alpha, max(doc_iter, 1), e_step_thresh, flags),
            rows=lambda eng: eng.get_factors(want_v=False)[0], topics=lambda state: state.get_lambda(), callback=callback)

    gamma, lam, info = _drive_locked(device, pieces)
    return (undo(gamma), lam, info) if return_info else (undo(gamma), lam)


class OnlineLDA(PartialFitMixin, LDA):
    """LDA fitted by online variational Bayes (lda_fit_online; module docstring): `components_`, `topic_word_`, `embedding_`,
    `training_data_`, `doc_topic_prior_`, `topic_word_prior_` as LDA's, `n_iter_` = epochs run, `n_steps_` = steps taken,
    `online_info_` = lda_fit_online's info, `bound_trace_` = L_e per epoch (progressive, without the topic part) and `bound_`
    its last value.  transform, score, perplexity, held_out_perplexity and the topic metrics are LDA's.  n_iter and
    n_iter_per_test are LDA's parameters and do not enter the online fit.

    partial_fit(X) takes one step on the documents X and may be called any number of times: the first call fixes the
    vocabulary size and draws lambda0 as lda_init draws it (rng.gamma(100., 0.01, (k, m))) from `random_state`; every call
    uploads X to one scratch engine of the estimator's own, draws that batch's gamma0 from the same stream
    (rng.gamma(100., 0.01, (n, k))), takes the step with rho of the step counter and scale = total_samples / n, and updates
    `components_`, `topic_word_`, `n_steps_` and `embedding_` (that batch's gamma, rows normalised).  n_batches, n_epochs,
    tolerance and shuffle_documents do not enter it.

    Priors: None (1 / k) or a finite number > 0.  The defaults are this package's choices from a float64 model of the
    algorithm, not tuned on a device."""

    def __init__(self, n_components=10, doc_topic_prior=None, topic_word_prior=None, n_iter=100, n_iter_per_test=10,
                 tolerance=0.001, doc_iter=3, random_state=None, n_batches=64, n_epochs=5, kappa=0.7, tau0=10.0, rho=None,
                 shuffle_documents=True, total_samples=1e6):
        super().__init__(n_components=n_components, doc_topic_prior=doc_topic_prior, topic_word_prior=topic_word_prior,
                         n_iter=n_iter, n_iter_per_test=n_iter_per_test, tolerance=tolerance, doc_iter=doc_iter,
                         random_state=random_state)
        self.n_batches = n_batches
        self.n_epochs = n_epochs
        self.kappa = kappa
        self.tau0 = tau0
        self.rho = rho
        self.shuffle_documents = shuffle_documents
        self.total_samples = total_samples

    def _priors(self):
        """LDA's shape, ((alpha, learned), (eta, learned)), with the scalars the online fit takes"""
        k = _resolve_count("n_components", self.n_components, 1)
        return ((resolve_online_prior("doc_topic_prior", self.doc_topic_prior, k), False),
                (resolve_online_prior("topic_word_prior", self.topic_word_prior, k), False))

    def _set_topics(self, lam, alpha, eta):
        k = lam.shape[0]
        self.doc_topic_prior_ = np.full(k, alpha, np.float64)
        self.topic_word_prior_ = float(eta)
        self.components_ = lam
        self.topic_word_ = lam / lam.sum(axis=1, keepdims=True)

    def fit_transform(self, X, y=None):
        (alpha, _), (eta, _) = self._priors()
        self._end_partial()
        X = _counts(X)
        gamma, lam, info = lda_fit_online(X, self.n_components, self.doc_topic_prior, self.topic_word_prior, n_batches=self.n_batches,
                                          n_epochs=self.n_epochs, doc_iter=self.doc_iter, kappa=self.kappa, tau0=self.tau0,
                                          rho=self.rho, tolerance=self.tolerance, shuffle_documents=self.shuffle_documents,
                                          random_state=self.random_state, return_info=True)
        self._set_topics(lam, alpha, eta)
        self.embedding_ = gamma / gamma.sum(axis=1, keepdims=True)
        self.training_data_ = X
        self.n_iter_ = info["n_epochs"]
        self.n_steps_ = info["n_steps"]
        self.online_info_ = info
        self.bound_trace_ = np.array(info["bounds"], np.float64)
        self.bound_ = float(self.bound_trace_[-1]) if len(self.bound_trace_) else float("nan")
        return self.embedding_

    # -- documents in pieces (online.PartialFitMixin) -------------------------------------------------------------------
    def partial_fit(self, X, y=None):
        (alpha, _), (eta, _) = self._priors()
        k = int(self.n_components)
        doc_iter = _resolve_count("doc_iter", self.doc_iter, 1)
        total = self.total_samples
        if isinstance(total, bool) or not isinstance(total, numbers.Real) or not np.isfinite(total) or not total > 0:
            raise ValueError("total_samples=%r: expected a finite number > 0" % (total,))
        flags = plain_fused_flags("online LDA")
        X = _counts(X)
        n, m = X.shape
        if n < 1:
            raise ValueError("partial_fit: no documents")
        p = self.__dict__.get("_partial")
        if p is not None and m != p["m"]:
            raise ValueError("partial_fit: X has %d words, the model was started with %d" % (m, p["m"]))
        if p is None:
            schedule = OnlineSchedule(1, 1, self.kappa, self.tau0, self.rho, 0.0)
            rng = check_random_state(self.random_state)
            lam0 = rng.gamma(100.0, 0.01, (k, m)).astype(np.float32)
            engine = Engine(get_engine(None).device)
            p = self._partial = dict(rng=rng, engine=engine, m=m, schedule=schedule,
                                     state=LdaOnlineState(engine, m, k).set_lambda(lam0))
            self._set_topics(lam0, alpha, eta)
            self.n_steps_ = 0
        gamma0 = p["rng"].gamma(100.0, 0.01, (n, k)).astype(np.float32)
        eng = p["engine"]
        eng.upload_csr(X)
        eng.set_factors(gamma0, self.components_)
        p["state"].step(eng, alpha, eta, p["schedule"].rho_at(self.n_steps_), float(total) / n, doc_iter, 1e-32, False, flags)
        self._set_topics(p["state"].get_lambda(), alpha, eta)
        gamma = eng.get_factors(want_v=False)[0]
        self.embedding_ = gamma / gamma.sum(axis=1, keepdims=True)
        self.n_steps_ += 1
        return self
