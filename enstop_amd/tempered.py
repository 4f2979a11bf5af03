"""Tempered EM with held-out early stopping (Hofmann 1999 / 2001), on the device.

pLSA fitted until its training likelihood flattens memorises its documents: the held-out perplexity
(scoring.held_out_scores, method="completion") passes a minimum long before.  The cure the model was published with flattens
the responsibilities by an exponent beta <= 1 and lets a held-out likelihood decide when to stop and when to lower beta:

    P_beta(z|d,w) = (P(z|d) P(w|z))^beta / sum_z' (P(z'|d) P(w|z'))^beta

`Engine.fit_tempered` runs such iterations (include/plsa_hip_tempered.h); this module holds what decides about beta:

  TemperingSchedule   a state machine without an engine in it: fed validation perplexities, it answers with actions
  plsa_fit_tempered   holds out a share of every document's tokens, fits the rest, and drives the schedule with
                      Engine.fit_tempered, Engine.score_rows(other=held_out) and the engine's factor snapshot

The rule and every default below (eta, beta_min, rel_tol, the burst length, the iteration budget) are this package's
choices; the papers describe the scheme, not these values.
"""
import math

import numpy as np
from scipy.sparse import csr_matrix, issparse
from sklearn.utils import check_random_state

from ._driver import effective_weights, init_factors, resolve_flags
from .engine import PLSA_FUSED, PLSA_STOP_NO_ZERO_ARM, get_engine
from .plsa import _locked, _refit_on_engine
from .scoring import _nonempty_rows, split_documents

SNAPSHOT, RESTORE, BURST, STOP = "snapshot", "restore", "burst", "stop"


class TemperingSchedule:
    """Decides what a tempered fit does next; it never touches an engine.

        actions = schedule.start()                  # [("snapshot",), ("burst", 1.0, n)]
        while actions[-1][0] == "burst":
            ... carry the actions out in order, take the validation perplexity after the burst ...
            actions = schedule.observe(perplexity)

    Actions: ("snapshot",) keep the current factors; ("restore",) go back to the kept ones; ("burst", beta, iterations) run
    that many EM iterations at beta with a tolerance of 0, so that the training likelihood never ends a burst; ("stop",).

    The rule:
      1. start at beta = 1 (the starting factors are kept first, so that a restore is always possible);
      2. run bursts of n_iter_per_test iterations;
      3. a burst whose validation perplexity improves on the best so far by more than rel_tol (relative) is kept, and the
         next burst runs at the same beta;
      4. otherwise the kept factors come back, beta <- eta * beta, and ONE burst runs at the new beta;
      5. if that burst does not improve on the best either, the fit stops;
      6. it also stops when beta would fall below beta_min, and when n_iter iterations are spent (discarded bursts count);
      7. whatever ends it, the factors in force at the stop are the kept ones.
    A perplexity that is NaN or infinite is no improvement.

    `history` has one record per observed burst (beta, iterations, spent, perplexity, improved, actions: what observe
    answered); `selected` is the record of the kept burst, or None while only the starting factors are kept."""

    def __init__(self, eta=0.9, beta_min=0.5, rel_tol=1e-4, n_iter_per_test=10, n_iter=200):
        if not 0.0 < eta < 1.0:
            raise ValueError("eta must be in (0, 1), not %r" % (eta,))
        if not 0.0 < beta_min <= 1.0:
            raise ValueError("beta_min must be in (0, 1], not %r" % (beta_min,))
        if not rel_tol >= 0.0:
            raise ValueError("rel_tol must be >= 0, not %r" % (rel_tol,))
        if int(n_iter_per_test) < 1 or int(n_iter) < 0:
            raise ValueError("n_iter_per_test must be >= 1 and n_iter >= 0")
        self.eta, self.beta_min, self.rel_tol = float(eta), float(beta_min), float(rel_tol)
        self.n_iter_per_test, self.n_iter = int(n_iter_per_test), int(n_iter)
        self.beta = 1.0
        self.best = math.inf
        self.spent = 0
        self.selected = None
        self.history = []
        self.stopped = False
        self._pending = None           # (beta, iterations) of the burst whose perplexity is awaited
        self._lowered = False          # that burst is the one burst granted to a freshly lowered beta

    def _burst(self):
        iterations = min(self.n_iter_per_test, self.n_iter - self.spent)
        self._pending = (self.beta, iterations)
        return (BURST, self.beta, iterations)

    def _stop(self):
        self.stopped = True
        self._pending = None
        return (STOP,)

    def start(self):
        if self._pending is not None or self.history or self.stopped:
            raise RuntimeError("the schedule has already started")
        if self.n_iter == 0:
            return [(SNAPSHOT,), self._stop()]
        return [(SNAPSHOT,), self._burst()]

    def observe(self, validation_perplexity):
        if self._pending is None:
            raise RuntimeError("no burst is pending: call start() first, and nothing after a stop")
        beta, iterations = self._pending
        self.spent += iterations
        p = float(validation_perplexity)
        improved = math.isfinite(p) and (p < self.best * (1.0 - self.rel_tol) if math.isfinite(self.best) else True)
        record = dict(beta=beta, iterations=iterations, spent=self.spent, perplexity=p, improved=improved)
        if improved:
            self.best = p
            self.selected = record
            self._lowered = False
            actions = [(SNAPSHOT,), self._stop() if self.spent >= self.n_iter else self._burst()]
        else:
            actions = [(RESTORE,)]
            lower = self.eta * self.beta
            if self._lowered or lower < self.beta_min or self.spent >= self.n_iter:
                actions.append(self._stop())
            else:
                self.beta = lower
                self._lowered = True
                actions.append(self._burst())
        record["actions"] = actions
        self.history.append(record)
        return actions


def validation_perplexity(ll, tokens, unscored, scored):
    """(perplexity, unscored share) from Engine.score_rows' three sums over the documents `scored`: exp(-sum ll / sum tokens),
    the mass on words the model gives no probability left out of both sums (scoring.held_out_scores, on_zero="skip") and
    reported as its share of the held-out mass."""
    total, left_out = float(np.sum(tokens[scored])), float(np.sum(unscored[scored]))
    perplexity = float(np.exp(-np.sum(ll[scored]) / total)) if total > 0 else float("nan")
    return perplexity, (left_out / (total + left_out) if total + left_out > 0 else 0.0)


@_locked
def plsa_fit_tempered(X, k, sample_weight=None, init="random", validation_fraction=0.1, eta=0.9, beta_min=0.5, rel_tol=1e-4,
                      n_iter_per_test=10, n_iter=200, e_step_thresh=1e-32, transform_random_seed=42, random_state=None,
                      device=None, callback=None, flags=None):
    """pLSA with k topics by tempered EM, stopped and tempered by a held-out likelihood; -> (P(z|d) [n, k], P(w|z) [k, m],
    report).

    1. `validation_fraction` of every document's tokens is held out (scoring.split_documents with
       fraction = 1 - validation_fraction, drawn from `random_state` before anything else).
    2. The observed part becomes the resident corpus and the factors are initialised exactly as plsa_fit initialises them.
    3. TemperingSchedule (its rule is stated there; eta, beta_min, rel_tol, n_iter_per_test, n_iter go to it) is driven with
       Engine.fit_tempered for the bursts, Engine.score_rows(other=held_out) for the validation perplexity -- the observed
       part's P(z|d) IS the fold-in on the observed part, and the resident corpus stays -- and the engine's snapshot slot.
       Nothing but the held-out part and the per-document sums crosses the bus during the loop.
    4. The validation perplexity is exp(-sum ll / sum tokens) over the documents whose observed and held-out parts are both
       non-empty; mass on words the model gives no probability is left out and its share reported.
    5. P(w|z) is the kept snapshot.  P(z|d) is the fold-in of the WHOLE X against it, as PLSA.transform does it (50
       iterations, a test every 5, tolerance 0.001, transform_random_seed): one vector per document over all its tokens.

    report: `betas`, `iterations`, `perplexities`, `training_log_likelihoods`, `unscored_shares`, `improved` (one entry per
    burst), `actions` (what the schedule answered after each burst), `initial_training_log_likelihood`, `selected_beta`,
    `selected_iteration`, `selected_perplexity` (None when no burst was kept), `unscored_share` (of the kept burst),
    `n_iter` (iterations spent), `scored_documents`.  callback(report_so_far, engine) is called after every burst's test,
    before the schedule's answer is carried out: the engine then holds that burst's factors and the observed corpus."""
    if not 0.0 < validation_fraction < 1.0:
        raise ValueError("validation_fraction must be in (0, 1), not %r" % (validation_fraction,))
    flags = resolve_flags(flags, extra=PLSA_STOP_NO_ZERO_ARM)
    if not flags & PLSA_FUSED:
        raise ValueError("tempered EM runs the fused schedule only (ENSTOP_AMD_MATERIALISE / flags without PLSA_FUSED)")
    X = X.tocsr() if issparse(X) else csr_matrix(X)
    rng = check_random_state(random_state)
    schedule = TemperingSchedule(eta, beta_min, rel_tol, n_iter_per_test, n_iter)
    observed, held = split_documents(X, 1.0 - validation_fraction, rng)
    scored = _nonempty_rows(observed) & _nonempty_rows(held)
    sw = effective_weights(sample_weight)
    eng = get_engine(device)
    eng.upload_csr(observed)
    # the initialisation of plsa_fit, and the likelihood of the starting factors: a traced fit of no iteration
    init_factors(eng, k, init, rng, observed)
    _, ll0 = eng.fit(sw, 0, n_iter_per_test, 0.0, e_step_thresh, flags, trace=True)
    report = dict(betas=[], iterations=[], perplexities=[], training_log_likelihoods=[], unscored_shares=[], improved=[],
                  actions=[], initial_training_log_likelihood=float(ll0[0]) if len(ll0) else None, selected_beta=None,
                  selected_iteration=0, selected_perplexity=None, unscored_share=0.0, n_iter=0,
                  scored_documents=int(np.sum(scored)), validation_fraction=float(validation_fraction))
    actions = schedule.start()
    while True:
        for action in actions:
            if action[0] == SNAPSHOT:
                eng.snapshot_factors()
            elif action[0] == RESTORE:
                eng.restore_factors()
        if actions[-1][0] == STOP:
            break
        _, beta, iterations = actions[-1]
        # one test per burst and a tolerance of 0: the training likelihood never ends a burst
        eng.fit_tempered(beta, sw, iterations, iterations, 0.0, e_step_thresh, flags)
        perplexity, share = validation_perplexity(*eng.score_rows(held, sw), scored)
        report["betas"].append(beta)
        report["iterations"].append(iterations)
        report["perplexities"].append(perplexity)
        report["unscored_shares"].append(share)
        report["training_log_likelihoods"].append(eng.log_likelihood(sw))
        report["n_iter"] += iterations
        if callback is not None:
            callback(report, eng)
        actions = schedule.observe(perplexity)
        report["actions"].append(actions)
        report["improved"].append(schedule.history[-1]["improved"])
        if schedule.selected is schedule.history[-1]:
            report.update(selected_beta=beta, selected_iteration=schedule.spent, selected_perplexity=perplexity,
                          unscored_share=share)
    _, topics = eng.get_factors(want_u=False)
    _refit_on_engine(eng, X, topics, sample_weight, 50, 5, 0.001, 1e-32, check_random_state(transform_random_seed),
                     flags & ~PLSA_STOP_NO_ZERO_ARM)
    doc_topics, _ = eng.get_factors(want_v=False)
    return doc_topics, topics, report


@_locked
def plsa_fit_fixed_beta(X, k, beta, sample_weight=None, init="random", n_iter=100, n_iter_per_test=10, tolerance=0.001,
                        e_step_thresh=1e-32, random_state=None, device=None, flags=None):
    """plsa_fit with every EM iteration tempered by the one exponent 0 < beta <= 1: all of X is fitted, the training
    likelihood stops the fit as usual.  -> (P(z|d), P(w|z), dict(n_iter, log_likelihood_trace))."""
    if not 0.0 < float(beta) <= 1.0:
        raise ValueError("beta must be in (0, 1], not %r" % (beta,))
    flags = resolve_flags(flags)
    if not flags & PLSA_FUSED:
        raise ValueError("tempered EM runs the fused schedule only (ENSTOP_AMD_MATERIALISE / flags without PLSA_FUSED)")
    X = X.tocsr() if issparse(X) else csr_matrix(X)
    eng = get_engine(device)
    eng.upload_csr(X)
    init_factors(eng, k, init, check_random_state(random_state), X)
    iters, ll = eng.fit_tempered(float(beta), effective_weights(sample_weight), n_iter, n_iter_per_test, tolerance,
                                 e_step_thresh, flags, trace=True)
    U, V = eng.get_factors()
    return U, V, dict(n_iter=iters, log_likelihood_trace=ll)
