"""Held-out scoring of a fitted topic model: per-document log-likelihood and perplexity on the device.

The reference returns one log-likelihood for a whole matrix (enstop/plsa.py:329-386) and has no score / perplexity.  Here
the same terms are summed per document (Engine.score_rows, include/plsa_hip_score.h), which gives the two standard
held-out figures of pLSA:

  "fold_in":    P(z|d) is fitted on a document's tokens and the same tokens are scored.  Optimistic: it is the likelihood
                of X under its own fold-in, not a held-out number.
  "completion": every document is split into an observed and a held-out part (split_documents); P(z|d) is folded in on
                the observed part and the held-out part is scored against it.  The fold-in leaves the observed half and
                its P(z|d) on the device; the held-out half is scored there without a factor leaving it.

Words the model gives no probability are reported (`unscored`), never smoothed away.
"""
import numpy as np
from scipy.sparse import csr_matrix, issparse
from sklearn.utils import check_random_state

from ._driver import resolve_smoothing, smoothed_flags
from .engine import get_engine
from .plsa import _refit_on_engine


def split_documents(X, fraction=0.5, random_state=None):
    """(observed, held_out): two CSR matrices of X's shape and dtype whose sum is X, `fraction` of every document's mass
    observed in expectation.  Integer-valued data is thinned token by token -- ONE rng.binomial(x, fraction) call over the
    stored entries in CSR order; other data is assigned entry by entry, rng.rand(nnz) < fraction.  Zeros are eliminated
    from both halves.  Host NumPy: O(nnz) host work and two more copies of X."""
    if not 0.0 <= fraction <= 1.0:
        raise ValueError("fraction must be in [0, 1], not %r" % (fraction,))
    X = X.tocsr() if issparse(X) else csr_matrix(X)
    rng = check_random_state(random_state)
    data = X.data
    if np.any(data < 0):
        raise ValueError("split_documents needs non-negative entries")
    if np.all(data == np.floor(data)):
        observed = rng.binomial(data.astype(np.int64), fraction).astype(data.dtype)
        held = data - observed
    else:
        take = rng.rand(data.shape[0]) < fraction
        observed = np.where(take, data, 0).astype(data.dtype)
        held = np.where(take, 0, data).astype(data.dtype)
    halves = []
    for vals in (observed, held):
        half = csr_matrix((vals, X.indices.copy(), X.indptr.copy()), shape=X.shape)
        half.eliminate_zeros()
        halves.append(half)
    return halves[0], halves[1]


def _nonempty_rows(X):
    """bool [n]: the document has a stored entry > 0"""
    rows = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    return np.bincount(rows[X.data > 0], minlength=X.shape[0]) > 0


def document_log_likelihood(X, doc_topics, topics, sample_weight=None, device=None):
    """log P(document) [n], float64, for given factors: sum over the document's entries of x log(sum_z P(w|z) P(z|d))
    (times the document's weight), the terms of `log_likelihood` kept per document.  A document that holds a word the
    model gives no mass gets -inf; stored zeros are skipped; an empty document gets 0."""
    X = X.tocsr() if issparse(X) else csr_matrix(X)
    eng = get_engine(device)
    with eng.lock:
        eng.upload_csr(X)
        eng.set_factors(doc_topics, topics)
        ll, _, unscored = eng.score_rows(None, sample_weight)
    return np.where(unscored > 0, -np.inf, ll)


def held_out_scores(X, topics, method="completion", fraction=0.5, random_state=42, n_iter=50, n_iter_per_test=5,
                    tolerance=0.001, device=None, flags=None, on_zero="inf", doc_topic_smoothing=0.0):
    """Scores the documents X under the fixed `topics` [k, m]; the iteration defaults are transform's.

    method="fold_in": refit P(z|d) on X, score X.  method="completion": split_documents(X, fraction, rng), refit on the
    observed half, score the held-out half against the P(z|d) just folded in -- both under one hold of the engine lock,
    nothing downloaded or uploaded in between but the held-out half itself.  `random_state` seeds one stream: the split
    draws from it first, then the fold-in's starting P(z|d).

    Returns a dict: `log_likelihood`, `tokens`, `unscored` (float64 [n]: the scored matrix' per-document sums; `unscored`
    is the mass on words the model gives no probability, which the other two leave out), `scored_documents` (bool [n]:
    False where the observed or the held-out part is empty -- a fold-in of nothing is undefined), `perplexity` =
    exp(-sum ll / sum tokens) over the scored documents, and `n_iter` of the fold-in.  on_zero="inf": the perplexity is
    inf when a scored document has unscored mass; "skip": that mass is left out of both sums.  doc_topic_smoothing: the
    document-side pseudo-count of a smoothed model (enstop_amd.smoothed): the fold-in is then the smoothed refit."""
    doc_topic_smoothing = resolve_smoothing("doc_topic_smoothing", doc_topic_smoothing)
    if doc_topic_smoothing:
        flags = smoothed_flags(flags)            # refused here, before an engine is touched
    if method not in ("completion", "fold_in"):
        raise ValueError('method must be "completion" or "fold_in", not %r' % (method,))
    if on_zero not in ("inf", "skip"):
        raise ValueError('on_zero must be "inf" or "skip", not %r' % (on_zero,))
    X = X.tocsr() if issparse(X) else csr_matrix(X)
    rng = check_random_state(random_state)
    if method == "completion":
        observed, held = split_documents(X, fraction, rng)
        scored = _nonempty_rows(observed) & _nonempty_rows(held)
    else:
        observed, held = X, None
        scored = _nonempty_rows(X)
    eng = get_engine(device)
    with eng.lock:
        iters, _ = _refit_on_engine(eng, observed, topics, None, n_iter, n_iter_per_test, tolerance, 1e-32, rng, flags,
                                    doc_topic_smoothing=doc_topic_smoothing)
        ll, tokens, unscored = eng.score_rows(held)
    if on_zero == "inf" and np.any(unscored[scored] > 0):
        perplexity = np.inf
    else:
        total = np.sum(tokens[scored])
        perplexity = float(np.exp(-np.sum(ll[scored]) / total)) if total > 0 else np.nan
    return dict(log_likelihood=ll, tokens=tokens, unscored=unscored, scored_documents=scored, perplexity=perplexity,
                n_iter=iters)
