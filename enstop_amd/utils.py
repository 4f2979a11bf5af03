"""Helpers with the reference's names (enstop/utils.py): input standardisation and sample-weight validation used by the
estimators (host-side, not hot-path code), and the topic-quality metrics -- coherence counts on the device when one is
there (plsa_codocument_counts), everything else on the host."""
import os

import numpy as np
from sklearn.preprocessing import normalize as _sk_normalize

from .engine import get_engine, host_normalize_rows


def normalize(ndarray, axis=0):
    """L1-normalise a 2-D float64 array IN PLACE along `axis` (enstop/utils.py:8-41): sequential
    float64 marginal, division only where the marginal is positive."""
    if ndarray.ndim != 2 or axis not in (0, 1):
        raise ValueError("axis must be 0 or 1")
    if axis == 1 and ndarray.dtype == np.float64 and ndarray.flags.c_contiguous:
        host_normalize_rows(ndarray)
        return
    work = np.ascontiguousarray(ndarray.T if axis == 0 else ndarray, dtype=np.float64)
    host_normalize_rows(work)
    ndarray[...] = work.T if axis == 0 else work


def standardize_input(input_matrix):
    """Float inputs are L1 row-normalised, integer counts pass through (enstop/utils.py:276-280).
    The reference tests `dtype in (np.float32, np.float64, np.float, np.double)`; `np.float` no
    longer exists in NumPy >= 1.24, the intended float test is applied here."""
    if input_matrix.dtype in (np.float32, np.float64):
        return _sk_normalize(input_matrix, norm="l1")
    return input_matrix


# sample-weight validation: scikit-learn's own validator, as the reference imports it by default
# (enstop/plsa.py:9, enstop_.py:8; its vendored copy enstop/utils.py:285-335 is only a fallback for
# scikit-learn versions that predate the function)
try:
    from sklearn.utils.validation import _check_sample_weight  # noqa: E402,F401
except ImportError:          # a private name: keep working if a scikit-learn release moves it
    def _check_sample_weight(sample_weight, X, dtype=None):
        """Fallback with the contract of enstop/utils.py:285-335: None -> ones, a number -> constant vector,
        otherwise a 1-D float array of length n_samples."""
        n = X.shape[0]
        dtype = np.float64 if dtype is None else dtype
        if sample_weight is None:
            return np.ones(n, dtype=dtype)
        if isinstance(sample_weight, (int, float, np.integer, np.floating)):
            return np.full(n, sample_weight, dtype=dtype)
        sw = np.asarray(sample_weight, dtype=dtype)
        if sw.ndim != 1:
            raise ValueError("Sample weights must be 1D array or scalar")
        if sw.shape != (n,):
            raise ValueError("sample_weight.shape == {}, expected {}!".format(sw.shape, (n,)))
        return sw


# ------------------------------------------------------------------------------------------------
# topic-quality metrics (enstop/utils.py:44-273): log-lift in host NumPy; the counts behind coherence on the device or the host
# ------------------------------------------------------------------------------------------------
def _empirical_probs(data):
    p = np.asarray(data.sum(axis=0)).squeeze().astype(np.float64)
    return p / p.sum()


def _log_lift(topics, z, empirical_probs, n=-1):
    words = np.arange(topics.shape[1]) if n <= 0 else np.argsort(topics[z])[-n:]
    ok = empirical_probs[words] > 0
    total = np.sum(topics[z, words][ok] * 1.0 / empirical_probs[words][ok])
    return np.log(total * 1.0 / len(words))


def log_lift(topics, z, data, n_words=-1):
    """log of the mean lift P(w|z) / P(w) over the topic's top `n_words` words (all when <= 0)."""
    t = np.array(topics, dtype=np.float64)
    normalize(t, axis=1)
    return _log_lift(t.astype(np.asarray(topics).dtype), z, _empirical_probs(data), n_words)


def mean_log_lift(topics, data, n_words=-1):
    """Mean over topics; like the reference it scores the topics AS GIVEN (enstop/utils.py:144 passes
    the un-normalised array) -- identical for the normalised topics the estimators produce."""
    e = _empirical_probs(data)
    return np.mean([_log_lift(np.asarray(topics), z, e, n_words) for z in range(np.asarray(topics).shape[0])])


def _coherence_from_counts(co, positive):
    """Coherence of one word list from its counts (the sum of enstop/utils.py:186-197): co [nw, nw] co-document counts of
    the list's words in their order, positive [nw] documents in which each word has a positive count.  Both back-ends
    finish here, so they return the same float64 bits."""
    co = np.asarray(co, dtype=np.float64)
    n = co.shape[0]
    total = 0.0
    for i in range(n - 1):
        if positive[i] == 0:
            continue
        total += np.sum(np.log((co[i, i + 1:] + 1.0) / positive[i]))
    return total


def _top_words(topics, z, n):
    return np.argsort(topics[z])[-n:]       # ascending: word i of the list is the denominator of every pair (i, j > i)


def _host_counts(top, B, n_docs_per_word):
    sub = B[:, top]
    co = np.asarray((sub.T @ sub).todense(), dtype=np.float64)        # co-document counts of the top words
    return co, n_docs_per_word[top]


def _coherence(topics, z, n, B, n_docs_per_word):
    return _coherence_from_counts(*_host_counts(_top_words(topics, z, n), B, n_docs_per_word))


def _binarised(data):
    from scipy.sparse import csc_matrix, issparse
    B = data.tocsc() if issparse(data) else csc_matrix(data)
    B = B.copy()
    B.data = np.ones_like(B.data, dtype=np.float64)       # stored entries count as occurrences, as the
    n_docs = np.asarray((data > 0).sum(axis=0)).squeeze()  # reference's index intersection does
    return B, n_docs


# -- back-end of the coherence counts ---------------------------------------------------------------------------------
METRIC_BACKENDS = ("host", "device", "auto")
DEVICE_MAX_WORDS = 32        # bits of a document mask (plsa_metric_kernels.hpp)
last_metric_path = None      # "device" / "host": where the counts of the last coherence / mean_coherence call were taken
_device_seen = None


def _device_present():
    """True when the library loads and the process-wide engine can be had (cached once it could)."""
    global _device_seen
    if _device_seen is None:
        try:
            get_engine()
            _device_seen = True
        except (ImportError, OSError, RuntimeError, AttributeError):
            return False          # not cached: a library built later in the process is found
    return _device_seen


def _requested_backend(backend):
    if backend is None:
        backend = (os.environ.get("ENSTOP_AMD_METRICS") or "auto").strip().lower()
        if backend not in METRIC_BACKENDS:
            raise ValueError("ENSTOP_AMD_METRICS=%r: expected one of %s" % (backend, ", ".join(METRIC_BACKENDS)))
        return backend, False
    if backend not in ("host", "device"):
        raise ValueError('backend must be None, "host" or "device", not %r' % (backend,))
    return backend, backend == "device"


def _device_obstacle(topics, data, n_words):
    """Why the device cannot take this call (None: it can)."""
    from scipy.sparse import issparse
    if not 2 <= n_words <= DEVICE_MAX_WORDS:
        return "n_words=%r outside [2, %d]" % (n_words, DEVICE_MAX_WORDS)
    if not issparse(data):
        return "dense data"
    if data.format not in ("csr", "csc") or not data.has_canonical_format:
        return "a sparse matrix that is not in canonical CSR / CSC format (duplicate or unsorted entries)"
    n, m = data.shape
    if topics.ndim != 2 or topics.shape[0] < 1 or topics.shape[1] != m or n_words > m:
        return "topics that do not match the data (or fewer than n_words words)"
    if n < 1 or data.nnz > 2 ** 31 - 64 or max(n, m) >= 2 ** 31 - 1:
        return "a matrix outside the device's 32-bit index range"
    return None


def _use_device(topics, data, n_words, backend):
    backend, explicit = _requested_backend(backend)
    if backend == "host" or n_words == 1:          # (one word: no pairs, 0.0 on either path)
        return False
    why = _device_obstacle(topics, data, n_words)
    if why is not None:
        if explicit:
            raise ValueError('backend="device" cannot score ' + why)
        return False
    return True if backend == "device" else _device_present()


def _device_counts(words, data):
    """(co [sets, nw, nw], positive [sets, nw]) of the word lists on `data`, counted on the device: the engine lock of the
    fit functions, one upload of the corpus' pattern, one call."""
    from scipy.sparse import csr_matrix
    X = data.tocsr()
    # the values travel as (value > 0): a cast of the real ones to float32 could flush a tiny positive float64 to zero
    pattern = csr_matrix(((X.data > 0).astype(np.float32), X.indices, X.indptr), shape=X.shape)
    eng = get_engine()
    with eng.lock:
        eng.upload_csr(pattern)
        return eng.codocument_counts(words)


def coherence(topics, z, data, n_words=20, backend=None):
    """UMass-style coherence of topic z over its top `n_words` words (enstop/utils.py:155-197).
    backend: "host" (NumPy / SciPy), "device" (the counts on the GPU: sparse canonical data, 2 <= n_words <= 32, else
    ValueError) or None: ENSTOP_AMD_METRICS = host | device | auto (default auto: the device when there is one and it can
    carry the call).  Both give the same float64 bits; `last_metric_path` says which ran."""
    global last_metric_path
    topics = np.asarray(topics)
    if _use_device(topics, data, n_words, backend):
        co, positive = _device_counts(_top_words(topics, z, n_words)[None, :], data)
        last_metric_path = "device"
        return _coherence_from_counts(co[0], positive[0])
    B, n_docs = _binarised(data)
    last_metric_path = "host"
    return _coherence(topics, z, n_words, B, n_docs)


def mean_coherence(topics, data, n_words=20, backend=None):
    """Mean of coherence() over the topics; on the device all topics' lists go through one call."""
    global last_metric_path
    topics = np.asarray(topics)
    if _use_device(topics, data, n_words, backend):
        words = np.stack([_top_words(topics, z, n_words) for z in range(topics.shape[0])])
        co, positive = _device_counts(words, data)
        last_metric_path = "device"
        return np.mean([_coherence_from_counts(co[z], positive[z]) for z in range(topics.shape[0])])
    B, n_docs = _binarised(data)
    last_metric_path = "host"
    return np.mean([_coherence(topics, z, n_words, B, n_docs) for z in range(topics.shape[0])])
