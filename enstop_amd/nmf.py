"""Kullback-Leibler NMF by multiplicative updates on the MI355X engine (include/plsa_hip_nmf.h).

The arithmetic is scikit-learn's `NMF(beta_loss=1, solver="mu", alpha_W=0)` -- the configuration the reference's
`model="nmf"` uses (enstop/enstop_.py:118-161) -- restated on the structures of the fused EM passes.  The starting
factors are computed on the host from public APIs (`randomized_svd`, NumPy's RandomState) and reproduce scikit-learn's
`init="nndsvd"` / `init="random"` bit for bit; everything after them runs on the device.

Which path a call takes: `backend=None | "host" | "device"` on `enstop_.nmf_topics` (and `nmf_backend=` above it);
None follows ENSTOP_AMD_NMF = host | device | auto, default host.
"""
import math
import os
import warnings

import numpy as np
from scipy.sparse import csr_matrix, issparse
from sklearn.utils import check_random_state

from .engine import get_engine
from .plsa import _locked

NMF_BACKENDS = ("host", "device", "auto")
INIT_EPS = 1e-6            # entries of the NNDSVD factors below it are set to 0 (scikit-learn's `eps`)


def requested_backend(backend):
    """(backend, explicit): `backend` as passed, or ENSTOP_AMD_NMF when it is None (default "host")."""
    if backend is None:
        backend = (os.environ.get("ENSTOP_AMD_NMF") or "host").strip().lower()
        if backend not in NMF_BACKENDS:
            raise ValueError("ENSTOP_AMD_NMF=%r: expected one of %s" % (backend, ", ".join(NMF_BACKENDS)))
        return backend, False
    if backend not in ("host", "device"):
        raise ValueError('nmf backend must be None, "host" or "device", not %r' % (backend,))
    return backend, backend == "device"


def device_obstacle(init="nndsvd", beta_loss=1, solver="mu", alpha=0.0):
    """Why the device cannot take this configuration (None: it can)."""
    if not (beta_loss == "kullback-leibler" or (not isinstance(beta_loss, str) and beta_loss == 1)):
        return "beta_loss=%r (only 1 / \"kullback-leibler\")" % (beta_loss,)
    if solver != "mu":
        return "solver=%r (only \"mu\")" % (solver,)
    if alpha != 0:
        return "alpha=%r (no regularisation)" % (alpha,)
    if isinstance(init, str):
        if init not in ("nndsvd", "random"):
            return "init=%r (only \"nndsvd\", \"random\" or a (W0, H0) tuple)" % (init,)
    elif not (isinstance(init, tuple) and len(init) == 2):
        return "init=%r (only \"nndsvd\", \"random\" or a (W0, H0) tuple)" % (init,)
    return None


def _device_present(device=None):
    try:
        get_engine(device)
        return True
    except (ImportError, OSError, RuntimeError, AttributeError):
        return False


def use_device(backend, device=None, **config):
    """True when the call runs on the device.  A configuration the device cannot carry, a missing library or GPU: the
    host under "auto" and under "device" from the environment, ValueError for an explicit backend="device" (raised for
    the configuration before any device is looked for)."""
    backend, explicit = requested_backend(backend)
    if backend == "host":
        return False
    why = device_obstacle(**config)
    if why is not None:
        if explicit:
            raise ValueError('backend="device" cannot fit NMF with ' + why)
        return False
    if _device_present(device):
        return True
    if explicit:
        raise ValueError('backend="device": the HIP library or a GPU is missing')
    return False


# ------------------------------------------------------------------------------------------------
# starting factors (host, public APIs only)
# ------------------------------------------------------------------------------------------------
def _norm(x):
    from sklearn.utils.extmath import squared_norm
    return math.sqrt(squared_norm(x))


def nmf_nndsvd(X, k, random_state=None, eps=INIT_EPS):
    """Boutsidis & Gallopoulos' non-negative double SVD as scikit-learn's NMF(init="nndsvd") computes it: a rank-k
    `randomized_svd(X, k, random_state=...)`, the leading triplet as is, every further pair replaced by the heavier of
    its positive / negative parts, entries below `eps` set to 0.  Same operations in the same order, column by column."""
    from sklearn.utils.extmath import randomized_svd
    if k > min(X.shape):
        raise ValueError("init = 'nndsvd' can only be used when n_components <= min(n_samples, n_features)")
    U, S, V = randomized_svd(X, k, random_state=random_state)
    W, H = np.zeros_like(U), np.zeros_like(V)
    W[:, 0] = np.sqrt(S[0]) * np.abs(U[:, 0])
    H[0, :] = np.sqrt(S[0]) * np.abs(V[0, :])
    for j in range(1, k):
        x, y = U[:, j], V[j, :]
        x_p, y_p = np.maximum(x, 0), np.maximum(y, 0)
        x_n, y_n = np.abs(np.minimum(x, 0)), np.abs(np.minimum(y, 0))
        x_p_nrm, y_p_nrm = _norm(x_p), _norm(y_p)
        x_n_nrm, y_n_nrm = _norm(x_n), _norm(y_n)
        m_p, m_n = x_p_nrm * y_p_nrm, x_n_nrm * y_n_nrm
        if m_p > m_n:
            u, v, sigma = x_p / x_p_nrm, y_p / y_p_nrm, m_p
        else:
            u, v, sigma = x_n / x_n_nrm, y_n / y_n_nrm, m_n
        lbd = np.sqrt(S[j] * sigma)
        W[:, j] = lbd * u
        H[j, :] = lbd * v
    W[W < eps] = 0
    H[H < eps] = 0
    return W, H


def nmf_random_init(X, k, random_state=None):
    """NMF(init="random"): avg * |standard_normal|, H drawn before W, avg = sqrt(X.mean() / k), in X's dtype."""
    n, m = X.shape
    avg = np.sqrt(X.mean() / k)
    rng = check_random_state(random_state)
    H = avg * rng.standard_normal(size=(k, m)).astype(X.dtype, copy=False)
    W = avg * rng.standard_normal(size=(n, k)).astype(X.dtype, copy=False)
    np.abs(H, out=H)
    np.abs(W, out=W)
    return W, H


def nmf_init(X, k, init="nndsvd", random_state=None):
    if isinstance(init, tuple):
        W0, H0 = init
        W0, H0 = np.asarray(W0), np.asarray(H0)
        if W0.shape != (X.shape[0], k) or H0.shape != (k, X.shape[1]):
            raise ValueError("init=(W0, H0): shapes %s, %s do not match (%d, %d) and (%d, %d)"
                             % (W0.shape, H0.shape, X.shape[0], k, k, X.shape[1]))
        return W0, H0
    if init == "nndsvd":
        return nmf_nndsvd(X, k, random_state)
    if init == "random":
        return nmf_random_init(X, k, random_state)
    raise ValueError('init must be "nndsvd", "random" or a (W0, H0) tuple, not %r' % (init,))


def refit_start(X, k):
    """W of non_negative_factorization(update_H=False, solver="mu"): sqrt(X.mean() / k) everywhere."""
    return np.full((X.shape[0], k), np.sqrt(X.mean() / k), dtype=np.float32)


# ------------------------------------------------------------------------------------------------
# fits
# ------------------------------------------------------------------------------------------------
def _as_csr32(X):
    A = X.tocsr() if issparse(X) else csr_matrix(X)
    return A.astype(np.float32, copy=False)


def _warn_max_iter(n_iter, max_iter, tol):
    if n_iter == max_iter and tol > 0:
        from sklearn.exceptions import ConvergenceWarning
        warnings.warn("Maximum number of iterations %d reached. Increase it to improve convergence." % max_iter,
                      ConvergenceWarning)


def fit_on_engine(eng, W0, H0, update_h=True, max_iter=200, tol=1e-4):
    """The driver on the matrix that is active on `eng`; returns (n_iter, errors)."""
    eng.nmf_set_factors(W0, H0)
    n_iter, errors = eng.nmf_fit(update_h=update_h, max_iter=max_iter, tol=tol)
    _warn_max_iter(n_iter, max_iter, tol)
    return n_iter, errors


@_locked
def nmf_fit(X, k, init="nndsvd", max_iter=200, tol=1e-4, random_state=None, device=None):
    """KL-divergence NMF of X on the device: (W [n, k], H [k, m], n_iter), float32.  `init`: "nndsvd", "random" or a
    (W0, H0) tuple; ConvergenceWarning when max_iter is reached with tol > 0, like scikit-learn."""
    A = _as_csr32(X)
    W0, H0 = nmf_init(A, int(k), init, random_state)
    eng = get_engine(device)
    eng.upload_csr(A)
    n_iter, _ = fit_on_engine(eng, W0, H0, True, max_iter, tol)
    W, H = eng.nmf_get_factors()
    return W, H, n_iter


@_locked
def nmf_refit(X, H, max_iter=200, tol=1e-4, device=None):
    """Document vectors against fixed topics H [k, m] (non_negative_factorization(update_H=False)): (W [n, k], n_iter)."""
    A = _as_csr32(X)
    H = np.ascontiguousarray(H, dtype=np.float32)
    if H.ndim != 2 or H.shape[1] != A.shape[1]:
        raise ValueError("H has shape %s, expected (k, %d)" % (H.shape, A.shape[1]))
    eng = get_engine(device)
    eng.upload_csr(A)
    n_iter, _ = fit_on_engine(eng, refit_start(A, H.shape[0]), H, False, max_iter, tol)
    W, _ = eng.nmf_get_factors(want_h=False)
    return W, n_iter
