"""float64 restatement of scikit-learn 1.7's Kullback-Leibler multiplicative updates (sparse X, beta_loss = 1, gamma = 1, no
regularisation: `_multiplicative_update_w`, `_multiplicative_update_h`, `_beta_divergence`, `_fit_multiplicative_update`)
and the corpora the NMF tests share.  Vectorised NumPy / SciPy, no scikit-learn internals: tests/test_nmf_host.py pins it
to scikit-learn through the public estimator, tests/test_nmf_device.py holds the device to it."""
import numpy as np
import scipy.sparse as sp

EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)


def _coo(X):
    X = sp.csr_matrix(X)
    rows = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    return X, rows, X.indices


def wh_entries(X, W, H):
    """(WH)_dw at the STORED entries of X, in CSR order, unclamped"""
    X, rows, cols = _coo(X)
    return np.multiply(W[rows, :], H.T[cols, :]).sum(axis=1)        # the summation order of scikit-learn's _special_sparse_dot


def step64(X, W, H, update_H=True, details=None):
    """one iteration of _fit_multiplicative_update: (W_new, H_new), float64.  `details` (a dict) receives the unclamped
    (WH) of both halves and H before its entries below float64 eps are zeroed."""
    X, rows, cols = _coo(X)
    W, H = np.asarray(W, np.float64), np.asarray(H, np.float64)
    data = X.data.astype(np.float64)

    def quotient(W, H):
        wh = wh_entries(X, W, H)
        if details is not None:
            details.setdefault("wh", []).append(wh.copy())
        wh[wh < EPS32] = EPS32
        return sp.csr_matrix((data / wh, X.indices, X.indptr), shape=X.shape)

    numerator = quotient(W, H) @ H.T
    H_sum = H.sum(axis=1)
    H_sum[H_sum == 0] = EPS32
    W = W * (numerator / H_sum[None, :])
    if update_H:
        numerator = (quotient(W, H).T @ W).T
        W_sum = W.sum(axis=0)
        W_sum[W_sum == 0] = 1.0
        H = H * (numerator / W_sum[:, None])
        if details is not None:
            details["H_unclamped"] = H.copy()
        H[H < EPS64] = 0.0
    return W, H


def step64_h(X, W, H, details=None):
    """the H half alone, from a given (already updated) W: (W, H_new)"""
    X, rows, cols = _coo(X)
    W, H = np.asarray(W, np.float64), np.asarray(H, np.float64)
    wh = wh_entries(X, W, H)
    if details is not None:
        details.setdefault("wh", []).append(wh.copy())
    wh[wh < EPS32] = EPS32
    Q = sp.csr_matrix((X.data.astype(np.float64) / wh, X.indices, X.indptr), shape=X.shape)
    W_sum = W.sum(axis=0)
    W_sum[W_sum == 0] = 1.0
    H = H * ((Q.T @ W).T / W_sum[:, None])
    if details is not None:
        details["H_unclamped"] = H.copy()
    H = H.copy()
    H[H < EPS64] = 0.0
    return W, H


def divergence64(X, W, H, want_d=False):
    """_beta_divergence(X, W, H, 1, square_root=True); want_d: (D, sum x max(1, |log(x / wh)|)) instead"""
    X = sp.csr_matrix(X)
    W, H = np.asarray(W, np.float64), np.asarray(H, np.float64)
    wh = wh_entries(X, W, H)
    x = X.data.astype(np.float64)
    keep = x > EPS32
    wh, x = wh[keep], x[keep]
    wh[wh < EPS32] = EPS32
    logs = np.log(x / wh)
    D = np.dot(x, logs) + (np.dot(W.sum(axis=0), H.sum(axis=1)) - x.sum())
    if want_d:
        return D, float(np.dot(x, np.maximum(1.0, np.abs(logs))))
    return np.sqrt(2.0 * max(D, 0.0))


def fit64(X, W, H, update_H=True, max_iter=200, tol=1e-4):
    """_fit_multiplicative_update: (W, H, n_iter, errors, ratios) -- errors[0] = error_at_init, then every tested error"""
    error_at_init = divergence64(X, W, H)
    errors, ratios, previous = [error_at_init], [], error_at_init
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        W, H = step64(X, W, H, update_H)
        if tol > 0 and n_iter % 10 == 0:
            error = divergence64(X, W, H)
            errors.append(error)
            ratios.append((previous - error) / error_at_init)
            if ratios[-1] < tol:
                break
            previous = error
    return W, H, n_iter, np.array(errors), np.array(ratios)


E2E_LENGTH = 400       # tokens per document of the end-to-end corpus (test_nmf_host.py checks the reference recovers it)


# ---- corpora ------------------------------------------------------------------------------------------------------
def planted_corpus(n=300, m=120, k0=6, seed=1, length=60):
    """Poisson counts from k0 Dirichlet topics; document 7 and word 11 are empty.  Returns (X csr float32, topics [k0, m])."""
    rs = np.random.RandomState(seed)
    topics = rs.dirichlet(np.full(m, 0.05), size=k0)
    mix = rs.dirichlet(np.full(k0, 0.2), size=n)
    X = rs.poisson(length * (mix @ topics)).astype(np.float32)
    X[7, :] = 0
    X[:, 11] = 0
    return sp.csr_matrix(X), topics


def planted_start(n, m, k, seed=1):
    rs = np.random.RandomState(seed)
    return (rs.rand(n, k) + 0.01).astype(np.float32), (rs.rand(k, m) + 0.01).astype(np.float32)


def edge_corpus(k, n=301, m=257, seed=3):
    """The corpus of the half-iteration tests and its start (X csr float32, W0 [n, k], H0 [k, m], float32):
    document 5 empty, document 3 with an all-zero W row, topic 2 with an all-zero H row (zero H_sum), topic 1 with an all-zero
    W column (zero W_sum), word 9 empty, word 0 in every other document (several column items, more than one chunk of 16),
    documents 20 .. 29 with 90 entries, stored zeros, fractional counts and counts above 255 (packed escapes, below 1/16 of
    the entries), n = 301 (no multiple of any number of groups per block)."""
    rs = np.random.RandomState(seed)
    dense = (rs.rand(n, m) < 0.06) * rs.randint(1, 6, size=(n, m))
    dense = dense.astype(np.float64)
    dense[20:30, :] = (rs.rand(10, m) < 0.36) * rs.randint(1, 4, size=(10, m))
    dense[:, 0] = rs.randint(1, 4, size=n)
    X = sp.csr_matrix(dense)
    X.data = X.data.astype(np.float32)
    pick = rs.permutation(X.nnz)
    X.data[pick[:40]] = 0.0                                  # stored zeros
    X.data[pick[40:120]] = rs.rand(80).astype(np.float32) * 3 + 0.25
    X.data[pick[120:160]] = rs.randint(256, 2000, size=40)
    X = X.tolil()
    X[5, :] = 0
    X[:, 9] = 0
    X = X.tocsr()
    W0 = (rs.rand(n, k) + 0.01).astype(np.float32)
    H0 = (rs.rand(k, m) + 0.01).astype(np.float32)
    W0[3, :] = 0
    if k >= 3:
        W0[:, 1] = 0
        H0[2, :] = 0
    return X, W0, H0


def long_rows_corpus(k, n=12, m=4000, per_row=3000, seed=4):
    """12 documents of 3000 entries: few, long rows -- what puts a context into row-item mode"""
    rs = np.random.RandomState(seed)
    indices = np.concatenate([np.sort(rs.choice(m, per_row, replace=False)) for _ in range(n)]).astype(np.int32)
    data = rs.randint(1, 5, size=n * per_row).astype(np.float32)
    X = sp.csr_matrix((data, indices, np.arange(n + 1, dtype=np.int32) * per_row), shape=(n, m))
    return X, (rs.rand(n, k) + 0.01).astype(np.float32), (rs.rand(k, m) + 0.01).astype(np.float32)
