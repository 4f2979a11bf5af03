"""Host steps of the native embedding behind topic_combination="hellinger_umap" (enstop_.py:354-414 calls umap.UMAP).

UMAP as published (McInnes, Healy, Melville 2018, and umap-learn's documented defaults) on the exact distance matrix of
the stacked topics.  The device does the neighbour selection with the bandwidth search (`Engine.knn_membership`) and the
force layout (`Engine.layout`); what lies between them is O(t * n_neighbors) plus one small dense eigenproblem and stays
here: the symmetric fuzzy graph, the sampling schedule's pruning, the curve parameters a and b, the initial layout.
`Engine.hellinger_embedding` chains all of it.  There is no host implementation of the two device steps.
"""
import functools

import numpy as np
import scipy.sparse as sp

NEGATIVE_SAMPLE_RATE = 5
DISCONNECTED_BELOW = 1e-8       # Laplacian eigenvalues below this count as zero: one per connected component


@functools.lru_cache(maxsize=8)
def find_ab_params(spread=1.0, min_dist=0.1):
    """a, b of 1 / (1 + a x^(2b)) fitted to the membership target of (min_dist, spread): 1 up to min_dist, then
    exp(-(x - min_dist) / spread), on linspace(0, 3 spread, 300).  (1.577, 0.895) for the defaults."""
    from scipy.optimize import curve_fit

    def curve(x, a, b):
        return 1.0 / (1.0 + a * x ** (2 * b))

    xv = np.linspace(0, spread * 3, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    params, _ = curve_fit(curve, xv, yv)
    return float(params[0]), float(params[1])


def default_n_epochs(t):
    return 500 if t <= 10000 else 200


def fuzzy_graph(idx, member):
    """W = A + A^T - A o A^T of the directed memberships A[i, idx[i, j]] = member[i, j]: symmetric CSR, float64, sorted
    indices, no stored zeros."""
    idx = np.asarray(idx)
    t, k = idx.shape
    A = sp.csr_matrix((np.asarray(member, np.float64).ravel(), (np.repeat(np.arange(t), k), idx.ravel())), shape=(t, t))
    W = (A + A.T - A.multiply(A.T)).tocsr()
    W.eliminate_zeros()
    W.sort_indices()
    return W


def prune_for_schedule(W, n_epochs):
    """Edges below max(W) / n_epochs would be sampled less than once in n_epochs: dropped, as the schedule never reaches them."""
    W = sp.csr_matrix(W, dtype=np.float64, copy=True)
    if W.nnz:
        W.data[W.data < W.data.max() / float(n_epochs)] = 0.0
        W.eliminate_zeros()
    W.sort_indices()
    return W


def initial_layout(W, dim, seed=0):
    """(Y0 [t, dim] float32, "spectral" | "random", components).  Spectral: eigenvectors 1..dim of the symmetric normalised
    Laplacian (dense eigh: t is small), each signed so that its largest-magnitude entry is positive, scaled to
    max |.| = 10, seeded N(0, 1e-4) noise added, every coordinate rescaled to [0, 10].  A graph with more than one
    component (more than one eigenvalue below 1e-8) or too few vertices gets seeded uniform(0, 10) positions: laying out
    the components separately, as umap-learn does, is not done here."""
    t = W.shape[0]
    rng = np.random.RandomState(seed)
    A = np.asarray(W.todense(), dtype=np.float64)
    deg = A.sum(axis=1)
    with np.errstate(divide="ignore"):
        inv_sqrt = np.where(deg > 0, 1.0 / np.sqrt(deg), 0.0)
    L = np.diag((deg > 0).astype(np.float64)) - inv_sqrt[:, None] * A * inv_sqrt[None, :]     # an isolated vertex: a zero row
    L = (L + L.T) * 0.5
    vals, vecs = np.linalg.eigh(L)
    components = int((vals < DISCONNECTED_BELOW).sum())
    if components > 1 or t <= dim + 1:
        return rng.uniform(0.0, 10.0, size=(t, dim)).astype(np.float32), "random", components
    Y = vecs[:, 1:dim + 1].copy()
    top = np.abs(Y).argmax(axis=0)
    Y *= np.where(Y[top, np.arange(dim)] < 0, -1.0, 1.0)[None, :]
    Y *= 10.0 / np.abs(Y).max()
    Y += rng.normal(scale=1e-4, size=Y.shape)
    lo, hi = Y.min(axis=0), Y.max(axis=0)
    Y = 10.0 * (Y - lo) / np.where(hi > lo, hi - lo, 1.0)
    return Y.astype(np.float32), "spectral", components
