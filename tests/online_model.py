"""Shared by tests/test_online_model_host.py and tests/test_online_em.py (not a test module): the planted corpus of the online-EM
end-to-end check, its split, and a float64 restatement of the whole stepwise algorithm (enstop_amd/online.py's docstring;
DESIGN.md section 17) and of batch EM, written out in NumPy.  Everything is computed once per process (lru_cache) and
handed out read-only.
"""
import functools

import numpy as np
import scipy.sparse as sp

CORPUS = dict(n=6000, m=600, topics=10, tokens=40, background=0.1, alpha=0.3, seed=7)
FIT = dict(k=10, held_fraction=0.1, random_state=0, n_batches=64, kappa=0.7, tau0=10.0, inner_iter=3, max_epochs=5,
           batch_iterations=20)
# the smallest epoch count after which the model's held-out perplexity is at least 2 % below batch EM's after 20 iterations
# (test_online_model_host.py asserts that it is this one)
EPOCHS = 2
ROOM = 0.02


@functools.lru_cache(maxsize=None)
def planted_corpus():
    """Host NumPy, the planted kind of test_tempered_em.planted_corpus at CORPUS' sizes: topics on disjoint blocks of words
    (Zipf-like inside a block) plus a background over all words; a document mixes Dirichlet(alpha) of the topics."""
    p = CORPUS
    rs = np.random.RandomState(p["seed"])
    block = p["m"] // p["topics"]
    within = 1.0 / np.arange(1, block + 1) ** 0.7
    within /= within.sum()
    T = np.full((p["topics"], p["m"]), p["background"] / p["m"])
    for z in range(p["topics"]):
        T[z, z * block:(z + 1) * block] += (1.0 - p["background"]) * within
    theta = rs.dirichlet(np.full(p["topics"], p["alpha"]), size=p["n"])
    P = theta @ T
    P /= P.sum(1, keepdims=True)
    X = np.stack([rs.multinomial(p["tokens"], P[d]) for d in range(p["n"])])
    return sp.csr_matrix(X.astype(np.float32))


@functools.lru_cache(maxsize=None)
def the_split():
    """(observed, held, scored, U0, V0): split_documents(X, 0.9, rng), then plsa_init's random factors from the same stream"""
    from enstop_amd.plsa import plsa_init
    from enstop_amd.scoring import split_documents
    X = planted_corpus()
    rng = np.random.RandomState(FIT["random_state"])
    observed, held = split_documents(X, 1.0 - FIT["held_fraction"], rng)
    U, V = plsa_init(observed, FIT["k"], "random", rng)
    scored = (np.diff(observed.indptr) > 0) & (np.diff(held.indptr) > 0)
    return observed, held, scored, U.astype(np.float32), V.astype(np.float32)


def coo(X):
    X = X.tocsr()
    rows = np.repeat(np.arange(X.shape[0], dtype=np.int64), np.diff(X.indptr))
    return rows, X.indices.astype(np.int64), X.data.astype(np.float64)


class Block:
    """the entries of a block of documents with the two indicator matrices that sum them per document and per word"""

    def __init__(self, X):
        self.n, self.m = X.shape
        self.rows, self.cols, self.x = coo(X)
        e = np.arange(self.x.shape[0])
        one = np.ones(self.x.shape[0])
        self.by_row = sp.csr_matrix((one, (self.rows, e)), shape=(self.n, e.shape[0]))
        self.by_col = sp.csr_matrix((one, (self.cols, e)), shape=(self.m, e.shape[0]))
        self.tokens = float(self.x.sum())

    def responsibilities(self, U, V):
        """x P(z|w,d) [nnz, k] and the log-likelihood of the entries under (U, V)"""
        v = V[:, self.cols].T * U[self.rows]
        dot = v.sum(1, keepdims=True)
        ll = float((self.x * np.log(dot[:, 0])).sum())
        return v / dot * self.x[:, None], ll

    def fold(self, U, V):
        """one frozen-topic iteration: the new P(z|d)"""
        A = self.by_row @ self.responsibilities(U, V)[0]
        norm = A.sum(1, keepdims=True)
        return np.divide(A, norm, out=np.zeros_like(A), where=norm > 0)

    def accumulate(self, U, V):
        """one EM iteration's sums: the new P(z|d), the un-normalised P(w|z) sums [m, k], the log-likelihood under (U, V)"""
        s, ll = self.responsibilities(U, V)
        A = self.by_row @ s
        norm = A.sum(1, keepdims=True)
        return np.divide(A, norm, out=np.zeros_like(A), where=norm > 0), self.by_col @ s, ll


def perplexity(held, scored, U, V):
    """exp(-log-likelihood per token) of the held-out entries of the scored documents under (U, V), float64"""
    rows, cols, x = coo(held)
    dot = (V[:, cols].T * U[rows]).sum(1)
    use = scored[rows] & (dot > 0)
    return float(np.exp(-(x[use] * np.log(dot[use])).sum() / x[use].sum()))


def row_ranges(indptr, parts):
    """enstop_amd.sharded.row_ranges_by_nnz restated"""
    n, nnz = len(indptr) - 1, int(indptr[-1])
    cuts = [0]
    for r in range(1, parts):
        c = int(np.searchsorted(indptr, nnz * r / parts))
        lo = min(cuts[-1] + 1, n)
        hi = max(lo, n - (parts - r))
        cuts.append(min(max(c, lo), hi))
    cuts.append(n)
    return [(cuts[i], cuts[i + 1]) for i in range(parts)]


def stepwise(X, U0, V0, n_batches, n_epochs, inner_iter, kappa, tau0, perm=None):
    """The stepwise algorithm in float64: -> ([(P(z|d), P(w|z)) after epoch 1, 2, ...], [L_e], [rho_t]); every P(z|d) is the
    final fold (max(inner_iter, 1) frozen-topic iterations of every block under the topics of that moment, which leaves the
    run itself untouched), in the caller's order."""
    n, m = X.shape
    k = U0.shape[1]
    order = np.arange(n) if perm is None else np.asarray(perm)
    Xp = X.tocsr()[order]
    U = np.asarray(U0, np.float64)[order].copy()
    V = np.asarray(V0, np.float64).copy()
    ranges = row_ranges(Xp.indptr, n_batches)
    blocks = [Block(Xp[a:b]) for a, b in ranges]
    S = V.T / k
    t, L, rhos, factors = 0, [], [], []
    for e in range(n_epochs):
        Le = 0.0
        for blk, (a, b) in zip(blocks, ranges):
            rho = (tau0 + t) ** (-kappa)
            Ub = U[a:b]
            for _ in range(inner_iter):
                Ub = blk.fold(Ub, V)
            U[a:b], acc, ll = blk.accumulate(Ub, V)
            S = (1.0 - rho) * S + rho / blk.tokens * acc
            V = (S / S.sum(0, keepdims=True)).T
            Le += ll
            rhos.append(rho)
            t += 1
        L.append(Le)
        folded = np.empty_like(U)
        for blk, (a, b) in zip(blocks, ranges):
            Ub = U[a:b]
            for _ in range(max(inner_iter, 1)):
                Ub = blk.fold(Ub, V)
            folded[order[a:b]] = Ub
        factors.append((folded, V.copy()))
    return factors, L, rhos


def batch_em(X, U0, V0, n_iter):
    blk = Block(X.tocsr())
    U, V = np.asarray(U0, np.float64), np.asarray(V0, np.float64)
    for _ in range(n_iter):
        U, acc, _ = blk.accumulate(U, V)
        V = (acc / acc.sum(0, keepdims=True)).T
    return U, V


@functools.lru_cache(maxsize=None)
def model():
    """dict: `perm`, `online_perplexity` (after 1 .. max_epochs epochs), `L` (per epoch), `rho`, `batch_perplexity`"""
    observed, held, scored, U0, V0 = the_split()
    perm = np.random.RandomState(FIT["random_state"]).permutation(observed.shape[0])
    factors, L, rhos = stepwise(observed, U0, V0, FIT["n_batches"], FIT["max_epochs"], FIT["inner_iter"], FIT["kappa"],
                                FIT["tau0"], perm)
    Ub, Vb = batch_em(observed, U0, V0, FIT["batch_iterations"])
    return dict(perm=perm, online_perplexity=[perplexity(held, scored, U, V) for U, V in factors], L=L, rho=rhos,
                batch_perplexity=perplexity(held, scored, Ub, Vb))
