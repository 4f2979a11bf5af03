"""Shared by tests/test_lda_online_model_host.py and tests/test_lda_online.py (not a test module): a float64 restatement of the
whole online variational Bayes LDA algorithm (enstop_amd/lda_online.py's docstring) and of batch LDA,
written out in NumPy on the planted corpus of tests/online_model.py, with its kind of split.  Everything is computed once per
process (lru_cache) and handed out read-only.

    A_dz = exp(psi(gamma_dz) - psi(S_d))        B_zw = exp(psi(lambda_zw) - psi(S_z))        phi_dwz ~ A_dz B_zw
    a round on a block:    gamma_dz = alpha + sum_w x_dw phi_dwz ;    the last round of a step also n_wz = sum_d x_dw phi_dwz
    a step:                doc_iter rounds, then lambda <- (1 - rho) lambda + rho (eta + (D / n_b) n_wz)
    its bound_partial:     sum x_dw log sum_z A'_dz B_zw + the Dirichlet part of gamma' with its constant, A' from the gamma'
                           the step left, B from the lambda the step started from

Blocks keep their gamma between epochs.  The held-out perplexity is online_model.perplexity under the means of the two
Dirichlets: gamma and lambda with their rows normalised.
"""
import functools

import numpy as np
from scipy.special import psi

import lda_model as lm
import online_model as om

FIT = dict(k=10, alpha=0.1, eta=0.01, held_fraction=0.1, random_state=0, n_batches=64, kappa=0.7, tau0=10.0, doc_iter=3,
           max_epochs=5, batch_iterations=20)
# the smallest epoch count after which the model's held-out perplexity is at least 2 % below batch LDA's after 20 iterations
# from the same start (test_lda_online_model_host.py asserts that it is this one)
EPOCHS = 2
ROOM = 0.02


@functools.lru_cache(maxsize=None)
def the_split():
    """(observed, held, scored, gamma0, lam0): split_documents(X, 0.9, rng), then lda_init's random start from the same stream"""
    from enstop_amd.lda import lda_init
    from enstop_amd.scoring import split_documents
    X = om.planted_corpus()
    rng = np.random.RandomState(FIT["random_state"])
    observed, held = split_documents(X, 1.0 - FIT["held_fraction"], rng)
    gamma0, lam0 = lda_init(observed, FIT["k"], "random", rng)
    scored = (np.diff(observed.indptr) > 0) & (np.diff(held.indptr) > 0)
    return observed, held, scored, gamma0, lam0


def table(T):
    """exp(psi(T) - psi(row sums)) of the rows of T"""
    return np.exp(psi(T) - psi(T.sum(1, keepdims=True)))


def rounds(blk, gamma, B, alpha, n_rounds):
    """n_rounds rounds on the block from gamma under the table B [k, m]: -> (gamma', n_wz [m, k] of the last round)"""
    acc = None
    for _ in range(n_rounds):
        s, _ = blk.responsibilities(table(gamma), B)
        gamma, acc = alpha + blk.by_row @ s, blk.by_col @ s
    return gamma, acc


def bound_partial(blk, gamma, B, alpha):
    """the block's bound without the topic part at (gamma, the lambda B was formed from)"""
    _, ll = blk.responsibilities(table(gamma), B)
    return ll + lm.dirichlet64(gamma, alpha)[0] + lm.dirichlet_constant(gamma.shape[0], gamma.shape[1], alpha)


def online(X, gamma0, lam0, alpha, eta, n_batches, n_epochs, doc_iter, kappa, tau0, perm=None):
    """The online algorithm in float64: -> ([(gamma, lambda) after epoch 1, 2, ...], [L_e], [rho_t]); every gamma is the final
    fold (max(doc_iter, 1) gamma-only rounds of every block under the tables of that moment, which leaves the run itself
    untouched), in the caller's order."""
    n, m = X.shape
    order = np.arange(n) if perm is None else np.asarray(perm)
    Xp = X.tocsr()[order]
    gamma = np.asarray(gamma0, np.float64)[order].copy()
    lam = np.asarray(lam0, np.float64).copy()
    ranges = om.row_ranges(Xp.indptr, n_batches)
    blocks = [om.Block(Xp[a:b]) for a, b in ranges]
    t, L, rhos, states = 0, [], [], []
    for e in range(n_epochs):
        Le = 0.0
        for blk, (a, b) in zip(blocks, ranges):
            rho = (tau0 + t) ** (-kappa)
            B = table(lam)
            gamma[a:b], acc = rounds(blk, gamma[a:b], B, alpha, doc_iter)
            Le += bound_partial(blk, gamma[a:b], B, alpha)
            lam = (1.0 - rho) * lam + rho * (eta + (n / (b - a)) * acc.T)
            rhos.append(rho)
            t += 1
        L.append(Le)
        B = table(lam)
        folded = np.empty_like(gamma)
        for blk, (a, b) in zip(blocks, ranges):
            folded[order[a:b]] = rounds(blk, gamma[a:b], B, alpha, max(doc_iter, 1))[0]
        states.append((folded, lam.copy()))
    return states, L, rhos


def batch(X, gamma0, lam0, alpha, eta, n_iter):
    """batch LDA, doc_iter = 1: both updates of an iteration from the same responsibilities"""
    blk = om.Block(X.tocsr())
    gamma, lam = np.asarray(gamma0, np.float64), np.asarray(lam0, np.float64)
    for _ in range(n_iter):
        gamma, acc = rounds(blk, gamma, table(lam), alpha, 1)
        lam = eta + acc.T
    return gamma, lam


def perplexity(held, scored, gamma, lam):
    gamma, lam = np.asarray(gamma, np.float64), np.asarray(lam, np.float64)
    return om.perplexity(held, scored, gamma / gamma.sum(1, keepdims=True), lam / lam.sum(1, keepdims=True))


def the_permutation():
    """what lda_fit_online draws from random_state = FIT["random_state"] when the start is handed to it (init draws nothing)"""
    return np.random.RandomState(FIT["random_state"]).permutation(om.CORPUS["n"])


@functools.lru_cache(maxsize=None)
def model(doc_iter=FIT["doc_iter"], tau0=FIT["tau0"]):
    """dict: `perm`, `online_perplexity` (after 1 .. max_epochs epochs), `L` (per epoch), `rho`"""
    observed, held, scored, gamma0, lam0 = the_split()
    perm = the_permutation()
    states, L, rhos = online(observed, gamma0, lam0, FIT["alpha"], FIT["eta"], FIT["n_batches"], FIT["max_epochs"], doc_iter,
                             FIT["kappa"], tau0, perm)
    return dict(perm=perm, online_perplexity=[perplexity(held, scored, g, l) for g, l in states], L=L, rho=rhos)


@functools.lru_cache(maxsize=None)
def batch_perplexity(n_iter=FIT["batch_iterations"]):
    observed, held, scored, gamma0, lam0 = the_split()
    return perplexity(held, scored, *batch(observed, gamma0, lam0, FIT["alpha"], FIT["eta"], n_iter))
