"""Shared by tests/test_lda_model_host.py and tests/test_lda_em.py (not a test module): a float64 restatement of one iteration of
variational Bayes LDA, of its exp-digamma tables and of its bound on top of test_pass_matrix.step64, and the planted corpus of
the end-to-end checks.

    A_dz = exp(psi(gamma_dz) - psi(S_d)), S_d = sum_z gamma_dz        B_zw = exp(psi(lambda_zw) - psi(S_z)), S_z = sum_w lambda_zw
    phi_dwz = A_dz B_zw / sum_z' A_dz' B_z'w
    gamma_dz = alpha + sum_w x_dw phi_dwz                             lambda_zw = eta + sum_d x_dw phi_dwz
    L = sum x_dw log sum_z A_dz B_zw
      + sum_d [lgamma(k alpha) - k lgamma(alpha) - lgamma(S_d) + sum_z (lgamma gamma_dz + (alpha - gamma_dz)(psi(gamma_dz) - psi(S_d)))]
      + sum_z [lgamma(m eta) - m lgamma(eta) - lgamma(S_z) + sum_w (lgamma lambda_zw + (eta - lambda_zw)(psi(lambda_zw) - psi(S_z)))]

The state is taken as float32 (what the device holds) and everything is formed from it in float64; the tables are scaled (every
document's row of A and every word's column of B to a largest entry of 1, which phi does not see) and rounded to float32
before step64 multiplies them, as the device scales and rounds them before the passes do.  step64 returns normalised factors and
their norms; the expected counts are their products.
"""
import functools

import numpy as np
from scipy.special import gammaln, psi

import smoothed_model as sm
from test_pass_matrix import loglik64, step64, _coo

PRIORS = (0.1, 0.01)      # (alpha, eta) of the planted checks: the sparse regime MAP EM cannot express


def state64(gamma, lam):
    return np.asarray(gamma, np.float32).astype(np.float64), np.asarray(lam, np.float32).astype(np.float64)


def tables64(gamma, lam):
    """(A [n, k], B [k, m]) in float64 from the float32 state"""
    g, l = state64(gamma, lam)
    return np.exp(psi(g) - psi(g.sum(1, keepdims=True))), np.exp(psi(l) - psi(l.sum(1, keepdims=True)))


def scaled_tables64(gamma, lam):
    """(A', B', shift_d [n], shift_w [m]): the tables the passes run on.  Every document's row of A and every word's column of
    B is divided by its largest entry, exp(shift): the responsibilities do not change, the largest entry of every such row is
    1, and sum_z A B = exp(shift_d + shift_w) sum_z A' B'."""
    g, l = state64(gamma, lam)
    log_a = psi(g) - psi(g.sum(1, keepdims=True))
    log_b = psi(l) - psi(l.sum(1, keepdims=True))
    shift_d, shift_w = log_a.max(1), log_b.max(0)
    return np.exp(log_a - shift_d[:, None]), np.exp(log_b - shift_w[None, :]), shift_d, shift_w


def lda_step64(X, gamma, lam, alpha, eta, thresh=1e-32, update_v=True):
    """One iteration from (gamma, lam) on X.  Returns step64's dict of the step on the float32 scaled tables with gamma, lam
    added (lam untouched when update_v is False: a gamma-only round)."""
    A, B, _, _ = scaled_tables64(gamma, lam)
    s = step64(X, A.astype(np.float32), B.astype(np.float32), thresh, None)
    out = dict(s, A=A, B=B)
    out["gamma"] = alpha + s["U"] * s["norm_pdz"][:, None]
    out["lam"] = eta + s["V"] * s["norm_pwz"][:, None] if update_v else state64(gamma, lam)[1]
    return out


def dirichlet64(T, prior):
    """(sum, sum of |terms|) of the Dirichlet part of the bound of the rows of T (float64 [rows, size]) without its constants:
    per entry lgamma(x) + (prior - x)(psi(x) - psi(S)), per row -lgamma(S)"""
    S = T.sum(1, keepdims=True)
    entries = gammaln(T) + (prior - T) * (psi(T) - psi(S))
    rows = -gammaln(S)
    return float(entries.sum() + rows.sum()), float(np.abs(entries).sum() + np.abs(rows).sum())


def dirichlet_constant(rows, size, prior):
    return rows * (gammaln(size * prior) - size * gammaln(prior))


def constant_scale(rows, size, prior):
    """the magnitudes the constant is formed from (it is computed once, in float64, on either side)"""
    return rows * (abs(gammaln(size * prior)) + size * abs(gammaln(prior)))


def bound64(X, gamma, lam, alpha, eta=None, round_tables=True):
    """(L, likelihood error scale, sum of |float64 terms|: the Dirichlet terms, the constants' parts, the shifts) of the float32
    state; eta None: without the topic part.
    round_tables: the likelihood term as the device forms it, on the float32 scaled tables plus sum x (shift_d + shift_w), a
    float64 sum (False: on the float64 tables of the definition)."""
    g, l = state64(gamma, lam)
    rows, cols, x = _coo(X)
    shift_scale = 0.0
    if round_tables:
        A, B, shift_d, shift_w = scaled_tables64(gamma, lam)
        ll, ll_scale = loglik64(rows, cols, x, A.astype(np.float32), B.astype(np.float32))
        shifts = x.astype(np.float64) * (shift_d[rows] + shift_w[cols])
        ll += float(shifts.sum())
        shift_scale = float(np.abs(shifts).sum())
    else:
        A, B = tables64(gamma, lam)
        dot = np.einsum("jz,zj->j", A[rows], B[:, cols])
        live = x > 0
        ll, ll_scale = float((x[live] * np.log(dot[live])).sum()), float((x[live] * np.maximum(1, np.abs(np.log(dot[live])))).sum())
    n, k = g.shape
    m = l.shape[1]
    part, scale = dirichlet64(g, alpha)
    total = ll + part + dirichlet_constant(n, k, alpha)
    scale += constant_scale(n, k, alpha) + shift_scale
    if eta is not None:
        part_v, scale_v = dirichlet64(l, eta)
        total += part_v + dirichlet_constant(k, m, eta)
        scale += scale_v + constant_scale(k, m, eta)
    return total, ll_scale, scale


@functools.lru_cache(maxsize=None)
def planted(seed=sm.PLANTED_SEED):
    """(X_train, X_test, gamma0, lam0): the planted corpus of smoothed_model.py (640 + 640 documents of 40 tokens over 480 words,
    8 topics) and a positive random float32 start for k = 8"""
    X, X_test, _, _, _ = sm.planted(seed)
    k = sm.PLANTED["topics"]
    rs = np.random.RandomState(seed + 100)
    gamma0 = rs.gamma(100.0, 0.01, (X.shape[0], k)).astype(np.float32)
    lam0 = rs.gamma(100.0, 0.01, (k, X.shape[1])).astype(np.float32)
    return X, X_test, gamma0, lam0


@functools.lru_cache(maxsize=None)
def planted_trace(alpha=PRIORS[0], eta=PRIORS[1], iterations=30, seed=sm.PLANTED_SEED):
    """L after 0 .. `iterations` steps of the model on the training half (the state rounded to float32 after every step, as
    the device holds it), with the likelihood error scale and the sum of |Dirichlet terms| of every L"""
    X, _, gamma, lam = planted(seed)
    L, ll_scales, scales = [], [], []
    for i in range(iterations + 1):
        f, ll_scale, scale = bound64(X, gamma, lam, alpha, eta)
        L.append(f)
        ll_scales.append(ll_scale)
        scales.append(scale)
        if i < iterations:
            s = lda_step64(X, gamma, lam, alpha, eta)
            gamma, lam = s["gamma"].astype(np.float32), s["lam"].astype(np.float32)
    return np.array(L), np.array(ll_scales), np.array(scales)


def monotone_bound(k, tokens, ll_scale, scale, L):
    """what a float32 trace value of the device may differ from the model's L by: check_ll's bound of the likelihood term, the
    tables' 3 u reaching every log dot twice (A and B), 2^-50 of the Dirichlet terms, the float32 rounding of the trace"""
    u = 2.0 ** -24
    return 4.0 * (k + 1) * u * ll_scale + 2 * 3 * u * tokens + 2.0 ** -50 * scale + abs(L) * u


# ------------------------------------------------------------------------------------------------
# the scheme in plain float64 (dense, small corpora): what the device's iteration approximates
# ------------------------------------------------------------------------------------------------
def exact_tables(gamma, lam):
    return np.exp(psi(gamma) - psi(gamma.sum(1, keepdims=True))), np.exp(psi(lam) - psi(lam.sum(1, keepdims=True)))


def exact_step(Xd, gamma, lam, alpha, eta):
    """one iteration on the dense count matrix Xd from a float64 state: both updates from the same responsibilities"""
    A, B = exact_tables(gamma, lam)
    dot = A @ B
    R = np.divide(Xd, dot, out=np.zeros_like(dot), where=Xd > 0)
    return alpha + A * (R @ B.T), eta + B * (A.T @ R)


def exact_bound(Xd, gamma, lam, alpha, eta):
    """(L, sum of |terms|) in float64"""
    A, B = exact_tables(gamma, lam)
    terms = Xd * np.log(np.where(Xd > 0, A @ B, 1.0))
    n, k = gamma.shape
    m = lam.shape[1]
    part_u, scale_u = dirichlet64(gamma, alpha)
    part_v, scale_v = dirichlet64(lam, eta)
    total = float(terms.sum()) + part_u + part_v + dirichlet_constant(n, k, alpha) + dirichlet_constant(k, m, eta)
    return total, float(np.abs(terms).sum()) + scale_u + scale_v


@functools.lru_cache(maxsize=None)
def small_planted(seed=5, n=96, m=80, k=4, tokens=30):
    """dense counts [n, m] of a planted corpus small enough for scikit-learn's batch fit to run in a test"""
    rs = np.random.RandomState(seed)
    T = rs.dirichlet(np.full(m, 0.1), size=k)
    theta = rs.dirichlet(np.full(k, 0.3), size=n)
    return np.stack([rs.multinomial(tokens, theta[d] @ T) for d in range(n)]).astype(np.float64)
