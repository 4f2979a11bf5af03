"""Shared by tests/test_smoothed_model_host.py and tests/test_smoothed_em.py (not a test module): a float64 restatement of one
smoothed (MAP) EM step and of its objective on top of test_pass_matrix.step64, and the planted corpus of the end-to-end checks.

    n_dz = sum_w x_dw P(z|w,d)              N_d = sum_z n_dz        (unweighted)
    n_wz = sum_d sw_d x_dw P(z|w,d)         N_z = sum_w n_wz        (weighted)
    P(z|d) = (n_dz + a) / (N_d + k a)       P(w|z) = (n_wz + b) / (N_z + m b)
    F = sum sw_d x_dw log sum_z P(w|z) P(z|d)  +  a sum_d sw_d sum_z log P(z|d)  +  b sum_z sum_w log P(w|z)

step64 returns the normalised factors and their norms; the expected counts are their products, formed here in float64.
"""
import functools

import numpy as np
import scipy.sparse as sp

from test_pass_matrix import step64

PLANTED = dict(n=1280, train=640, m=480, topics=8, tokens=40, topic_alpha=0.05, doc_alpha=0.2)
PLANTED_SEED = 3          # test_smoothed_model_host.py: the smallest increase of F over 30 iterations is > 10 x its bound


def smoothed_step64(X, U, V, thresh, a, b, sw=None, update_v=True):
    """One smoothed EM step from (U, V) on X in float64 after step64's float32 products.  Returns step64's dict with U and
    V replaced by the MAP updates (V untouched when update_v is False: the refit), the plain ones kept as U_plain, V_plain."""
    return smooth_step(step64(X, U, V, thresh, sw), V, a, b, update_v)


def smooth_step(s, V, a, b, update_v=True):
    """the pseudo-counts applied to a plain step `s` (step64's dict) that started from the topics V [k, m]"""
    k, m = np.asarray(V).shape
    n_dz = s["U"] * s["norm_pdz"][:, None]
    out = dict(s, U_plain=s["U"], V_plain=s["V"])
    out["U"] = (n_dz + a) / (s["norm_pdz"][:, None] + k * a) if a > 0 else s["U"]
    if not update_v:
        out["V"] = np.asarray(V, np.float64)
    elif b > 0:
        n_wz = s["V"] * s["norm_pwz"][:, None]
        out["V"] = (n_wz + b) / (s["norm_pwz"][:, None] + m * b)
    return out


def log_prior64(U, V, a, b, sw=None):
    """(prior, sum of |terms|): a sum_d sw_d sum_z log P(z|d) + b sum_z sum_w log P(w|z) of float32 factors, float64; an
    entry equal to 0 adds nothing"""
    total, scale = 0.0, 0.0
    for T, coef, w in ((np.asarray(U, np.float32), a, sw), (np.asarray(V, np.float32).T, b, None)):
        if coef <= 0:
            continue
        T = T.astype(np.float64)
        lg = np.log(np.where(T > 0, T, 1.0))
        rows = coef * (np.ones(T.shape[0]) if w is None else np.asarray(w, np.float64))
        terms = rows[:, None] * lg
        total += float(terms.sum())
        scale += float(np.abs(terms).sum())
    return total, scale


def objective64(X, U, V, a, b, sw=None):
    """(F, likelihood error scale, sum of |prior terms|) of float32 factors"""
    s = step64(X, U, V, 1e-32, sw)
    prior, scale = log_prior64(U, V, a, b, sw)
    return s["ll"] + prior, s["ll_scale"], scale


@functools.lru_cache(maxsize=None)
def planted(seed=PLANTED_SEED):
    """(X_train, X_test, sw, U0, V0): topics Dirichlet(0.05) over 480 words, document mixtures Dirichlet(0.2) over 8 topics,
    1 280 documents of 40 tokens, the first 640 train; weights in (0.5, 1.5) and a positive random start for k = 8"""
    p = PLANTED
    rs = np.random.RandomState(seed)
    T = rs.dirichlet(np.full(p["m"], p["topic_alpha"]), size=p["topics"])
    theta = rs.dirichlet(np.full(p["topics"], p["doc_alpha"]), size=p["n"])
    P = theta @ T
    P /= P.sum(1, keepdims=True)
    X = sp.csr_matrix(np.stack([rs.multinomial(p["tokens"], P[d]) for d in range(p["n"])]).astype(np.float32))
    sw = (0.5 + rs.rand(p["train"])).astype(np.float32)
    k = p["topics"]
    U = rs.rand(p["train"], k) + 0.05
    V = rs.rand(k, p["m"]) + 0.05
    U0 = (U / U.sum(1, keepdims=True)).astype(np.float32)
    V0 = (V / V.sum(1, keepdims=True)).astype(np.float32)
    return X[:p["train"]].tocsr(), X[p["train"]:].tocsr(), sw, U0, V0


@functools.lru_cache(maxsize=None)
def planted_trace(a=0.1, b=0.01, iterations=30, seed=PLANTED_SEED):
    """F after 0 .. `iterations` smoothed steps of the model on the training half (the factors rounded to float32 after every
    step, as the device holds them), with check_ll's error scale of every F"""
    X, _, sw, U, V = planted(seed)
    F, scales = [], []
    for i in range(iterations + 1):
        f, ll_scale, _ = objective64(X, U, V, a, b, sw)
        F.append(f)
        scales.append(ll_scale)
        if i < iterations:
            s = smoothed_step64(X, U, V, 1e-32, a, b, sw)
            U, V = s["U"].astype(np.float32), s["V"].astype(np.float32)
    return np.array(F), np.array(scales)
