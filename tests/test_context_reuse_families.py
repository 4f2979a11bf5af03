"""A reused engine context computes what a fresh one computes: the fit families that came after tests/test_context_reuse.py.

    Whatever a context has done before, an operation on it returns exactly the bits that the same operation returns on
    a context created for it alone.  The fresh result itself stays within the float64 bounds its family's suite derives.

test_context_reuse.py walks plain pLSA, the metric kernels, topic combination and member batches.  Since then the context
(csrc/plsa_hip.hip: plsa_ctx) has grown state that no Derived<T> guards: the tempered side tables and the snapshot slot with
its hand-kept shape (Tempered), the smoothed scratch (Smoothed), the exp-digamma tables with two hand-kept validity flags and
ONE grow-only buffer of float64 side arrays whose six regions sit at offsets computed from the n and kp of the moment (Lda:
lda_sums()), a page-locked slot that is grow-only in kp (LdaPrior), the scratch of score_rows and NMF, and the online states,
which stage their host copies through the home context's tmp0, put their V or B into a block context's slots (StandIn) and, for
LDA, copy their side arrays into the tail of the block's lda.sums at offset 3 n.  Each family's own suite starts from a fresh
Engine for nearly every check.  The product does not: get_engine() hands one process-wide context to every estimator.

Three kinds of check, on the corpora, topic counts and helpers of test_context_reuse.py (A, B, C, A', D; K_WALK = 6, 60, 64, 130):

* the walk: a seeded sequence of state changes and operations (build_segments), every operation compared bit for bit with the
  same operation on a fresh `with Engine()` that holds only its corpus, topic count and start (Baselines).  The walk is cut
  into N_SEGMENTS segments, each on an Engine of its own and each a GPU test of its own; facts are computed per segment and
  united, so a pair of operations counts only inside one segment.  REQUIRED is the list of transitions the union must
  contain (test_family_walk_reaches_every_transition, CPU).
  The rule for ("k", a, b, family): the FULL one.  For every ordered pair (a, b) of distinct topic counts and EVERY family of
  K_FAMILIES (lda, prior, tempered, lda_online) the walk changes k from a to b on an unchanged upload and runs that family
  next: 48 facts, from one Euler circuit over the twelve pairs per family, each circuit on another corpus (A, B, C, A').  No
  family is spread thinner than that, so each sees every k as source and as target three times.
* directed cases, one test each: a block context reused over blocks of different size under one online state (the path
  partial_fit takes), the snapshot slot against a shape that moved, the learned-prior scratch across kp, the process-wide
  engine behind the estimators, and lda_bound after set_factors on an unchanged shape (the validity flags alone).
* anchors: the bit comparisons do not say that the fresh result is right, so for every (corpus, k) a fresh context's
  one-iteration LDA step and bound, smoothed step, tempered tables and step and score_rows are held to float64 with the
  bounds of test_lda_em (step_bounds, check_bound), test_smoothed_em (bounds), test_tempered_em (1 ulp; the bits of
  ordinary_step_on) and test_score_rows (restate, check_rows).  No tolerance is new.

Operations (each sets its own start; fits run n_iter=4, n_iter_per_test=2, tolerance=0, PLSA_FUSED, traced): OPS below.  The LDA
start is test_lda_em.start's: gamma0 = alpha + 20 U0, lambda0 = eta + 50 V0 at (alpha, eta) = (0.1, 0.05); `prior` starts from the
"decreasing" vector of test_lda_priors.  The online states are created inside their operation on the walked engine, which
serves as home AND as block context, and closed before it returns.

Needs a real MI355X except for the tests without the gpu mark.  Measured wall time of `pytest -m gpu` on one MI355X, both in one
session on the same machine, pytest's own totals (imports and the float64 models included): this module 8.7 s for its 43 GPU
tests (490 walk steps in 12 segments, 298 operations; the slowest segment 0.63 s, the slowest test 1.6 s with the library's
first load in it), tests/test_context_reuse.py 4.0 s for its 10 (its walk: 1.5 s).  No segment takes as long as the old walk.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import lda_model as lm
import smoothed_model as sm
import test_lda_em as le
import test_score_rows as sr
import test_smoothed_em as se
import test_tempered_em as te
from test_context_reuse import (K_WALK, OPS as OLD_OPS, SHRINKING, THRESH, _euler_circuit, _history, _seed, assert_same, base_of,
                                bootstrap_idx, corpus, data, hold)
from test_lda_priors import vector
from test_pass_matrix import _bits, check

PLSA_FUSED = le.PLSA_FUSED
ALPHA, ETA = 0.1, 0.05
BETA = 0.9
SMOOTH_A, SMOOTH_B = 0.5, 0.05
FIT = dict(n_iter=4, n_iter_per_test=2, tolerance=0.0, flags=PLSA_FUSED, trace=True)
CORPORA = ("A", "B", "C", "A'", "D")


# ------------------------------------------------------------------------------------------------
# starts (host only)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lda_start(name, k):
    """test_lda_em.start on the walk's factors: (gamma0, lambda0)"""
    D = data(name, k)
    out = (np.float32(ALPHA) + 20 * D.U0).astype(np.float32), (np.float32(ETA) + 50 * D.V0).astype(np.float32)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def prior_start(name, k):
    """test_lda_priors.start with the "decreasing" vector: (alpha float64 [k], gamma0, lambda0)"""
    D = data(name, k)
    alpha = vector("decreasing", k)
    out = (alpha, (alpha.astype(np.float32)[None, :] + 20 * D.U0).astype(np.float32),
           (np.float32(ETA) + 50 * D.V0).astype(np.float32))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def other_factors(name, k, what="other"):
    """seeded factors of the shape of data(name, k), different from them"""
    n, m = corpus(name).shape
    rs = np.random.RandomState(_seed(what, name, k))
    U = rs.rand(n, k) + 0.05
    V = rs.rand(k, m) + 0.05
    out = (U / U.sum(1, keepdims=True)).astype(np.float32), (V / V.sum(1, keepdims=True)).astype(np.float32)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rolled(name):
    """the corpus with its rows rolled by one: the same shape, another pattern"""
    X = corpus(name).tocsr()
    return sp.vstack([X[-1:], X[:-1]]).tocsr()


# ------------------------------------------------------------------------------------------------
# operations: an engine that holds (corpus, k) -> a dict of arrays and scalars
# ------------------------------------------------------------------------------------------------
def _weights(D, arg):
    """arg: "sw" the weights are passed, "none" no weights, "resident" none passed while resident ones apply, "-" the
    operation takes none"""
    return D.sw if arg == "sw" else None


def _factors(eng, **more):
    U, V = eng.get_factors()
    return dict(U=U, V=V, **more)


def op_tempered(amd, eng, D, arg):
    eng.set_factors(D.U0, D.V0)
    iters, trace = eng.fit_tempered(BETA, _weights(D, arg), **FIT)
    return _factors(eng, iters=int(iters), trace=trace)


def op_temper(amd, eng, D, arg):
    eng.set_factors(D.U0, D.V0)
    TU, TV = eng.temper_factors(BETA)
    return dict(TU=TU, TV=TV)


def op_snap(amd, eng, D, arg):
    eng.set_factors(D.U0, D.V0)
    eng.snapshot_factors()
    eng.set_factors(*other_factors(D.name, D.k))
    eng.em_accumulate(None, THRESH)
    eng.em_finish()
    eng.restore_factors()
    out = _factors(eng)
    assert np.array_equal(_bits(out["U"]), _bits(D.U0)) and np.array_equal(_bits(out["V"]), _bits(D.V0)), \
        "restore_factors did not return the snapshot on %s at k=%d" % (D.name, D.k)
    return out


def op_smoothed(amd, eng, D, arg):
    eng.set_factors(D.U0, D.V0)
    iters, trace = eng.fit_smoothed(SMOOTH_A, SMOOTH_B, _weights(D, arg), **FIT)
    return _factors(eng, iters=int(iters), trace=trace)


def op_resmoothed(amd, eng, D, arg):
    eng.set_factors(D.U0, D.V0)
    iters, trace = eng.refit_smoothed(SMOOTH_A, _weights(D, arg), **FIT)
    return _factors(eng, iters=int(iters), trace=trace)


def op_posterior(amd, eng, D, arg):
    eng.set_factors(D.U0, D.V0)
    return dict(F=eng.log_posterior(_weights(D, arg), SMOOTH_A, SMOOTH_B))


def op_lda(amd, eng, D, arg):
    eng.set_factors(*lda_start(D.name, D.k))
    iters, trace = eng.lda_fit(ALPHA, ETA, doc_iter=2, **FIT)
    return _factors(eng, iters=int(iters), trace=trace)


def op_lda_refit(amd, eng, D, arg):
    eng.set_factors(*lda_start(D.name, D.k))
    iters, trace = eng.lda_refit(ALPHA, doc_iter=2, **FIT)
    return _factors(eng, iters=int(iters), trace=trace)


def op_lda_bound(amd, eng, D, arg):
    eng.set_factors(*lda_start(D.name, D.k))
    return dict(L=eng.lda_bound(ALPHA, ETA), L_documents=eng.lda_bound(ALPHA))


def op_lda_tables(amd, eng, D, arg):
    eng.set_factors(*lda_start(D.name, D.k))
    A, B = eng.lda_tables()
    return dict(A=A, B=B)


def op_prior(amd, eng, D, arg):
    alpha0, gamma0, lam0 = prior_start(D.name, D.k)
    eng.set_factors(gamma0, lam0)
    iters, trace, alpha, eta = eng.lda_prior_fit(alpha0, ETA, learn=3, prior_start=1, prior_every=1, **FIT)
    assert alpha.shape == (D.k,), alpha.shape
    t_doc, t_topic = eng.lda_prior_stats()
    assert t_doc.shape == t_topic.shape == (D.k,)
    return _factors(eng, iters=int(iters), trace=trace, alpha=alpha, eta=float(eta), t_doc=t_doc, t_topic=t_topic)


def op_prior_bound(amd, eng, D, arg):
    alpha0, gamma0, lam0 = prior_start(D.name, D.k)
    eng.set_factors(gamma0, lam0)
    return dict(L=eng.lda_prior_bound(alpha0, ETA), L_documents=eng.lda_prior_bound(alpha0))


def op_score(amd, eng, D, arg):
    eng.set_factors(D.U0, D.V0)
    sw = _weights(D, arg)
    out = dict(zip(("ll", "tokens", "unscored"), eng.score_rows(None, sw)))
    out.update(zip(("other_ll", "other_tokens", "other_unscored"), eng.score_rows(rolled(D.name), sw)))
    return out


def op_nmf(amd, eng, D, arg):
    n, m = D.X.shape
    rs = np.random.RandomState(_seed("nmf", D.name, D.k))
    W0, H0 = (rs.rand(n, D.k) + 0.1).astype(np.float32), (rs.rand(D.k, m) + 0.1).astype(np.float32)
    eng.nmf_set_factors(W0, H0)
    iters, errors = eng.nmf_fit(max_iter=3, tol=0)
    W, H = eng.nmf_get_factors()
    return dict(iters=int(iters), errors=errors, W=W, H=H, divergence=eng.nmf_divergence())


def op_online(amd, eng, D, arg):
    m = D.X.shape[1]
    with amd.OnlineState(eng, m, D.k) as st:
        st.set_topics(D.V0)
        eng.set_factors(D.U0, D.V0)
        ll = st.step(eng, rho=0.5, scale=2.0, inner_iter=2, want_ll=True, flags=PLSA_FUSED)
        V, S, steps = st.get_topics(), st.statistic_get(), st.steps
    return dict(ll=ll, V=V, S=S, steps=int(steps), U=eng.get_factors(want_v=False)[0])


def op_lda_online(amd, eng, D, arg):
    m = D.X.shape[1]
    gamma0, lam0 = lda_start(D.name, D.k)
    with amd.LdaOnlineState(eng, m, D.k) as st:
        st.set_lambda(lam0)
        eng.set_factors(gamma0, lam0)
        bound = st.step(eng, ALPHA, ETA, rho=0.5, scale=2.0, doc_iter=2, want_bound=True, flags=PLSA_FUSED)
        lam, steps = st.get_lambda(), st.steps
    return dict(bound=bound, lam=lam, steps=int(steps), gamma=eng.get_factors(want_v=False)[0])


def _old(name):
    def op(amd, eng, D, arg):
        eng.set_factors(D.U0, D.V0)
        return OLD_OPS[name](amd, eng, D, arg)
    op.__name__ = "op_" + name
    return op


NEIGHBOURS = ("step", "fit_fused", "codoc", "hellinger", "members")          # of the old walk
OPS = dict(tempered=op_tempered, temper=op_temper, snap=op_snap, smoothed=op_smoothed, resmoothed=op_resmoothed,
           posterior=op_posterior, lda=op_lda, lda_refit=op_lda_refit, lda_bound=op_lda_bound, lda_tables=op_lda_tables,
           prior=op_prior, prior_bound=op_prior_bound, score=op_score, nmf=op_nmf, online=op_online, lda_online=op_lda_online,
           **{name: _old(name) for name in NEIGHBOURS})
WEIGHTED_OPS = ("tempered", "smoothed", "resmoothed", "posterior", "score", "fit_fused")     # take "sw" / "none" / "resident"
FAMILIES = ("step", "tempered", "smoothed", "lda", "prior", "nmf", "online", "lda_online", "score")
K_FAMILIES = ("lda", "prior", "tempered", "lda_online")
READERS = ("lda_bound", "lda_tables", "prior_bound", "score", "posterior", "temper")    # read side buffers, no fit in front
WRITERS = ("prior", "tempered", "smoothed", "score")                                    # fill them before the corpus changes
GROWING = (("B", "C"), ("A", "C"), ("B", "A"))
CORPUS_CHANGES = tuple(SHRINKING) + GROWING
MOVED_OPS = ("lda", "smoothed", "tempered", "score")                                    # behind bootstrap and a second upload
D_OPS = ("lda", "tempered", "smoothed")
RESIDENT_OPS = ("tempered", "smoothed", "score")
FAILS = dict(tempered_beta="tempered", lda_alpha="lda", lda_reference="lda", restore_none="snap", prior_length="prior")


def run_op(amd, eng, name, k, op, arg):
    out = OPS[op](amd, eng, data(name, k), arg)
    assert out, "%s returned nothing" % op
    return out


def baseline_key(name, k, op, arg):
    """the memo key of a baseline: resident weights are the same weights passed, nothing else shares a key"""
    assert name in CORPORA and k in K_WALK and op in OPS, (name, k, op)
    assert arg in (("sw", "none", "resident") if op in WEIGHTED_OPS else ("-",)), (op, arg)
    return (name, int(k), op, "sw" if arg == "resident" else arg)


class Baselines:
    """the same operation on a fresh `with Engine()` that holds only that corpus, k and start; memoised"""

    def __init__(self, amd):
        self.amd = amd
        self.memo = {}

    def get(self, name, k, op, arg):
        key = baseline_key(name, k, op, arg)
        if key not in self.memo:
            with self.amd.Engine() as eng:
                hold(eng, name)
                assert eng.shape[:2] == corpus(name).shape
                out = run_op(self.amd, eng, name, k, op, key[3])
            self.memo[key] = (corpus(name).shape + (k,), out)
        shape, out = self.memo[key]
        assert shape == corpus(name).shape + (k,), (key, shape)             # a key never aliases across k or corpus
        return out


# ------------------------------------------------------------------------------------------------
# the walk: seeded segments of state changes and operations
# ------------------------------------------------------------------------------------------------
# steps: ("upload", corpus) ("bootstrap", "idx" | None) ("setk", k) ("release",) ("set_sw", bool) ("fail", kind)   -- state changes
#        ("op", name, arg)                                                                                          -- operations
ARRIVAL_WINDOW = len(READERS)

REQUIRED = (
    # every ordered pair of distinct families as consecutive operations with no upload between them
    [("pair", a, b) for a in FAMILIES for b in FAMILIES if a != b] +
    # every ordered pair of distinct topic counts on an unchanged upload, followed by every family of K_FAMILIES
    [("k", a, b, op) for a in K_WALK for b in K_WALK if a != b for op in K_FAMILIES] +
    # the shrinking and the growing corpus changes, followed by the calls that read side buffers without a fit in front
    [("corpus", a, b, op) for a, b in CORPUS_CHANGES for op in READERS] +
    # release_scratch followed by every operation of this module
    [("after", "release", op) for op in OPS] +
    # a bootstrap resample, and the base uploaded again behind it
    [("after", "bootstrap", op) for op in MOVED_OPS] + [("reupload", "A'", "A", op) for op in MOVED_OPS] +
    [("after", "restore", "step")] +
    # the row-item corpus under every topic count's document pass, entered and left at an unchanged topic count
    [("at", "D", k, op) for k in K_WALK for op in D_OPS] +
    [("arrive_same_k", "D", k) for k in K_WALK] + [("leave_same_k", "D", k) for k in K_WALK] +
    # resident weights: the weighted calls with none passed; LDA takes none and ignores them
    [("after", "set_sw:on", op + ":resident") for op in RESIDENT_OPS] + [("after", "set_sw:on", "lda"), ("after", "set_sw:off", "step")] +
    # a refusal that launches nothing, then step and the family's own operation
    [("after", "fail:" + kind, op) for kind, family in FAILS.items() for op in ("step", family)] +
    # every operation; the weighted ones with and without weights
    [("op", name) for name in OPS] + [("op", name, arg) for name in WEIGHTED_OPS for arg in ("sw", "none")]
)


def walk_facts(steps):
    """the transitions ONE segment contains: two operations are a pair when no upload or bootstrap lies between them"""
    facts = set()
    cur, k = None, None
    prev = None                     # (op, arg, corpus, k) of the last operation
    changes = []                    # state changes since it
    arrival = None                  # [from, to, operations seen since] of the last corpus change
    for s in steps:
        if s[0] != "op":
            changes.append(s)
            if s[0] == "upload":
                cur = s[1]
            elif s[0] == "bootstrap":
                assert base_of(cur) == "A", "the walk bootstraps A only"
                cur = "A'" if s[1] else "A"
            elif s[0] == "setk":
                k = s[1]
            continue
        _, name, arg = s
        assert cur is not None and k is not None, "operation before a corpus and a topic count"
        facts.add(("op", name))
        facts.add(("op", name, arg))
        facts.add(("at", cur, k, name))
        moved = any(c[0] in ("upload", "bootstrap") for c in changes)
        same_k = prev is not None and prev[3] == k and not any(c[0] == "setk" and c[1] != k for c in changes)
        if prev is not None and prev[2] != cur:
            arrival = [prev[2], cur, 0]
            if same_k and cur == "D":
                facts.add(("arrive_same_k", "D", k))
            if same_k and prev[2] == "D":
                facts.add(("leave_same_k", "D", k))
        elif moved:
            arrival = None
        if arrival is not None and arrival[2] < ARRIVAL_WINDOW:
            facts.add(("corpus", arrival[0], arrival[1], name))
            arrival[2] += 1
        if prev is not None and prev[2] == "A'" and cur == "A" and ("upload", "A") in changes:
            facts.add(("reupload", "A'", "A", name))
        if prev is not None and not moved:
            facts.add(("pair", prev[0], name))
            if prev[3] != k:
                facts.add(("k", prev[3], k, name))
        for c in changes:
            kind = c[0]
            if kind == "fail":
                kind = "fail:" + c[1]
            elif kind == "set_sw":
                kind = "set_sw:%s" % ("on" if c[1] else "off")
            elif kind == "bootstrap" and not c[1]:
                kind = "restore"
            facts.add(("after", kind, name))
            facts.add(("after", kind, "%s:%s" % (name, arg)))
        prev = (name, arg, cur, k)
        changes = []
    return facts


def united_facts(segments):
    facts = set()
    for steps in segments:
        facts |= walk_facts(steps)
    return facts


class _Segment:
    """one segment under construction: it begins with an upload and a topic count"""

    def __init__(self, rs, name, k):
        self.rs = rs
        self.steps = []
        self.cur = self.k = None
        self.goto(name, k)

    def emit(self, *step):
        self.steps.append(tuple(step))

    def pick_k(self, other_than=None):
        ks = [k for k in K_WALK if k != other_than]
        return ks[self.rs.randint(len(ks))]

    def setk(self, k):
        self.emit("setk", k)
        self.k = k

    def goto(self, name, k=None):
        if name == "A'":
            if self.cur != "A":
                self.emit("upload", "A")
            self.emit("bootstrap", "idx")
        else:
            self.emit("upload", name)
        self.cur = name
        self.setk(self.k if k is None else k)

    def op(self, name, arg=None):
        if arg is None:
            arg = ("sw", "sw", "none")[self.rs.randint(3)] if name in WEIGHTED_OPS else "-"
        self.emit("op", name, arg)

    def ops(self, names, shuffled=True):
        for i in (self.rs.permutation(len(names)) if shuffled else range(len(names))):
            self.op(names[i])


def _pair_segments(rs):
    """an Euler circuit over the 72 ordered pairs of families, cut into three pieces that share their end points, each
    on another corpus; the topic count changes every eighth operation"""
    circuit = _euler_circuit([(a, b) for a in FAMILIES for b in FAMILIES if a != b], FAMILIES[0], rs)
    out = []
    for (lo, hi), (name, k) in zip(((0, 25), (24, 49), (48, 73)), (("A", 60), ("C", 130), ("B", 6))):
        seg = _Segment(rs, name, k)
        for i, family in enumerate(circuit[lo:hi]):
            if i and i % 8 == 0:
                seg.setk(seg.pick_k(other_than=seg.k))
            seg.op(family)
        out.append(seg.steps)
    return out


def _corpus_segments(rs):
    """an Euler circuit over the six changes between A, B and C, cut into two pieces that share a stop: at every stop the
    readers, then the writers (what the next stop's readers must not see)"""
    tour = _euler_circuit(list(CORPUS_CHANGES), "C", rs)
    out = []
    for lo, hi in ((0, 4), (3, 7)):
        seg = _Segment(rs, tour[lo], K_WALK[rs.randint(len(K_WALK))])
        seg.ops(WRITERS)
        for name in tour[lo + 1:hi]:
            seg.goto(name, seg.pick_k())
            seg.ops(READERS)
            seg.ops(WRITERS)
        out.append(seg.steps)
    return out


def _k_segments(rs):
    """one Euler circuit over the twelve ordered pairs of topic counts per family of K_FAMILIES, two circuits to a segment;
    behind every third stop a neighbour of the old walk"""
    out = []
    plan = list(zip(K_FAMILIES, ("A", "B", "C", "A'")))
    for half in (plan[:2], plan[2:]):
        seg = None
        for j, (family, name) in enumerate(half):
            ks = _euler_circuit([(a, b) for a in K_WALK for b in K_WALK if a != b], K_WALK[(j + len(out)) % len(K_WALK)], rs)
            if seg is None:
                seg = _Segment(rs, name, ks[0])
            else:
                seg.goto(name, ks[0])
            seg.op(family)
            for i, k in enumerate(ks[1:]):
                seg.setk(k)
                seg.op(family)
                if i % 3 == 2:
                    seg.op(NEIGHBOURS[rs.randint(len(NEIGHBOURS))])
        out.append(seg.steps)
    return out


def _release_segments(rs):
    """release_scratch in front of every operation of this module, in two segments; something of the LDA families runs
    first, so that there is something to release"""
    names = [list(OPS)[i] for i in rs.permutation(len(OPS))]
    out = []
    for part, (name, k), first in ((names[:11], ("C", 130), "prior"), (names[11:], ("A", 60), "lda_online")):
        seg = _Segment(rs, name, k)
        seg.op(first)
        for i, op in enumerate(part):
            if i == 6:
                seg.goto("B", 6)
            elif i % 4 == 3:
                seg.setk(seg.pick_k(other_than=seg.k))
            seg.emit("release")
            seg.op(op)
        out.append(seg.steps)
    return out


def _moved_segment(rs):
    """bootstrap and a second upload of the base in front of MOVED_OPS, one restore, and the resident weights"""
    seg = _Segment(rs, "A", 60)
    for i, op in enumerate(MOVED_OPS):
        if i == 2:
            seg.setk(130)
        seg.goto("A'")
        seg.op(op)
        seg.goto("A")
        seg.op(op)
    seg.goto("A'")
    seg.op("step")
    seg.emit("bootstrap", None)
    seg.cur = "A"
    seg.setk(seg.k)
    seg.op("step")
    for op in RESIDENT_OPS:
        seg.emit("set_sw", True)
        seg.op(op, "resident")
        seg.emit("set_sw", False)
        seg.op("step")
    seg.emit("set_sw", True)
    seg.op("lda")
    seg.op("tempered", "resident")
    seg.emit("set_sw", False)
    seg.op("smoothed", "none")
    for op in ("resmoothed", "fit_fused", "posterior"):          # (wherever the seeded choice of the other segments fell)
        seg.op(op, "sw")
        seg.op(op, "none")
    return [seg.steps]


def _fail_segment(rs):
    """every refusal, then step; every refusal again, then the family's own operation.  restore_none needs a context
    without a snapshot: release_scratch comes first"""
    seg = _Segment(rs, "A", 64)
    seg.ops(("lda", "tempered", "snap", "prior"))
    for follow_family in (False, True):
        for i in rs.permutation(len(FAILS)):
            kind = list(FAILS)[i]
            if kind == "restore_none":
                seg.emit("release")
            seg.emit("fail", kind)
            seg.op(FAILS[kind] if follow_family else "step")
        if not follow_family:
            seg.goto("B", 6)
            seg.op("snap")
    return [seg.steps]


def _row_item_segment(rs):
    """D, the corpus on row items, entered and left at an unchanged topic count, once per topic count, from A, B, C and A"""
    seg = None
    for k, base in zip(K_WALK, ("A", "B", "C", "A")):
        if seg is None:
            seg = _Segment(rs, base, k)
        else:
            seg.goto(base, k)
        seg.op(D_OPS[rs.randint(len(D_OPS))])
        seg.goto("D")
        seg.ops(D_OPS)
        seg.goto(base)
        seg.op("step")
        seg.op(D_OPS[rs.randint(len(D_OPS))])
    return [seg.steps]


@functools.lru_cache(maxsize=None)
def build_segments(seed=20241):
    rs = np.random.RandomState(seed)
    segments = []
    for part in (_pair_segments, _corpus_segments, _k_segments, _release_segments, _moved_segment, _fail_segment,
                 _row_item_segment):
        segments.extend(tuple(steps) for steps in part(rs))
    return tuple(segments)


N_SEGMENTS = 12
MIN_STEPS, MAX_STEPS = 450, 540          # all segments together; stated after building (the CPU test prints the count)


def test_family_walk_reaches_every_transition():
    """The cap that keeps the walk from hiding a hole: every transition of REQUIRED occurs in a segment."""
    segments = build_segments()
    assert segments == build_segments.__wrapped__(), "the builder is deterministic"
    assert len(segments) == N_SEGMENTS
    facts = united_facts(segments)
    missing = [r for r in REQUIRED if r not in facts]
    assert not missing, missing
    assert len(REQUIRED) == len(set(REQUIRED)) and sum(r[0] == "pair" for r in REQUIRED) == 72
    total = sum(len(steps) for steps in segments)
    n_ops = sum(s[0] == "op" for steps in segments for s in steps)
    assert MIN_STEPS <= total <= MAX_STEPS, total
    assert max(len(steps) for steps in segments) <= 90, [len(steps) for steps in segments]
    for steps in segments:
        assert steps[0][0] == "upload" and "setk" in (steps[1][0], steps[2][0]), steps[:3]
        # resident weights never meet a call that would pass none on purpose, nor another document count
        resident = False
        for s in steps:
            if s[0] == "set_sw":
                resident = s[1]
            assert not (resident and s[0] in ("upload", "bootstrap", "fail", "setk")), s
            assert not (resident and s[0] == "op" and s[2] in ("sw", "none")), s
            assert not (resident and s[0] == "op" and s[1] in ("online", "fit_fused", "step", "members")), s
            assert not (not resident and s[0] == "op" and s[2] == "resident"), s
            assert s[0] != "op" or s[1] in OPS, s
        assert not resident
    print("\nfamily walk: %d segments, %d steps, %d operations, %d distinct transitions; steps per segment %s"
          % (len(segments), total, n_ops, len(facts), [len(steps) for steps in segments]))


def test_baseline_keys_never_alias_across_corpus_or_topic_count():
    """Every (corpus, k, operation, weights) of the walk has a memo key of its own, except that resident weights share the
    key of the same weights passed; a key names its corpus and k."""
    seen = {}
    for steps in build_segments():
        cur = k = None
        for s in steps:
            if s[0] == "upload":
                cur = s[1]
            elif s[0] == "bootstrap":
                cur = "A'" if s[1] else "A"
            elif s[0] == "setk":
                k = s[1]
            elif s[0] == "op":
                key = baseline_key(cur, k, s[1], s[2])
                assert key[:2] == (cur, k)
                want = (cur, k, s[1], "sw" if s[2] == "resident" else s[2])
                assert seen.setdefault(key, want) == want, (key, want, seen[key])
    assert len({key[:2] for key in seen}) >= 16, "the walk visits most (corpus, k)"
    with pytest.raises(AssertionError):
        baseline_key("A", 60, "lda", "sw")                                 # LDA takes no weights
    with pytest.raises(AssertionError):
        baseline_key("A", 61, "lda", "-")


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


@pytest.fixture(scope="module")
def baselines(amd):
    return Baselines(amd)


def fail_on_purpose(amd, eng, name, k, kind):
    """A refusal that launches nothing: the ABI's status code (DeviceError) or the driver's own ValueError."""
    D = data(name, k)
    if kind == "tempered_beta":
        eng.set_factors(D.U0, D.V0)
        with pytest.raises(amd.DeviceError, match="beta"):
            eng.fit_tempered(2.0, None, **FIT)
    elif kind == "lda_alpha":
        eng.set_factors(*lda_start(name, k))
        with pytest.raises(amd.DeviceError, match="alpha"):
            eng.lda_fit(0.0, ETA, **FIT)
    elif kind == "lda_reference":
        eng.set_factors(*lda_start(name, k))
        eng.set_arithmetic("reference")
        try:
            with pytest.raises(amd.DeviceError, match="reference arithmetic"):
                eng.lda_fit(ALPHA, ETA, **FIT)
        finally:
            eng.set_arithmetic(None)
    elif kind == "restore_none":
        with pytest.raises(amd.DeviceError, match="no snapshot"):
            eng.restore_factors()
    elif kind == "prior_length":
        alpha0, gamma0, lam0 = prior_start(name, k)
        eng.set_factors(gamma0, lam0)
        with pytest.raises((amd.DeviceError, ValueError), match="doc_topic_prior|alpha"):
            eng.lda_prior_fit(np.append(alpha0, 0.5), ETA, learn=3, prior_start=1, prior_every=1, **FIT)
    else:
        raise KeyError(kind)


def apply_change(amd, eng, state, s):
    kind = s[0]
    if kind == "upload":
        eng.upload_csr(corpus(s[1]))
        state["corpus"] = s[1]
    elif kind == "bootstrap":
        eng.bootstrap(bootstrap_idx() if s[1] else None)
        state["corpus"] = "A'" if s[1] else "A"
    elif kind == "setk":
        state["k"] = s[1]
        D = data(state["corpus"], s[1])
        eng.set_factors(D.U0, D.V0)
    elif kind == "release":
        eng.release_scratch()
    elif kind == "set_sw":
        eng.set_sample_weight(data(state["corpus"], state["k"]).sw if s[1] else None)
    elif kind == "fail":
        fail_on_purpose(amd, eng, state["corpus"], state["k"], s[1])
    else:
        raise KeyError(s)


def run_segment(amd, baselines, steps):
    state = dict(corpus=None, k=None)
    with amd.Engine() as eng:
        for i, s in enumerate(steps):
            if s[0] != "op":
                apply_change(amd, eng, state, s)
                continue
            _, op, arg = s
            want = baselines.get(state["corpus"], state["k"], op, arg)
            try:
                got = run_op(amd, eng, state["corpus"], state["k"], op, arg)
                assert_same(got, want, "%s(%s) on %s at k=%d" % (op, arg, state["corpus"], state["k"]))
            except (AssertionError, amd.DeviceError) as e:
                raise AssertionError("step %d of the segment differs from a fresh context: %s\nsteps since the last upload:\n%s"
                                     % (i, e, _history(steps, i))) from e


@pytest.mark.gpu
@pytest.mark.parametrize("segment", range(N_SEGMENTS))
def test_family_walk_equals_fresh_contexts(amd, baselines, segment):
    """Every operation of one segment of the walk, on one Engine with everything before it behind it, against a fresh Engine."""
    run_segment(amd, baselines, build_segments()[segment])


@pytest.mark.gpu
def test_lda_bound_follows_set_factors(amd, baselines):
    """lda_bound, set_factors with other factors of the same shape, lda_bound: no buffer changes its size, so only a table
    kept from the first call could make the second differ from a fresh context's."""
    name, k = "A", 60
    gamma1, lam1 = other_factors(name, k, "other lda state")
    gamma1, lam1 = (np.float32(ALPHA) + 20 * gamma1).astype(np.float32), (np.float32(ETA) + 50 * lam1).astype(np.float32)

    def second(eng):
        eng.set_factors(gamma1, lam1)
        return dict(L=eng.lda_bound(ALPHA, ETA), L_documents=eng.lda_bound(ALPHA))

    with amd.Engine() as eng:
        hold(eng, name)
        fresh = second(eng)
    with amd.Engine() as eng:
        hold(eng, name)
        first = run_op(amd, eng, name, k, "lda_bound", "-")
        assert_same(first, baselines.get(name, k, "lda_bound", "-"), "the first lda_bound")
        got = second(eng)
    assert first["L"] != fresh["L"], "the two states have different bounds"
    print("\nlda_bound behind set_factors: %.9f, fresh %.9f, difference %.3g" % (got["L"], fresh["L"], got["L"] - fresh["L"]))
    assert_same(got, fresh, "lda_bound behind set_factors with other factors")




# ------------------------------------------------------------------------------------------------
# directed case 1: a block context reused over blocks of different size (the path partial_fit takes)
# ------------------------------------------------------------------------------------------------
BLOCK_SLICES = ((0, 700), (700, 740), (740, 2240), (2240, 2241), (2300, 3000), (1995, 2005))     # rows of C: n = 700, 40, 1500, 1, 700, 10
OWN_AT = 1                                                                                   # behind the n = 40 step


def test_block_slices_have_the_sizes_and_the_empty_document():
    C = corpus("C")
    assert [b - a for a, b in BLOCK_SLICES] == [700, 40, 1500, 1, 700, 10]
    lengths = np.diff(C.indptr)
    assert lengths[2000] == 0 and BLOCK_SLICES[-1][0] <= 2000 < BLOCK_SLICES[-1][1] and lengths[2240] > 0
    assert all(lengths[a:b].sum() > 0 for a, b in BLOCK_SLICES)


def _block_rho(i):
    return float((10.0 + i) ** -0.7)


def _lda_state_of(g, l):
    return (np.float32(ALPHA) + 20 * g).astype(np.float32), (np.float32(ETA) + 50 * l).astype(np.float32)


def _drive_lda_blocks(amd, k, reuse):
    """One LdaOnlineState stepped and folded over BLOCK_SLICES.  reuse: ONE engine is the state's home and the block context
    of every block; otherwise every block gets a fresh engine, and `own` (the block's own bound) yet another one."""
    C = corpus("C")
    n_all, m = C.shape
    lam0 = np.random.RandomState(_seed("blocks", "lambda", k)).gamma(100.0, 0.01, (k, m)).astype(np.float32)
    g_own, l_own = other_factors("C", k, "own lda")
    out = []
    with amd.Engine() as home, amd.LdaOnlineState(home, m, k) as st:
        st.set_lambda(lam0)
        for i, (a, b) in enumerate(BLOCK_SLICES):
            Xb, n = C[a:b], b - a
            gamma0 = np.random.RandomState(_seed("blocks", "gamma", k, i)).gamma(100.0, 0.01, (n, k)).astype(np.float32)
            eng = home if reuse else amd.Engine()
            try:
                eng.upload_csr(Xb)
                eng.set_factors(gamma0, st.get_lambda())
                rec = dict(bound=st.step(eng, ALPHA, ETA, _block_rho(i), float(n_all) / n, doc_iter=2, want_bound=True,
                                         flags=PLSA_FUSED))
                rec["lam"], rec["gamma"] = st.get_lambda(), eng.get_factors(want_v=False)[0]
                st.fold(eng, ALPHA, 2, flags=PLSA_FUSED)
                rec["folded"], rec["steps"] = eng.get_factors(want_v=False)[0], int(st.steps)
                if i == OWN_AT:                  # the block's own state: nothing of the online state may have stayed in its lda
                    own = eng if reuse else amd.Engine()
                    try:
                        if not reuse:
                            own.upload_csr(Xb)
                        own.set_factors(*_lda_state_of(g_own[a:b], l_own))
                        rec["own_L"], rec["own_L_documents"] = own.lda_bound(ALPHA, ETA), own.lda_bound(ALPHA)
                    finally:
                        if not reuse:
                            own.close()
            finally:
                if not reuse:
                    eng.close()
            out.append(rec)
    return out


def _drive_plsa_blocks(amd, k, reuse):
    """the same with an OnlineState: V, S, the block's P(z|d) and log-likelihood; `own` is one plain EM step"""
    C = corpus("C")
    m = C.shape[1]
    U_all, V0 = other_factors("C", k, "blocks plsa")
    U_own, V_own = other_factors("C", k, "own plsa")
    out = []
    with amd.Engine() as home, amd.OnlineState(home, m, k) as st:
        st.set_topics(V0)
        for i, (a, b) in enumerate(BLOCK_SLICES):
            Xb = C[a:b]
            eng = home if reuse else amd.Engine()
            try:
                eng.upload_csr(Xb)
                eng.set_factors(U_all[a:b], st.get_topics())
                rec = dict(ll=st.step(eng, _block_rho(i), 1.0 / float(Xb.sum()), inner_iter=2, want_ll=True, flags=PLSA_FUSED))
                rec["V"], rec["S"], rec["U"] = st.get_topics(), st.statistic_get(), eng.get_factors(want_v=False)[0]
                st.fold(eng, 2, flags=PLSA_FUSED)
                rec["folded"], rec["steps"] = eng.get_factors(want_v=False)[0], int(st.steps)
                if i == OWN_AT:
                    own = eng if reuse else amd.Engine()
                    try:
                        if not reuse:
                            own.upload_csr(Xb)
                        own.set_factors(U_own[a:b], V_own)
                        rec["own_ll"] = own.em_accumulate(None, THRESH, want_ll=True)
                        rec["own_acc"] = own.accumulator_get()
                        own.em_finish()
                        rec["own_U"], rec["own_V"] = own.get_factors()
                    finally:
                        if not reuse:
                            own.close()
            finally:
                if not reuse:
                    eng.close()
            out.append(rec)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k", (6, 64, 130))
@pytest.mark.parametrize("kind", ("lda", "plsa"))
def test_one_block_context_over_blocks_of_different_size(amd, kind, k):
    """One online state and ONE engine that is its home and the block context of every block -- blocks of 700, 40, 1500, 1,
    700 and 10 documents, the last with the empty document -- against the same steps on a fresh block engine each.  After
    every step the state's table(s), the block's rows and the partial bound (log-likelihood) are the same bits, and so are
    the rows after the fold.  Behind the 40-document step the block engine evaluates its OWN state (lda_bound; one EM step):
    the state's B and side arrays (V) must not have stayed behind in the block."""
    drive = _drive_lda_blocks if kind == "lda" else _drive_plsa_blocks
    fresh = drive(amd, k, reuse=False)
    got = drive(amd, k, reuse=True)
    assert len(got) == len(fresh) == len(BLOCK_SLICES) and got[-1]["steps"] == len(BLOCK_SLICES)
    for i, (g, w) in enumerate(zip(got, fresh)):
        assert_same(g, w, "%s k=%d: block %d (%d documents) on the reused block context" % (kind, k, i, BLOCK_SLICES[i][1] - BLOCK_SLICES[i][0]))


# ------------------------------------------------------------------------------------------------
# directed case 2: the snapshot slot against a shape that moved
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_snapshot_slot_against_a_shape_that_moved(amd, baselines):
    """A snapshot on A at k = 60.  Another k, another corpus and a resample of another n each make restore_factors a refusal
    that leaves the factors as they were; A at k = 60 again restores the snapshot's bits; release_scratch drops it.  After
    each refusal a plain step equals the fresh one."""
    A60, A64, B60, R60 = data("A", 60), data("A", 64), data("B", 60), data("A'", 60)

    def refused(eng, name, D, match):
        with pytest.raises(amd.DeviceError, match=match):
            eng.restore_factors()
        U, V = eng.get_factors()
        assert np.array_equal(_bits(U), _bits(D.U0)) and np.array_equal(_bits(V), _bits(D.V0)), "the refusal moved the factors"
        assert_same(run_op(amd, eng, name, D.k, "step", "-"), baselines.get(name, D.k, "step", "-"), "step behind the refusal on " + name)
        eng.set_factors(D.U0, D.V0)

    with amd.Engine() as eng:
        eng.upload_csr(corpus("A"))
        eng.set_factors(A60.U0, A60.V0)
        eng.snapshot_factors()
        eng.set_factors(A64.U0, A64.V0)
        refused(eng, "A", A64, r"640 x 480 with k=60.*640 x 480 with k=64")
        eng.upload_csr(corpus("B"))
        eng.set_factors(B60.U0, B60.V0)
        refused(eng, "B", B60, r"640 x 480 with k=60.*97 x 61 with k=60")
        eng.upload_csr(corpus("A"))
        eng.set_factors(*other_factors("A", 60))
        eng.restore_factors()
        U, V = eng.get_factors()
        assert np.array_equal(_bits(U), _bits(A60.U0)) and np.array_equal(_bits(V), _bits(A60.V0)), "the snapshot's bits"
        assert_same(run_op(amd, eng, "A", 60, "step", "-"), baselines.get("A", 60, "step", "-"), "step behind the restore")
        eng.bootstrap(bootstrap_idx())
        eng.set_factors(R60.U0, R60.V0)
        refused(eng, "A'", R60, r"640 x 480 with k=60.*600 x 480 with k=60")
        eng.bootstrap(None)
        eng.set_factors(A60.U0, A60.V0)
        eng.release_scratch()
        refused(eng, "A", A60, "no snapshot")


# ------------------------------------------------------------------------------------------------
# directed case 3: the learned-prior scratch across kp
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("via_c", (False, True))
def test_the_learned_prior_scratch_across_kp(amd, baselines, via_c):
    """`prior` at k = 130, 6, 64, 130 on one context over A (via_c: with C uploaded, fitted and A uploaded again between 6
    and 64): the page-locked slot and the device copies of the prior are grow-only in kp, so after 130 the fit at 6 works in a
    slot laid out for kp = 8 inside one sized for 132.  Every result is the fresh one, the learned alpha has exactly k entries
    and the sums of lda_prior_stats() exactly k (op_prior asserts both)."""
    with amd.Engine() as eng:
        eng.upload_csr(corpus("A"))
        for k in (130, 6, 64, 130):
            if via_c and k == 64:
                eng.upload_csr(corpus("C"))
                assert_same(run_op(amd, eng, "C", 6, "prior", "-"), baselines.get("C", 6, "prior", "-"), "prior on C at k=6")
                eng.upload_csr(corpus("A"))
            got = run_op(amd, eng, "A", k, "prior", "-")
            assert got["alpha"].shape == got["t_doc"].shape == got["t_topic"].shape == (k,)
            assert_same(got, baselines.get("A", k, "prior", "-"), "prior on A at k=%d behind the other topic counts" % k)


# ------------------------------------------------------------------------------------------------
# directed case 4: the process-wide engine behind the estimators
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_estimators_on_the_process_wide_engine(amd):
    """PLSA, LDA, OnlineLDA (two partial_fit calls of different n), tempered PLSA and smoothed PLSA, one after the other on
    get_engine()'s context, on A at k = 60, B at k = 6, A at k = 64 -- and each of them first thing after reset_engines().
    Constructor defaults but for the iteration counts (4; a test every 2 for the tempering schedule) and the seed."""
    from enstop_amd.engine import reset_engines

    def calls():
        for name, k in (("A", 60), ("B", 6), ("A", 64)):
            X = corpus(name)
            rows = X[20:40]
            e = amd.PLSA(n_components=k, n_iter=4, random_state=5).fit(X)
            yield dict(components=e.components_, transformed=e.transform(rows))
            e = amd.LDA(n_components=k, n_iter=4, random_state=6).fit(X)
            yield dict(components=e.components_, transformed=e.transform(rows))
            e = amd.OnlineLDA(n_components=k, n_iter=4, random_state=7)
            try:
                e.partial_fit(X[:50])
                e.partial_fit(X[50:85])
                yield dict(components=e.components_, embedding=e.embedding_, transformed=e.transform(rows))
            finally:
                e._end_partial()
            e = amd.PLSA(n_components=k, n_iter=4, n_iter_per_test=2, tempering="auto", random_state=8).fit(X)
            yield dict(components=e.components_, transformed=e.transform(rows))
            e = amd.PLSA(n_components=k, n_iter=4, doc_topic_smoothing=SMOOTH_A, topic_word_smoothing=SMOOTH_B, random_state=9).fit(X)
            yield dict(components=e.components_, transformed=e.transform(rows))

    reset_engines()
    try:
        shared = list(calls())                      # one context, its history growing
        own = []
        it = calls()
        while True:
            reset_engines()                         # a new context for every estimator
            try:
                own.append(next(it))
            except StopIteration:
                break
        assert len(shared) == len(own) == 15
        for i, (g, w) in enumerate(zip(shared, own)):
            assert_same(g, w, "estimator %d of round %d on the process-wide engine" % (i % 5, i // 5))
    finally:
        reset_engines()


# ------------------------------------------------------------------------------------------------
# anchors: the fresh result against float64, once per (corpus, k)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worst():
    out = {}
    yield out
    for family in sorted(out):
        ratios = out[family]
        if ratios:
            key = max(ratios, key=ratios.get)
            print("\ncontext reuse, %s: fresh results, worst error / bound %.3g (%s)" % (family, ratios[key], key))


def _fresh(amd, name):
    eng = amd.Engine()
    hold(eng, name)
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("k", K_WALK)
@pytest.mark.parametrize("name", CORPORA)
def test_fresh_results_against_float64(amd, worst, name, k):
    """One iteration of each family on a fresh context, held to the family's own float64 model and bounds."""
    D = data(name, k)
    X = D.X
    tag = "%s k=%d" % (name, k)
    # LDA: one step and the bound
    ratios = {}
    gamma0, lam0 = lda_start(name, k)
    with _fresh(amd, name) as eng:
        eng.set_factors(gamma0, lam0)
        bound0 = eng.lda_bound(ALPHA, ETA)
        iters, trace = eng.lda_fit(ALPHA, ETA, trace=True, **le.ONE)
        gamma, lam = eng.get_factors()
    want = lm.lda_step64(X, gamma0, lam0, ALPHA, ETA, THRESH)
    b_u, b_v = le.step_bounds(want, k)
    assert iters == 1 and len(trace) == 2
    check("gamma " + tag, gamma, want["gamma"], b_u, ratios)
    check("lambda " + tag, lam, want["lam"], b_v, ratios)
    assert (gamma > 0).all() and (lam > 0).all(), tag
    le.check_bound(tag + " bound", bound0, X, gamma0, lam0, k, ALPHA, ETA, ratios, float32=False)
    le.check_bound(tag + " before", trace[0], X, gamma0, lam0, k, ALPHA, ETA, ratios)
    le.check_bound(tag + " after", trace[1], X, gamma, lam, k, ALPHA, ETA, ratios)
    worst.setdefault("LDA", {}).update({"%s %s" % (key, tag) if key == "L" else key: v for key, v in ratios.items()})
    # smoothed: one step
    ratios = {}
    with _fresh(amd, name) as eng:
        eng.set_factors(D.U0, D.V0)
        iters, _ = eng.fit_smoothed(SMOOTH_A, SMOOTH_B, D.sw, **se.ONE)
        U1, V1 = eng.get_factors()
    want = sm.smoothed_step64(X, D.U0, D.V0, THRESH, SMOOTH_A, SMOOTH_B, D.sw)
    b_u, b_v = se.bounds(want, k, SMOOTH_A, SMOOTH_B)
    assert iters == 1
    check("P(z|d) " + tag, U1, want["U"], b_u, ratios)
    check("P(w|z) " + tag, V1, want["V"], b_v, ratios)
    worst.setdefault("smoothed", {}).update(ratios)
    # tempered: the tables within one ulp of the rounded power, the step the bits of an ordinary step on them
    with _fresh(amd, name) as one, _fresh(amd, name) as two:
        one.set_factors(D.U0, D.V0)
        TU, TV = one.temper_factors(BETA)
        ulps = max(int(te.ulp_distance(TU, te.power32(D.U0, BETA)).max()), int(te.ulp_distance(TV, te.power32(D.V0, BETA)).max()))
        assert ulps <= 1, (tag, ulps)
        (Ut, Vt), _ = te.tempered_step(one, D.U0, D.V0, D.sw, BETA)
        (Uo, Vo), _ = te.ordinary_step_on(two, TU, TV, D.sw)
    te.same_bits(Ut, Uo, tag + ": tempered U")
    te.same_bits(Vt, Vo, tag + ": tempered V")
    worst.setdefault("tempered tables (ulp)", {})["ulp " + tag] = float(ulps)
    # score_rows
    ref = sr.restate(X, D.U0, D.V0, D.sw, k)
    with _fresh(amd, name) as eng:
        eng.set_factors(D.U0, D.V0)
        got = eng.score_rows(None, D.sw)
    worst.setdefault("score_rows", {})["ll " + tag] = sr.check_rows(got, ref, tag)
