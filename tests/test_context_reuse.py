"""A reused engine context computes what a fresh one computes.

    Whatever a context has done before, an operation on it returns exactly the bits that the same operation returns on
    a context created for it alone.  The fresh result itself stays within the pass matrix's float64 bounds.

The suite's other modules start almost every check from a new Engine.  The product does not: get_engine() hands out one
process-wide context, an ensemble bootstraps one upload dozens of times, a sweep changes k on a resident corpus, coherence
and topic combination run between fits, release_scratch() is called when memory is tight.  The context carries a dozen
structures derived from the active matrix, the lane shape or P(z|w,d) (csrc/plsa_hip.hip: Derived<T>) and grow-only scratch
that the EM passes, the structure builders, the metric kernels and the topic-combination kernels share.  Results are a
function of the inputs and the knobs only if every derived structure is invalidated by everything it was computed from
and no kernel reads scratch it did not write.  Two checks of that:

* the walk: one seeded sequence of state changes and operations over ONE Engine (build_walk), every operation compared
  bit for bit with the same operation on a fresh Engine that holds only its corpus, topic count and factors.  REQUIRED
  is the list of transitions the sequence must contain (test_walk_reaches_every_transition, CPU); the fresh result of
  `step` for every (corpus, k) is held to step64 with the pass matrix's bounds.
* directed cases, one test each: row items across the 16 x 1 / 8 x 2 document-pass shapes at k = 60 / 64, the structure
  builders under forced item lengths, shrinking and growing buffers, the process-wide engine behind the estimators,
  status-code failures.

Corpora (small: 60 002 non-zeros at most).  A: the pass matrix's corpus (matrix_corpus(6): empty documents, a 300-entry
document, a word in every document, stored zeros, escaped counts) with the factors matrix_corpus(k) seeds for each k.
B: 97 x 61, smaller than A in n, m and nnz (stale tails in every grow-only buffer after A).  C: 3000 x 2000, larger than A
in every dimension.  A': a bootstrap resample of A (600 draws: repeats and drops).  D: 2 documents of 160 entries, smaller
than B in n and nnz -- the only corpus whose document pass runs over ROW ITEMS (more than 128 entries per document), so
that the walk sees that structure too.  The walk enters and leaves D at an unchanged topic count, so that only the
new active matrix, not a new lane shape, can be what rebuilds the row items.  Topic counts 6, 60, 64, 130: column / document lane shapes (2,1)/(2,1), (16,1)/(16,1) partial,
(16,1)/(8,2) full, (32,2)/(32,2).

p_borrow takes its memory from a second Engine that only lends (p_reserve): a context that borrowed its own buffer would
free it first.

Needs a real MI355X except for test_walk_reaches_every_transition.  The wall time of the GPU tests has NOT been measured:
no figure for `pytest tests/test_context_reuse.py -m gpu`, nor for the parent commit's `tests/test_pass_matrix.py -m gpu` on the
same machine, exists yet.  By construction the work is 171 walk steps and about 100 fresh-context baselines on corpora of at
most 60 002 non-zeros, plus one directed case of about 1.4 M non-zeros fitted six times for two iterations.
"""
import functools
import zlib

import numpy as np
import pytest
import scipy.sparse as sp

from test_pass_matrix import C_FACTOR, U32, check, check_ll, lane_shape, matrix_corpus, step64, _bits

K_WALK = (6, 60, 64, 130)
BASES = ("A", "B", "C", "D")
CORPORA = ("A", "B", "C", "A'", "D")
THRESH = 1e-32
FIT = dict(n_iter=7, n_iter_per_test=3, tolerance=0.0)
MEMBER_FIT = dict(n_iter=4, n_iter_per_test=2, tolerance=0.0)
N_MEMBERS = 3
STACK_ROWS = 24


# ------------------------------------------------------------------------------------------------
# corpora, factors and the other seeded inputs (host only)
# ------------------------------------------------------------------------------------------------
def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def _random_corpus(n, m, density, seed, empty=()):
    rs = np.random.RandomState(seed)
    mask = rs.rand(n, m) < density
    mask[list(empty), :] = False
    r, c = np.nonzero(mask)
    x = rs.randint(1, 8, size=r.shape[0]).astype(np.float32)
    return sp.csr_matrix((x, (r, c)), shape=(n, m))


def _long_documents(n, m, entries, seed):
    rs = np.random.RandomState(seed)
    r = np.repeat(np.arange(n), entries)
    c = np.concatenate([np.sort(rs.choice(m, entries, replace=False)) for _ in range(n)])
    x = rs.randint(1, 8, size=r.shape[0]).astype(np.float32)
    return sp.csr_matrix((x, (r, c)), shape=(n, m))


def base_of(name):
    return "A" if name == "A'" else name


@functools.lru_cache(maxsize=None)
def bootstrap_idx():
    """A' = A[idx]: 600 draws from 640 documents (repeats some, drops others)"""
    idx = np.random.RandomState(77).randint(0, 640, size=600).astype(np.int64)
    assert np.unique(idx).shape[0] < 600 and np.setdiff1d(np.arange(640), idx).shape[0] > 0
    return idx


@functools.lru_cache(maxsize=None)
def corpus(name):
    if name == "A":
        return matrix_corpus(K_WALK[0])[0]
    if name == "A'":
        return corpus("A")[bootstrap_idx()]
    if name == "B":
        return _random_corpus(97, 61, 0.06, 11, empty=(4,))
    if name == "C":
        return _random_corpus(3000, 2000, 0.01, 12, empty=(9, 2000))
    if name == "D":
        return _long_documents(2, 300, 160, 13)
    raise KeyError(name)


class Data:
    """what an operation reads: the corpus, k, the seeded factors and document weights"""

    def __init__(self, name, k):
        self.name, self.k = name, k
        self.X = corpus(name)
        n, m = self.X.shape
        rs = np.random.RandomState(_seed("factors", name, k))
        if name == "A":                       # the pass matrix's own factors for k (subnormal block included)
            _, self.U0, self.V0, self.sw = matrix_corpus(k)
        else:
            U = rs.rand(n, k) + 0.05
            V = rs.rand(k, m) + 0.05
            self.U0 = (U / U.sum(1, keepdims=True)).astype(np.float32)
            self.V0 = (V / V.sum(1, keepdims=True)).astype(np.float32)
            self.sw = (0.5 + rs.rand(n)).astype(np.float32)
        for a in (self.U0, self.V0, self.sw):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def data(name, k):
    return Data(name, k)


def word_sets(name):
    m = corpus(name).shape[1]
    rs = np.random.RandomState(_seed("words", name))
    return np.stack([rs.choice(m, 8, replace=False) for _ in range(3)]).astype(np.int32)


def topic_stack(name):
    m = corpus(name).shape[1]
    rs = np.random.RandomState(_seed("stack", name))
    T = rs.rand(STACK_ROWS, m) ** 3 + 1e-6
    labels = (np.arange(STACK_ROWS) % 4).astype(np.int32)
    labels[[5, 17]] = -1
    return (T / T.sum(1, keepdims=True)).astype(np.float32), labels


# ------------------------------------------------------------------------------------------------
# operations: an engine that holds (corpus, k, factors) -> a dict of arrays and scalars
# ------------------------------------------------------------------------------------------------
def _weights(D, arg):
    """arg: "sw" the weights are passed, "none" no weights, "resident" none passed while resident ones apply"""
    return D.sw if arg == "sw" else None


def op_step(amd, eng, D, arg, materialised=False):
    ll = eng.em_accumulate(D.sw, THRESH, want_ll=True, materialised=materialised)
    acc = eng.accumulator_get()
    eng.em_finish()
    U, V = eng.get_factors()
    return dict(ll=ll, acc=acc, U=U, V=V)


def op_step_mat(amd, eng, D, arg):
    return op_step(amd, eng, D, arg, materialised=True)


def op_kernels(amd, eng, D, arg):
    sw = _weights(D, arg)
    ll = eng.log_likelihood(sw)
    P = eng.e_step(THRESH)
    norm_pwz, norm_pdz = eng.m_step(sw)
    U, V = eng.get_factors()
    return dict(ll=ll, P=P, norm_pwz=norm_pwz, norm_pdz=norm_pdz, U=U, V=V)


def _fit(eng, D, arg, flags):
    iters, trace = eng.fit(_weights(D, arg), flags=flags, trace=True, **FIT)
    U, V = eng.get_factors()
    return dict(iters=int(iters), trace=trace, U=U, V=V)


def op_fit_fused(amd, eng, D, arg):
    return _fit(eng, D, arg, amd.PLSA_FUSED)


def op_fit_mat(amd, eng, D, arg):
    return _fit(eng, D, arg, 0)


def op_fit_ref(amd, eng, D, arg):
    eng.set_arithmetic("reference")
    try:
        return _fit(eng, D, arg, 0)
    finally:
        eng.set_arithmetic(None)


def op_refit(amd, eng, D, arg):
    eng.fit(_weights(D, arg), flags=amd.PLSA_FUSED, **FIT)
    _, V = eng.get_factors()
    eng.set_factors(D.U0, V)
    iters, trace = eng.refit(_weights(D, arg), flags=amd.PLSA_FUSED, trace=True, **FIT)
    U, V1 = eng.get_factors()
    return dict(iters=int(iters), trace=trace, U=U, V_fitted=V, V=V1)


def op_init_mt(amd, eng, D, arg):
    rng = np.random.RandomState(_seed("mt", D.name, D.k))
    eng.init_factors_numpy_stream(D.k, rng)
    U, V = eng.get_factors()
    return dict(U=U, V=V, next_draw=float(rng.rand()))


def op_codoc(amd, eng, D, arg):
    co, positive = eng.codocument_counts(word_sets(D.name))
    return dict(co=co, positive=positive)


def op_kl(amd, eng, D, arg):
    return dict(D=eng.all_pairs_kl(topic_stack(D.name)[0]))


def op_hellinger(amd, eng, D, arg):
    return dict(D=eng.all_pairs_hellinger(topic_stack(D.name)[0]))


def op_representatives(amd, eng, D, arg):
    T, labels = topic_stack(D.name)
    return dict(R=eng.cluster_representatives(T, labels))


def op_members(amd, eng, D, arg):
    """three bootstrap members of the BASE corpus (a batch resamples the upload, not the active matrix)"""
    Db = data(base_of(D.name), D.k)
    nb = Db.X.shape[0]
    batch = eng.member_batch(N_MEMBERS)
    for j in range(N_MEMBERS):
        idx = np.random.RandomState(_seed("member", Db.name, j)).randint(0, nb, size=nb)
        batch.prepare(j, D.k, idx=idx, U=Db.U0[idx], V=Db.V0)
    iters, traces = batch.fit(N_MEMBERS, flags=amd.PLSA_FUSED, trace=True, **MEMBER_FIT)
    out = dict(iters=np.asarray(iters, np.int32))
    for j in range(N_MEMBERS):
        out["trace%d" % j] = traces[j]
        out["components%d" % j] = batch.components(j)
    return out


OPS = dict(step=op_step, step_mat=op_step_mat, kernels=op_kernels, fit_fused=op_fit_fused, fit_mat=op_fit_mat,
           fit_ref=op_fit_ref, refit=op_refit, init_mt=op_init_mt, codoc=op_codoc, kl=op_kl, hellinger=op_hellinger,
           representatives=op_representatives, members=op_members)
WEIGHTED_OPS = ("kernels", "fit_fused", "fit_mat", "fit_ref", "refit")      # take "sw" / "none" / "resident"


def hold(eng, name):
    """make `name` the active matrix of an engine that holds something else (or nothing)"""
    eng.upload_csr(corpus(base_of(name)))
    if name == "A'":
        eng.bootstrap(bootstrap_idx())


def run_op(amd, eng, name, k, op, arg):
    D = data(name, k)
    eng.set_factors(D.U0, D.V0)
    return OPS[op](amd, eng, D, arg)


def assert_same(got, want, what):
    """every array and scalar bit for bit (as _bits / _same_bits of the pass matrix)"""
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for key in sorted(got):
        g, w = got[key], want[key]
        if isinstance(g, (list, tuple)):
            g, w = np.asarray(g), np.asarray(w)
        if isinstance(g, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, w.dtype, g.shape, w.shape)
            if g.dtype.kind == "f":
                g, w = _bits(np.ascontiguousarray(g)), _bits(np.ascontiguousarray(w))
            diff = int((g != w).sum())
            assert diff == 0, "%s: %s differs in %d of %d entries (first at flat index %d)" % (
                what, key, diff, g.size, int(np.flatnonzero((g != w).ravel())[0]))
        elif isinstance(g, float):
            assert np.float64(g).view(np.uint64) == np.float64(w).view(np.uint64), (what, key, g, w)
        else:
            assert g == w, (what, key, g, w)


def check_step_against_float64(name, k, got, ratios=None):
    """the fresh `step` against the float64 step, the pass matrix's bounds: 4 (L + k) 2^-24 and check_ll"""
    D = data(name, k)
    n, m = D.X.shape
    want = step64(D.X, D.U0, D.V0, THRESH, D.sw)
    b_row = C_FACTOR * (want["L_row"] + k) * U32
    b_col = C_FACTOR * (want["L_col"] + k) * U32
    tag = "%s k=%d" % (name, k)
    kp = lane_shape(k)[0]
    acc = got["acc"].reshape(m, -1)
    assert acc.shape == (m, kp) and not acc[:, k:].any(), tag
    check("U " + tag, got["U"], want["U"], b_row, ratios)
    check("V " + tag, got["V"], want["V"], b_col, ratios)
    check("acc " + tag, acc[:, :k].T, want["V"] * want["norm_pwz"][:, None], b_col, ratios)
    check_ll("LL " + tag, got["ll"], want["ll"], want["ll_scale"], k, ratios)


class Baselines:
    """the same operation on a fresh `with Engine()` that holds only that corpus, k and factors; memoised"""

    def __init__(self, amd):
        self.amd = amd
        self.memo = {}
        self.ratios = {}

    def get(self, name, k, op, arg):
        arg = "sw" if arg == "resident" else arg             # resident weights == the same weights passed
        key = (name, k, op, arg)
        if key not in self.memo:
            with self.amd.Engine() as eng:
                hold(eng, name)
                if name == "A'":                             # the resample on the device is the host's A[idx]
                    A = eng.download_active_csr()
                    X = corpus(name)
                    assert (A.indptr == X.indptr).all() and (A.indices == X.indices).all() and (A.data == X.data).all()
                out = run_op(self.amd, eng, name, k, op, arg)
            if op == "step":
                check_step_against_float64(name, k, out, self.ratios)
            self.memo[key] = out
        return self.memo[key]


# ------------------------------------------------------------------------------------------------
# the walk: a seeded sequence of state changes and operations
# ------------------------------------------------------------------------------------------------
# steps: ("upload", corpus) ("bootstrap", "idx" | None) ("setk", k) ("release",) ("set_sw", bool) ("p_reserve",)
#        ("p_reserve_borrow",) ("p_unborrow",) ("timing", bool) ("fail", kind)          -- state changes
#        ("op", name, arg)                                                                -- operations
FAILS = ("m_step_no_p", "ll_wrong_sw")
CORPUS_PAIRS = [(a, b) for a in ("A", "B", "C", "A'") for b in ("A", "B", "C", "A'") if a != b] + \
               [(a, b) for a in ("A", "B", "C") for b in ("D",)] + [(a, b) for a in ("D",) for b in ("A", "B", "C")]
SHRINKING = (("C", "A"), ("A", "B"), ("C", "B"))

# what the walk must contain, each at least once; (a fact is produced by walk_facts below)
REQUIRED = (
    # every corpus change, both directions (D: towards and from A, B, C); the shrinking ones followed by step, kernels, codoc
    [("corpus", a, b) for a, b in CORPUS_PAIRS] +
    [("corpus", a, b, op) for a, b in SHRINKING for op in ("step", "kernels", "codoc")] +
    # every ordered pair of distinct topic counts on an unchanged upload, followed by step
    [("k", a, b) for a in K_WALK for b in K_WALK if a != b] +
    # release_scratch followed by ...
    [("after", "release", op) for op in ("step", "step_mat", "kernels", "fit_ref", "codoc", "kl", "members")] +
    # tile sums, validity of P, arithmetic scope
    [("pair", "fit_ref", "fit_fused"), ("pair", "fit_fused", "fit_ref"), ("pair", "fit_mat", "step")] +
    # shared scratch
    [("pair", a, b) for a in ("codoc", "kl", "hellinger", "representatives") for b in ("step", "kernels")] +
    # members and the leader's fits on the same upload
    [("pair", "members", "fit_fused"), ("pair", "fit_fused", "members")] +
    # bootstrap -> step, upload(A) again -> step
    [("after", "bootstrap", "step"), ("reupload", "A'", "A", "step")] +
    # a failed call, then step
    [("after", "fail:" + kind, "step") for kind in FAILS] +
    # P(z|w,d) lent, borrowed and given back
    [("after", "p_reserve_borrow", "step_mat"), ("after", "p_unborrow", "step_mat"), ("after", "p_reserve", "step_mat")] +
    # resident weights
    [("after", "set_sw:on", "fit_fused:resident"), ("after", "set_sw:off", "step")] +
    [("after", "timing:on", "fit_fused"), ("after", "timing:off", "step")] +
    # every operation; kernels with and without weights
    [("op", name) for name in ("step", "step_mat", "kernels", "fit_fused", "fit_mat", "fit_ref", "refit", "init_mt", "codoc",
                               "kl", "hellinger", "representatives", "members")] +
    [("op", "kernels", "sw"), ("op", "kernels", "none")] +
    # to and from the row-item corpus at an UNCHANGED topic count, followed by step (set_shape must not be what rebuilds them)
    [("corpus_same_k", a, "D") for a in ("A", "B", "C")] + [("corpus_same_k", "D", b) for b in ("A", "B", "C")] +
    # the row-item corpus under every topic count's document pass
    [("at", "D", k, "step") for k in K_WALK]
)


def walk_facts(steps):
    """the transitions a sequence contains: two operations are a pair when only state changes lie between them"""
    facts = set()
    cur, k = None, None
    prev = None                     # (op, arg, corpus, k) of the last operation
    changes = []                    # state changes since it
    arrival = None                  # (from, to, operations seen since) of the last corpus change
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
        if prev is not None and prev[2] != cur:
            facts.add(("corpus", prev[2], cur))
            if prev[3] == k and name == "step" and not any(c[0] == "setk" and c[1] != k for c in changes):
                facts.add(("corpus_same_k", prev[2], cur))
            arrival = [prev[2], cur, 0]
        elif moved:
            arrival = None
        if arrival is not None and arrival[2] < 3:
            facts.add(("corpus", arrival[0], arrival[1], name))
            arrival[2] += 1
        if prev is not None and prev[2] == "A'" and cur == "A" and ("upload", "A") in changes:
            facts.add(("reupload", "A'", "A", name))
        if prev is not None and not moved:
            facts.add(("pair", prev[0], name))
            if prev[3] != k and name == "step":
                facts.add(("k", prev[3], k))
        for c in changes:
            kind = c[0]
            if kind == "fail":
                kind = "fail:" + c[1]
            elif kind in ("set_sw", "timing"):
                kind = "%s:%s" % (kind, "on" if c[1] else "off")
            elif kind == "bootstrap" and not c[1]:
                kind = "restore"
            facts.add(("after", kind, name))
            facts.add(("after", kind, "%s:%s" % (name, arg)))
        prev = (name, arg, cur, k)
        changes = []
    return facts


def _euler_circuit(edges, start, rs):
    """Hierholzer over a directed multigraph, the next edge chosen by rs"""
    out = {}
    for a, b in edges:
        out.setdefault(a, []).append(b)
    for a in out:
        out[a] = [out[a][i] for i in rs.permutation(len(out[a]))]
    stack, circuit = [start], []
    while stack:
        v = stack[-1]
        if out.get(v):
            stack.append(out[v].pop())
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    assert len(circuit) == len(edges) + 1
    return circuit


class _Walk:
    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)
        self.steps = []
        self.cur = None
        self.k = None

    def emit(self, *step):
        self.steps.append(tuple(step))

    def pick_k(self):
        return K_WALK[self.rs.randint(len(K_WALK))]

    def setk(self, k):
        self.emit("setk", k)
        self.k = k

    def goto(self, name, restore=False, k=None):
        if name == "A'":
            if self.cur != "A":
                self.emit("upload", "A")
            self.emit("bootstrap", "idx")
        elif restore and self.cur == "A'" and name == "A":
            self.emit("bootstrap", None)
        else:
            self.emit("upload", name)
        self.cur = name
        self.setk(self.pick_k() if k is None else k)

    def op(self, name, arg=None):
        if arg is None:
            arg = ("sw", "none")[self.rs.randint(2)] if name in WEIGHTED_OPS else "-"
        self.emit("op", name, arg)


def _local_segments(rs):
    """pieces that leave the corpus as they found it (the A -> A' -> A one needs A); returned shuffled"""
    segs = []

    def add(fn, needs=None):
        segs.append((fn, needs))
    # topic counts: an Euler circuit over the 12 ordered pairs, cut into three pieces (each at another corpus)
    ks = _euler_circuit([(a, b) for a in K_WALK for b in K_WALK if a != b], K_WALK[1], rs)
    for lo in (0, 4, 8):
        def k_tour(w, piece=ks[lo:lo + 5]):
            w.setk(piece[0]); w.op("step")
            for k in piece[1:]:
                w.setk(k); w.op("step")
        add(k_tour)
    for name in ("step", "step_mat", "kernels", "fit_ref", "codoc", "kl", "members"):
        def release(w, name=name):
            w.emit("release"); w.op(name)
        add(release)

    def arithmetic(w):
        w.op("fit_ref"); w.op("fit_fused"); w.op("fit_ref"); w.op("fit_mat"); w.op("step")
    add(arithmetic)
    for after, args in (("step", (None, None)), ("kernels", ("sw", "none"))):
        for pair in (("codoc", "kl"), ("hellinger", "representatives")):
            def metrics(w, after=after, args=args, pair=pair):
                for metric, arg in zip(pair, args):
                    w.op(metric); w.op(after, arg)
            add(metrics)

    def members(w):
        w.op("members"); w.op("fit_fused"); w.op("members")
    add(members)

    def resample(w):
        w.emit("bootstrap", "idx"); w.cur = "A'"; w.setk(w.k); w.op("step")
        w.emit("upload", "A"); w.cur = "A"; w.setk(w.k); w.op("step")
    add(resample, "A")
    for kind in FAILS:
        def failed(w, kind=kind):
            w.emit("fail", kind); w.op("step")
        add(failed, "base")

    def lend(w):
        w.emit("p_reserve_borrow"); w.op("step_mat"); w.emit("p_unborrow"); w.op("step_mat")
    add(lend)

    def reserve(w):                       # (its own buffer handed out: it may not move until release_scratch)
        w.emit("p_reserve"); w.op("step_mat"); w.op("kernels"); w.emit("release"); w.op("fit_mat")
    add(reserve)

    def resident(w):
        w.emit("set_sw", True); w.op("fit_fused", "resident"); w.op("kernels", "resident")
        w.emit("set_sw", False); w.op("step")
    add(resident)

    def timed(w):
        w.emit("timing", True); w.op("fit_fused"); w.op("members"); w.emit("timing", False); w.op("step")
    add(timed)

    def others(w):
        w.op("init_mt"); w.op("refit"); w.op("kernels", "sw")
    add(others)
    return [segs[i] for i in rs.permutation(len(segs))]


@functools.lru_cache(maxsize=None)
def build_walk(seed=20240):
    """The sequence: an Euler circuit over the corpus changes; at every stop the operation(s) the arrival asks for, at D a
    step under every document-pass shape, then up to two of the local pieces, drawn without replacement."""
    w = _Walk(seed)
    rs = w.rs
    pool = _local_segments(rs)
    tour = _euler_circuit(CORPUS_PAIRS, "C", rs)
    restored = False
    d_ks = list(K_WALK)

    def fits(needs):
        return needs is None or (needs == "A" and w.cur == "A") or (needs == "base" and w.cur != "A'")

    def run_local(count):
        for _ in range(count):
            for i, (fn, needs) in enumerate(pool):
                if fits(needs):
                    fn(w)
                    del pool[i]
                    break
    w.goto(tour[0])
    w.op("step")
    for a, b in zip(tour[:-1], tour[1:]):
        assert w.cur == a
        w.goto(b, restore=(a, b) == ("A'", "A") and not restored, k=w.k if "D" in (a, b) else None)
        restored = restored or (a, b) == ("A'", "A")
        if (a, b) in SHRINKING:
            for name in [("step", "kernels", "codoc")[i] for i in rs.permutation(3)]:
                w.op(name)
        elif b == "D":                                   # arrives at the k it left with; then the topic counts D has not seen
            w.op("step")
            d_ks = [k for k in d_ks if k != w.k]
            for k in [d_ks.pop() for _ in range(min(len(d_ks), 2))]:
                w.setk(k); w.op("step")
        elif a == "D":
            w.op("step")
        else:
            w.op(("step", "kernels", "fit_fused", "step_mat")[rs.randint(4)])
        if b != "D":
            run_local(2 if len(w.steps) % 2 else 1)
    while pool:                                          # what is left, wherever it fits
        before = len(pool)
        run_local(len(pool))
        if len(pool) == before:
            w.goto("A")
            w.op("step")
    return tuple(w.steps)


def test_walk_reaches_every_transition():
    """The cap that keeps the walk from hiding a hole: every transition of REQUIRED occurs in it."""
    steps = build_walk()
    assert steps == build_walk.__wrapped__(), "the builder is deterministic"
    facts = walk_facts(steps)
    missing = [r for r in REQUIRED if r not in facts]
    assert not missing, missing
    n_ops = sum(s[0] == "op" for s in steps)
    assert 100 <= len(steps) <= 260, len(steps)
    # resident weights never meet a call that would pass none on purpose, nor another document count
    resident = False
    for s in steps:
        if s[0] == "set_sw":
            resident = s[1]
        assert not (resident and s[0] in ("upload", "bootstrap", "fail")), s
        assert not (resident and s[0] == "op" and s[2] == "none"), s
        assert not (not resident and s[0] == "op" and s[2] == "resident"), s
    print("\nwalk: %d steps, %d operations, %d distinct transitions" % (len(steps), n_ops, len(facts)))


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def amd():
    import enstop_amd
    return enstop_amd


@pytest.fixture(scope="module")
def baselines(amd):
    b = Baselines(amd)
    yield b
    if b.ratios:
        print("\ncontext reuse: fresh steps, worst error / bound %.3g (%s)" % (max(b.ratios.values()),
                                                                             max(b.ratios, key=b.ratios.get)))


def fail_on_purpose(amd, eng, name, k, kind):
    """A call the ABI answers with a status code; the context holds (corpus, k, factors) again afterwards."""
    D = data(name, k)
    if kind == "m_step_no_p":
        eng.set_factors(D.U0, D.V0)                       # new factors: no P(z|w,d) for them yet
        with pytest.raises(amd.DeviceError, match="no P"):
            eng.m_step()
    elif kind == "ll_wrong_sw":
        assert name != "A'"
        n = D.X.shape[0]
        eng.set_sample_weight(D.sw)                       # resident weights for n documents ...
        eng.bootstrap(np.arange(n - 1, dtype=np.int64))   # ... and an active matrix of n - 1
        eng.set_factors(D.U0[:n - 1], D.V0)
        with pytest.raises(amd.DeviceError, match="resident sample weights"):
            eng.log_likelihood(None)
        eng.set_sample_weight(None)
        eng.bootstrap(None)
        eng.set_factors(D.U0, D.V0)
    else:
        raise KeyError(kind)


MAX_P_BYTES = 4 * (60000 + 64) * 132 * 2                  # P(z|w,d) of C at k = 130, twice over


def apply_change(amd, eng, lender, state, s):
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
    elif kind == "p_reserve":
        eng.p_reserve(MAX_P_BYTES)
    elif kind == "p_reserve_borrow":
        eng.p_borrow(lender.p_reserve(MAX_P_BYTES), MAX_P_BYTES)
    elif kind == "p_unborrow":
        eng.p_borrow(None)
    elif kind == "timing":
        eng.timing(s[1])
    elif kind == "fail":
        fail_on_purpose(amd, eng, state["corpus"], state["k"], s[1])
    else:
        raise KeyError(s)


def _history(steps, i):
    lo = max([j for j in range(i) if steps[j][0] == "upload"], default=0)
    return "\n".join("  %3d %s" % (j, " ".join(str(v) for v in steps[j])) for j in range(lo, i + 1))


@pytest.mark.gpu
def test_walk_equals_fresh_contexts(amd, baselines):
    """Every operation of the walk, on one Engine with everything before it behind it, against a fresh Engine."""
    steps = build_walk()
    assert max(corpus(name).nnz for name in CORPORA) <= 61000
    state = dict(corpus=None, k=None)
    with amd.Engine() as eng, amd.Engine() as lender:
        for i, s in enumerate(steps):
            if s[0] != "op":
                apply_change(amd, eng, lender, state, s)
                continue
            _, op, arg = s
            want = baselines.get(state["corpus"], state["k"], op, arg)
            try:
                got = run_op(amd, eng, state["corpus"], state["k"], op, arg)
                assert_same(got, want, "%s(%s) on %s at k=%d" % (op, arg, state["corpus"], state["k"]))
            except (AssertionError, amd.DeviceError) as e:
                raise AssertionError("step %d of the walk differs from a fresh context: %s\nsteps since the last upload:\n%s"
                                     % (i, e, _history(steps, i))) from e
    for name in CORPORA:                                    # the float64 bound was applied to every (corpus, k) the walk steps at
        for k in K_WALK:
            if ("at", name, k, "step") in walk_facts(steps):
                assert (name, k, "step", "-") in baselines.memo


def _row_item_corpus(cus, seed=5):
    """about 300 entries per document, nnz in [34, 60] x slots16 (slots16 = cus x 32 x 4 groups of 16 lanes): per group slot
    34 to 60 entries at row_lpn = 16 (32-entry items) and 17 to 30 at row_lpn = 8 (16-entry items)"""
    slots16 = cus * 32 * 4
    m = 2000
    n = int(round(47 * slots16 / 300.0))
    rs = np.random.RandomState(seed)
    r = np.repeat(np.arange(n), 300)
    c = rs.randint(0, m, size=r.shape[0])
    X = sp.csr_matrix((rs.randint(1, 8, size=r.shape[0]).astype(np.float32), (r, c)), shape=(n, m))
    X.sum_duplicates()
    X.sort_indices()
    assert 34 * slots16 <= X.nnz <= 60 * slots16, (X.nnz, slots16)
    assert X.nnz / n > 128 and n < 2 * slots16                 # ensure_ritems: row items in use at both shapes
    return X


def _seeded_factors(n, m, k, seed):
    rs = np.random.RandomState(seed)
    U = rs.rand(n, k).astype(np.float32) + 0.05
    V = rs.rand(k, m).astype(np.float32) + 0.05
    return (U / U.sum(1, keepdims=True)).astype(np.float32), (V / V.sum(1, keepdims=True)).astype(np.float32)


def _two_iterations(amd, eng, U0, V0):
    eng.set_factors(U0, V0)
    eng.timing_reset()
    iters, trace = eng.fit(None, n_iter=2, n_iter_per_test=1, tolerance=0.0, flags=amd.PLSA_FUSED, trace=True)
    U, V = eng.get_factors()
    names = set(eng.timing_report())
    assert "k_row_reduce" in names, "the document pass did not run over row items: %s" % sorted(names)
    return dict(iters=int(iters), trace=trace, U=U, V=V), eng.pass_info()["row"]


@pytest.mark.gpu
def test_row_items_follow_the_document_pass_shape(amd):
    """k = 60 and k = 64 share the column-pass lane count (16) but not the document pass' (16 x 1 and 8 x 2): the row items
    are sized from the latter (ensure_ritems), so a change between the two must rebuild them.  A context that fitted at
    the one k and then at the other on the same upload returns the bits of a context that only ever saw the other."""
    with amd.Engine() as eng:
        cus = eng.device_info()["cus"]
    X = _row_item_corpus(cus)
    n, m = X.shape
    factors = {k: _seeded_factors(n, m, k, 100 + k) for k in (60, 64)}
    fresh = {}
    for k in (60, 64):
        with amd.Engine() as eng:
            eng.upload_csr(X)
            eng.timing(True)
            fresh[k], shape = _two_iterations(amd, eng, *factors[k])
            assert shape[:2] == ((16, 1) if k == 60 else (8, 2)), shape
    for first, second in ((60, 64), (64, 60)):
        with amd.Engine() as eng:
            eng.upload_csr(X)
            eng.timing(True)
            got, _ = _two_iterations(amd, eng, *factors[first])
            assert_same(got, fresh[first], "k=%d on a fresh upload" % first)
            got, shape = _two_iterations(amd, eng, *factors[second])
            assert shape[:2] == ((16, 1) if second == 60 else (8, 2)), shape
            assert_same(got, fresh[second], "k=%d after k=%d on the same upload" % (second, first))


def _builder_corpus():
    """300 x 200: word 0 in every document (300 entries: 38 column items of 8, a heavy column), document 7 with 150 entries
    (10 row items of 16), the others about 10 entries"""
    rs = np.random.RandomState(31)
    mask = rs.rand(300, 200) < 0.05
    mask[:, 0] = True
    mask[7, :] = False
    mask[7, rs.choice(200, 150, replace=False)] = True
    mask[7, 0] = True
    r, c = np.nonzero(mask)
    X = sp.csr_matrix((rs.randint(1, 8, size=r.shape[0]).astype(np.float32), (r, c)), shape=mask.shape)
    assert X.getnnz(axis=0)[0] == 300 and 150 <= X.getnnz(axis=1)[7] <= 151
    return X


BUILDER_KNOBS = dict(PLSA_ROW_ITEMS="1", PLSA_ROW_SEG="16", PLSA_COL_SEG="8")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ("default", "reference", "e_rows"))
def test_structure_builders_on_a_reused_context(amd, monkeypatch, variant):
    """Row items, E-step items, the CSC copy, the packed streams and the XCD stretches come from the builders of
    csrc/plsa_structures.hpp, the only code that tells a fresh context from one whose structures were built for something
    else.  One context, the smallest corpus on which each builder has more than one path (forced row items of 16 entries,
    column items of 8: several items per long row and column, a heavy column), four steps:

    1. a fit at k = 8;
    2. a fit at k = 64 on the same upload: another lane shape, so the row items and the E-step items are rebuilt.  The CSC
       copy is NOT: PLSA_COL_SEG fixes the column item length, and set_shape then keeps the copy (item_entries and n_items
       must stay what they were).  Steps 3 and 4 are what rebuilds the column side here;
    3. release_scratch and k = 8 again: the packed streams are gone and come back from the CSC arrays;
    4. a bootstrap resample and a fit, then the base corpus and k = 8 a third time: every structure is rebuilt, twice.

    Every fit and what packed_info / pass_info / balance_info say after it equal those of a context created for that fit
    alone.  In the default arithmetic; in the reference arithmetic; and in the default arithmetic with PLSA_E_ROWS=1, where
    every step also runs the E-step, over its own items, on the fitted factors and compares P(z|w,d).
    The walk above meets the same transitions, but with the knobs' defaults, under which no corpus of it has row items of
    more than one length, column items of a forced length or E-step items at all.

    One comparison is not with the fresh context.  plsa_release_scratch frees both packed streams, and only a fused pass
    writes the column stream again (ensure_packed_csc): nothing else reads it.  A fit in the reference arithmetic has no fused
    pass, so after step 3 its context must say csc: None (include/plsa_hip_diag.h: -1, not built yet), where a fresh one says
    'packed' only because k_csc_gather wrote the stream while it built the copy.  The reused context is held to exactly that:
    None for both streams, in the reference arithmetic, after release_scratch; equal to the fresh context everywhere else."""
    for name, value in BUILDER_KNOBS.items():
        monkeypatch.setenv(name, value)
    if variant == "e_rows":
        monkeypatch.setenv("PLSA_E_ROWS", "1")
    flags = 0 if variant == "reference" else amd.PLSA_FUSED
    X = _builder_corpus()
    n, m = X.shape
    idx = np.random.RandomState(32).randint(0, n, size=n).astype(np.int64)
    factors = {k: _seeded_factors(n, m, k, 200 + k) for k in (8, 64)}

    def fit(eng, k, rows=None):
        U0, V0 = factors[k]
        eng.set_factors(U0 if rows is None else U0[rows], V0)
        iters, trace = eng.fit(None, flags=flags, trace=True, **FIT)
        U, V = eng.get_factors()
        out = dict(iters=int(iters), trace=trace, U=U, V=V)
        if variant == "e_rows":
            out["P"] = eng.e_step(THRESH)
        bal = eng.balance_info()
        out.update(packed=repr(eng.packed_info()), passes=repr(eng.pass_info()), item_entries=bal["item_entries"],
                   n_items=bal["n_items"])
        return out

    def engine():
        eng = amd.Engine()
        if variant == "reference":
            eng.set_arithmetic("reference")
        eng.upload_csr(X)
        return eng

    fresh = {}
    for key, k, rows in (("k8", 8, None), ("k64", 64, None), ("resample", 8, idx)):
        with engine() as eng:
            if rows is not None:
                eng.bootstrap(rows)
            fresh[key] = fit(eng, k, rows)
    assert fresh["k8"]["item_entries"] == 8 and fresh["k8"]["n_items"] == int(np.ceil(X.getnnz(axis=0) / 8.0).sum())
    assert (fresh["k64"]["item_entries"], fresh["k64"]["n_items"]) == (fresh["k8"]["item_entries"], fresh["k8"]["n_items"])
    # the document pass does run over row items, several to a row: the longest document has more entries than an item holds
    assert X.getnnz(axis=1).max() >= 9 * int(BUILDER_KNOBS["PLSA_ROW_SEG"])
    if variant != "reference":                          # (the reference arithmetic has its own document pass)
        with engine() as eng:
            eng.timing(True)
            fit(eng, 8)
            assert "k_row_reduce" in set(eng.timing_report()), sorted(eng.timing_report())
    not_built = repr(dict(csr=None, csc=None))
    assert fresh["k8"]["packed"] == (repr(dict(csr=None, csc="packed")) if variant == "reference" else
                                     repr(dict(csr="packed", csc="packed")))
    differs = []

    def compare(got, want, what):                       # every key on its own: one difference does not hide the next
        assert sorted(got) == sorted(want)
        for key in sorted(got):
            try:
                assert_same({key: got[key]}, {key: want[key]}, what)
            except AssertionError as e:
                differs.append(str(e))

    with engine() as eng:
        compare(fit(eng, 8), fresh["k8"], "k=8 on a fresh upload")
        compare(fit(eng, 64), fresh["k64"], "k=64 after k=8 on the same upload")
        eng.release_scratch()
        after_release = dict(fresh["k8"], packed=not_built) if variant == "reference" else fresh["k8"]
        compare(fit(eng, 8), after_release, "k=8 after release_scratch")
        eng.bootstrap(idx)
        compare(fit(eng, 8, idx), fresh["resample"], "k=8 on a bootstrap resample")
        eng.bootstrap(None)
        compare(fit(eng, 8), fresh["k8"], "k=8 on the base corpus again")
    assert not differs, "\n".join(differs)


@pytest.mark.gpu
def test_shrinking_then_growing_buffers(amd, baselines):
    """C at k = 130, B at k = 6, C at k = 130 again: every grow-only buffer has a stale tail for B and is reused, not
    re-grown, for the second C."""
    with amd.Engine() as eng:
        for visit, (name, k) in enumerate((("C", 130), ("B", 6), ("C", 130))):
            eng.upload_csr(corpus(name))
            for op, arg in (("step", "-"), ("kernels", "sw"), ("kernels", "none"), ("fit_fused", "sw")):
                got = run_op(amd, eng, name, k, op, arg)
                assert_same(got, baselines.get(name, k, op, arg), "visit %d: %s(%s) on %s at k=%d" % (visit, op, arg, name, k))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FAILS)
def test_error_then_reuse(amd, baselines, kind):
    """a call that fails with a status code leaves a context that computes what a fresh one computes"""
    for name, k in (("A", 60), ("B", 6)):
        with amd.Engine() as eng:
            eng.upload_csr(corpus(name))
            got = run_op(amd, eng, name, k, "kernels", "sw")        # (a P(z|w,d) and staged weights exist)
            assert_same(got, baselines.get(name, k, "kernels", "sw"), "before the failure")
            fail_on_purpose(amd, eng, name, k, kind)
            for op, arg in (("step", "-"), ("kernels", "none")):
                got = run_op(amd, eng, name, k, op, arg)
                assert_same(got, baselines.get(name, k, op, arg), "%s after %s on %s" % (op, kind, name))


@pytest.mark.gpu
def test_initialisation_kinds_on_one_context(amd):
    """Host factors, the MT19937 stream, host document rows over the resident topics, the device generator and the refit
    initialisation, one after the other on one context: every way in sizes the factor buffers and resets the parities and
    P(z|w,d) in one place (plsa_init.hpp: alloc_factors), so after each step the context holds, bit for bit, what a fresh
    context holds after that step alone.  k = 6, 33, 6, 20, 6 pads to 8, 36, 8, 20 (no padding), 8: the lane shape changes in
    both directions."""
    X = _random_corpus(130, 70, 0.1, _seed("init kinds"))
    n, m = X.shape
    U6, V6 = _seeded_factors(n, m, 6, 61)
    U6b, V6b = _seeded_factors(n, m, 6, 62)
    U6c, _ = _seeded_factors(n, m, 6, 63)

    def read(eng, **more):
        U, V = eng.get_factors()
        return dict(U=U, V=V, **more)

    def two_iterations(eng):
        iters, trace = eng.fit(None, n_iter=2, n_iter_per_test=1, tolerance=0.0, flags=amd.PLSA_FUSED, trace=True)
        return read(eng, iters=int(iters), trace=trace)

    def host(eng):
        return read(eng.set_factors(U6, V6)), None

    def stream(eng):
        rng = np.random.RandomState(_seed("init kinds", 33))
        got = read(eng.init_factors_numpy_stream(33, rng), next_draw=float(rng.rand()))
        return got, two_iterations(eng)

    def rows_only(eng):
        eng.set_factors(U6b, V6b)
        got = read(eng.set_factors(U6c))
        assert np.array_equal(_bits(got["V"]), _bits(V6b)) and np.array_equal(_bits(got["U"]), _bits(U6c))
        return got, None

    def device(eng):
        return read(eng.init_factors_device(20, seed=77)), None

    def refit_stream(eng):
        rng = np.random.RandomState(_seed("init kinds", 6))
        got = read(eng.init_factors_numpy_stream(6, rng, topics=V6), next_draw=float(rng.rand()))
        assert np.array_equal(_bits(got["V"]), _bits(V6))
        return got, two_iterations(eng)

    steps = (host, stream, rows_only, device, refit_stream)
    fresh = []
    for step in steps:
        with amd.Engine() as eng:
            eng.upload_csr(X)
            fresh.append(step(eng))
    assert [(f[0]["U"].shape[1], lane_shape(f[0]["U"].shape[1])[0]) for f in fresh] == [(6, 8), (33, 36), (6, 8), (20, 20), (6, 8)]
    with amd.Engine() as eng:
        eng.upload_csr(X)
        for step, (want, want_fit) in zip(steps, fresh):
            got, got_fit = step(eng)
            assert_same(got, want, "%s after the steps before it" % step.__name__)
            if want_fit is not None:
                assert_same(got_fit, want_fit, "two fused iterations after %s" % step.__name__)


def _planted(n, m, k_true, seed):
    rs = np.random.RandomState(seed)
    topics = rs.dirichlet(np.full(m, 0.03), size=k_true)
    mix = rs.dirichlet(np.full(k_true, 0.2), size=n)
    X = sp.csr_matrix(rs.poisson(80 * (mix @ topics)).astype(np.float32))
    return X[np.asarray(X.sum(1)).ravel() > 0]


@pytest.mark.gpu
def test_process_wide_engine_history(amd):
    """The estimators share get_engine(): PLSA at k = 60, PLSA at k = 64 on the same data, a transform, an ensemble on
    other data, one after the other on the process-wide context -- and the same calls each on a context of its own."""
    from enstop_amd.engine import reset_engines
    X1 = _planted(500, 300, 5, 1)
    X2 = _planted(600, 300, 4, 0)

    def calls():
        a = amd.PLSA(n_components=60, n_iter=12, n_iter_per_test=4, random_state=3).fit(X1)
        yield dict(components=a.components_, embedding=np.asarray(a.embedding_))
        b = amd.PLSA(n_components=64, n_iter=12, n_iter_per_test=4, random_state=4).fit(X1)
        yield dict(components=b.components_, embedding=np.asarray(b.embedding_))
        yield dict(transformed=b.transform(X1[:200]))
        e = amd.EnsembleTopics(n_components=4, n_starts=8, min_samples=2, min_cluster_size=3, topic_combination="hellinger",
                               n_iter=40, random_state=3)
        emb = e.fit_transform(X2)
        yield dict(components=e.components_, embedding=emb)
        yield dict(transformed=e.transform(X2[:100]), again=b.transform(X1[:200]))

    reset_engines()
    try:
        shared = list(calls())                      # one context, its history growing
        own = []
        it = calls()
        while True:
            reset_engines()                         # a new context for every call
            try:
                own.append(next(it))
            except StopIteration:
                break
        assert len(shared) == len(own) == 5
        for i, (g, w) in enumerate(zip(shared, own)):
            assert_same(g, w, "call %d on the process-wide engine" % i)
    finally:
        reset_engines()
