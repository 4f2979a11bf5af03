"""Online (stepwise) EM for pLSA on the device (Cappe & Moulines 2009; Liang & Klein 2009 -- the scheme behind scikit-learn's
LatentDirichletAllocation(learning_method="online") and its partial_fit).

Batch EM updates P(w|z) once per pass over the corpus, from topics that are one whole pass old.  Stepwise EM cuts the
documents into blocks and updates P(w|z) after every block from a running sufficient statistic S and a decaying step size:

    one step on block b, step counter t (include/plsa_hip_online.h):
      1. inner fold-in: `inner_iter` frozen-topic iterations over the block's rows under the current topics V
      2. accumulate: the fused passes of one EM iteration over the block; Vacc = the block's un-normalised P(w|z) sums
      3. S <- (1 - rho_t) S + rho_t * scale_b * Vacc,   V <- S / column sums of S
    rho_t = (tau0 + t)^(-kappa) for t = 0, 1, ... (a fixed `rho` overrides it);  scale_b = 1 / (weighted tokens of block b),
    so the statistic is per token and no corpus size has to be promised in advance;  S_0 = V0 / k.

  DeviceState       the frame of a device-side state behind the C ABI (shared with lda_online.LdaOnlineState)
  OnlineState       the device-side state (V, S, t); steps and folds are driven through it
  cut_blocks, drive_blocks   the permutation and block cutting, and the block loop, of both online fits: no engine in them
  OnlineSchedule    a state machine without an engine in it: hands out (epoch, block, rho) and takes each epoch's likelihood
  plsa_fit_online   cuts X into blocks of whole documents, one context each, and drives the schedule
  OnlinePLSA        the estimator: fit / fit_transform through plsa_fit_online, and partial_fit for documents in pieces

Every default below (n_batches, n_epochs, inner_iter, kappa, tau0) is this package's choice from a float64 NumPy model of the
algorithm on a planted corpus; none of them was tuned on a device, and the papers describe the scheme,
not these values.
"""
import ctypes as C

import numpy as np
from scipy.sparse import csr_matrix, issparse
from sklearn.utils import check_array, check_random_state

from . import _lib
from ._driver import effective_weights, host_factors, init_refit_factors, resolve_flags
from ._lib import PLSA_FUSED, PLSA_GRAPH, PLSA_REFERENCE_LL, PLSA_REFERENCE_SUMS, PLSA_SHARDED, ptr
from .engine import Engine, get_engine
from .plsa import PLSA, _locked
from .sharded import row_ranges_by_nnz
from .utils import _check_sample_weight, normalize, standardize_input

MAX_BATCHES = 256          # every block context carries three [m, kp] tables of its own
_ABI_FLAGS = PLSA_FUSED | PLSA_SHARDED | PLSA_GRAPH | PLSA_REFERENCE_SUMS | PLSA_REFERENCE_LL      # the bits a step looks at


class DeviceState:
    """The frame of a device-side online state behind the C ABI, on the device of `home` (an Engine, which must outlive the
    state: the host copies of its [k, m] tables go through its stream).  A subclass names the prefix of its entry points
    (`_prefix`_create / _destroy) and the entry point that reports the step counter, called as (state, NULL, &t)."""
    _prefix = None
    _counter = None

    def __init__(self, home, m, k):
        self._L = _lib.load()
        self.home = home
        self.m, self.k = int(m), int(k)
        self._h = C.c_void_p()
        home._ok(getattr(self._L, self._prefix + "_create")(home._h, self.m, self.k, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            if self.home._h.value:              # (a state dies with its home engine)
                getattr(self._L, self._prefix + "_destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _table(self, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.shape != (self.k, self.m):
            raise ValueError("the table has shape %s, expected %s" % (a.shape, (self.k, self.m)))
        return a

    @property
    def steps(self):
        t = C.c_int64(0)
        self.home._ok(getattr(self._L, self._counter)(self._h, None, C.byref(t)))
        return t.value


class OnlineState(DeviceState):
    """The topics V, the statistic S and the step counter on the device of `home` (an Engine, which must outlive the state:
    the host copies of V and S go through its stream).  One ABI call per method."""
    _prefix = "plsa_online"
    _counter = "plsa_online_statistic_get"

    def set_topics(self, topics):
        """V := topics [k, m], S := topics / k, t := 0"""
        self.home._ok(self._L.plsa_online_set_topics(self._h, self._table(topics)))
        return self

    def get_topics(self):
        V = np.empty((self.k, self.m), np.float32)
        self.home._ok(self._L.plsa_online_get_topics(self._h, V))
        return V

    def statistic_get(self):
        S = np.empty((self.k, self.m), np.float32)
        self.home._ok(self._L.plsa_online_statistic_get(self._h, ptr(S), None))
        return S

    def statistic_set(self, S):
        self.home._ok(self._L.plsa_online_statistic_set(self._h, self._table(S)))
        return self

    def step(self, eng, rho, scale, inner_iter=0, sample_weight=None, e_step_thresh=1e-32, want_ll=False, flags=None):
        """One step on the block resident on `eng` (module docstring); -> the block's log-likelihood under the factors the
        accumulate started from when want_ll, else None.  Without want_ll (and without host weights) nothing waits."""
        sw = None if sample_weight is None else np.ascontiguousarray(sample_weight, dtype=np.float32)
        ll = C.c_double(0.0)
        eng._ok(self._L.plsa_online_step(self._h, eng._h, ptr(sw), int(inner_iter), np.float32(e_step_thresh), float(rho),
                                         float(scale), resolve_flags(flags) & _ABI_FLAGS, C.byref(ll) if want_ll else None))
        return ll.value if want_ll else None

    def fold(self, eng, n_iter, sample_weight=None, e_step_thresh=1e-32, flags=None):
        """n_iter frozen-topic iterations over the block resident on `eng` under the state's topics, nothing else"""
        sw = None if sample_weight is None else np.ascontiguousarray(sample_weight, dtype=np.float32)
        eng._ok(self._L.plsa_online_fold(self._h, eng._h, ptr(sw), int(n_iter), np.float32(e_step_thresh),
                                         resolve_flags(flags) & _ABI_FLAGS))


class OnlineSchedule:
    """Decides what an online fit does next; it never touches an engine.

        step = schedule.next_step()               # (epoch, block, rho), or None once the fit has stopped
        ... after the last block of an epoch:  schedule.end_epoch(L_e)

    Blocks are visited in order 0 .. n_blocks - 1, every epoch.  rho of step t (t counts the steps handed out, from 0) is
    (tau0 + t)^(-kappa), or the fixed `rho`.  The stop test runs once per epoch with n_epochs as the cap: L_e is the sum of
    the blocks' log-likelihoods of epoch e, and the fit stops when |L_e - L_(e-1)| / |L_e| < tolerance (never on the first
    epoch, never with tolerance = 0, never on a NaN).  A stopped schedule stays stopped.

    `rhos`: the step sizes handed out; `log_likelihoods`: one L_e per finished epoch; `n_steps`, `n_epochs_done`."""

    def __init__(self, n_blocks, n_epochs=5, kappa=0.7, tau0=10.0, rho=None, tolerance=0.001):
        if int(n_blocks) < 1 or int(n_epochs) < 0:
            raise ValueError("n_blocks must be >= 1 and n_epochs >= 0")
        if rho is not None and not 0.0 < float(rho) <= 1.0:
            raise ValueError("rho must be in (0, 1], not %r" % (rho,))
        if rho is None and not (float(kappa) >= 0.0 and float(tau0) >= 1.0):
            raise ValueError("kappa must be >= 0 and tau0 >= 1 (so that every rho is in (0, 1]), not %r, %r" % (kappa, tau0))
        if not float(tolerance) >= 0.0:
            raise ValueError("tolerance must be >= 0, not %r" % (tolerance,))
        self.n_blocks, self.n_epochs = int(n_blocks), int(n_epochs)
        self.kappa, self.tau0 = float(kappa), float(tau0)
        self.rho = None if rho is None else float(rho)
        self.tolerance = float(tolerance)
        self.epoch, self.block, self.n_steps = 0, 0, 0
        self.rhos, self.log_likelihoods = [], []
        self.stopped = self.n_epochs == 0
        self._awaiting = False         # the last block of an epoch was handed out: end_epoch comes next

    @property
    def n_epochs_done(self):
        return len(self.log_likelihoods)

    def rho_at(self, t):
        return self.rho if self.rho is not None else float((self.tau0 + t) ** (-self.kappa))

    def next_step(self):
        if self.stopped:
            return None
        if self._awaiting:
            raise RuntimeError("epoch %d is complete: end_epoch(L) comes first" % self.epoch)
        step = (self.epoch, self.block, self.rho_at(self.n_steps))
        self.rhos.append(step[2])
        self.n_steps += 1
        self.block += 1
        self._awaiting = self.block == self.n_blocks
        return step

    def end_epoch(self, log_likelihood):
        """Takes L_e; -> True when another epoch follows."""
        if self.stopped or not self._awaiting:
            raise RuntimeError("no epoch is complete")
        cur = float(log_likelihood)
        prev = self.log_likelihoods[-1] if self.log_likelihoods else None
        self.log_likelihoods.append(cur)
        self._awaiting = False
        self.epoch, self.block = self.epoch + 1, 0
        with np.errstate(invalid="ignore", divide="ignore"):
            converged = prev is not None and bool(np.abs(np.float64(cur) - prev) / np.abs(np.float64(cur)) < self.tolerance)
        self.stopped = converged or self.epoch >= self.n_epochs
        return not self.stopped


def block_tokens(X, sample_weight=None):
    """The weighted token count of a block: sum_d w_d sum_w x_dw over the float32 values the device holds, in float64."""
    rows = np.asarray(X.astype(np.float32).astype(np.float64).sum(axis=1)).ravel()
    return float(rows.sum() if sample_weight is None else np.dot(rows, np.asarray(sample_weight, np.float64)))


def _scale(tokens, what):
    if not (tokens > 0.0 and np.isfinite(tokens)):
        raise ValueError("%s holds no tokens (weighted count %r): a step on it has no scale" % (what, tokens))
    return 1.0 / tokens


def _csr(X):
    return X.tocsr() if issparse(X) else csr_matrix(X)


def plain_fused_flags(form):
    """The resolved flags of a fit of `form` ("online EM", "online LDA"), which runs the plain fused schedule only"""
    flags = resolve_flags(None)
    if not flags & PLSA_FUSED or flags & (PLSA_REFERENCE_SUMS | PLSA_REFERENCE_LL):
        raise ValueError("%s runs the fused schedule in the default arithmetic only "
                         "(ENSTOP_AMD_MATERIALISE / ENSTOP_AMD_ARITHMETIC are set)" % form)
    return flags


def cut_blocks(who, X, n_blocks, rng, shuffle, *per_document):
    """ONE permutation of the documents drawn from `rng` (shuffle), applied to X and to every per-document array (None stays
    None), and the permuted documents cut into n_blocks ranges of whole documents with about equal non-zeros; ->
    (X, per_document, perm, ranges, undo), undo(rows) putting rows of the permuted documents back into the caller's order"""
    n = X.shape[0]
    perm = rng.permutation(n) if shuffle else None
    if perm is not None:
        X = X[perm]
        per_document = [None if a is None else a[perm] for a in per_document]
    ranges = row_ranges_by_nnz(X.indptr, n_blocks)
    if any(b <= a for a, b in ranges):
        raise ValueError("%s: %d documents cannot be split over %d blocks" % (who, n, n_blocks))

    def undo(rows):
        if perm is None:
            return rows
        out = np.empty_like(rows)
        out[perm] = rows
        return out
    return X, list(per_document), perm, ranges, undo


def drive_blocks(n, k, ranges, perm, schedule, want, series, new_engine, setup, make_state, step, fold, rows, topics,
                 callback=None):
    """The block loop of both online fits.  It imports no engine: everything that touches a device comes in as a callable.

        new_engine()             -> the context of one block (one per range, opened in block order)
        setup(eng, i, a, b)      -> (tokens, scale) of block i, documents a .. b, once it is resident on eng
        make_state()             -> the device state, made after every block is set up
        step(state, eng, rho, scale, want) -> the block's term of the epoch sum (read only when `want`)
        fold(state, eng), rows(eng), topics(state)   the final pass over a block, its rows [b - a, k], the state's [k, m] table

    Steps follow `schedule`; an epoch's sum (NaN when nothing is read) goes to schedule.end_epoch, then callback(info, state).
    After the last epoch every block is folded before any is read back.  The state is closed before the engines, whatever
    happens.  -> (rows [n, k] of the permuted documents, topics, info); `series` names the per-epoch sums in info."""
    n_blocks = len(ranges)
    engines, state = [], None
    try:
        scales, tokens = [], []
        for i, (a, b) in enumerate(ranges):
            eng = new_engine()
            engines.append(eng)
            t, scale = setup(eng, i, a, b)
            tokens.append(t)
            scales.append(scale)
        state = make_state()
        _, acc_floats = engines[0].accumulator_device()
        info = {"n_epochs": 0, "n_steps": 0, "rho": schedule.rhos, series: schedule.log_likelihoods, "block_ranges": ranges,
                "permutation": perm, "tokens": tokens, "bytes_per_block_context": 3 * 4 * int(acc_floats)}
        epoch_sum = 0.0
        while True:
            nxt = schedule.next_step()
            if nxt is None:
                break
            _, block, rho_t = nxt
            value = step(state, engines[block], rho_t, scales[block], want)
            epoch_sum += value if want else float("nan")
            if block == n_blocks - 1:
                schedule.end_epoch(epoch_sum)
                epoch_sum = 0.0
                info.update(n_epochs=schedule.n_epochs_done, n_steps=schedule.n_steps)
                if callback is not None:
                    callback(info, state)
        out = np.zeros((n, k), np.float32)
        for eng in engines:
            fold(state, eng)
        for eng, (a, b) in zip(engines, ranges):
            out[a:b] = rows(eng)
        table = topics(state)
    finally:
        if state is not None:
            state.close()
        for eng in engines:
            eng.close()
    return out, table, dict(info, rho=list(schedule.rhos), **{series: list(schedule.log_likelihoods)})


@_locked
def plsa_fit_online(X, k, sample_weight=None, init="random", n_batches=64, n_epochs=5, inner_iter=3, kappa=0.7, tau0=10.0,
                    rho=None, tolerance=0.001, shuffle_documents=True, e_step_thresh=1e-32, random_state=None, device=None,
                    return_info=False, callback=None):
    """pLSA with k topics by stepwise EM; -> (P(z|d) [n, k], P(w|z) [k, m]) as float32, with return_info an `info` dict too.

    1. The initial factors are plsa_fit's for the same seed: drawn from `random_state` first, rows of P(z|d) stay with their
       documents.
    2. shuffle_documents: ONE permutation of the documents, drawn from `random_state` after the factors.  The (permuted)
       documents are cut into min(n_batches, n) blocks of whole documents with about equal non-zeros (row_ranges_by_nnz);
       every block gets a context of its own on the device: its rows, its P(z|d), and three [m, kp] tables (n_batches is
       capped at 256; the bytes are in info["bytes_per_block_context"]).
    3. Epochs of one step per block, in block order (OnlineSchedule: rho_t, the cap n_epochs, the stop on the relative change
       of L_e, the sum of the blocks' log-likelihoods of the epoch -- a progressive likelihood that rides on the accumulate).
    4. After the last epoch every block runs max(inner_iter, 1) frozen-topic iterations under the final topics; those rows
       are the returned P(z|d), in the caller's order.

    The log-likelihoods are read (one host wait per step) only when the tolerance is positive or return_info is set.
    info: `n_epochs`, `n_steps`, `rho` (one per step), `log_likelihoods` (L_e per epoch), `block_ranges` (row ranges of the
    permuted documents), `permutation` (None without shuffling), `tokens` (per block), `bytes_per_block_context`.
    callback(info_so_far, state) is called after every epoch.  Default arithmetic, fused schedule only."""
    flags = plain_fused_flags("online EM")
    if not 1 <= int(n_batches) <= MAX_BATCHES:
        raise ValueError("n_batches must be in [1, %d], not %r" % (MAX_BATCHES, n_batches))
    if int(inner_iter) < 0:
        raise ValueError("inner_iter must be >= 0, not %r" % (inner_iter,))
    X = _csr(X)
    n, m = X.shape
    n_blocks = min(int(n_batches), n)
    if n_blocks < 1:
        raise ValueError("plsa_fit_online: no documents")
    schedule = OnlineSchedule(n_blocks, n_epochs, kappa, tau0, rho, tolerance)
    rng = check_random_state(random_state)
    U0, V0 = host_factors(k, init, rng, X=X)
    sw = effective_weights(sample_weight)
    X, (U0, sw), perm, ranges, undo = cut_blocks("plsa_fit_online", X, n_blocks, rng, shuffle_documents, U0, sw)
    home = get_engine(device)

    def setup(eng, i, a, b):
        sw_b = None if sw is None else sw[a:b]
        eng.upload_csr(X[a:b])
        eng.set_factors(U0[a:b], V0)
        eng.set_sample_weight(sw_b)
        tokens = block_tokens(X[a:b], sw_b)
        return tokens, _scale(tokens, "block %d (documents %d .. %d)" % (i, a, b))

    U, V, info = drive_blocks(
        n, k, ranges, perm, schedule, bool(return_info) or schedule.tolerance > 0.0, "log_likelihoods",
        new_engine=lambda: Engine(home.device), setup=setup, make_state=lambda: OnlineState(home, m, k).set_topics(V0),
        step=lambda state, eng, rho_t, scale, want: state.step(eng, rho_t, scale, inner_iter, None, e_step_thresh, want, flags),
        fold=lambda state, eng: state.fold(eng, max(int(inner_iter), 1), None, e_step_thresh, flags),
        rows=lambda eng: eng.get_factors(want_v=False)[0], topics=lambda state: state.get_topics(), callback=callback)
    return (undo(U), V, info) if return_info else (undo(U), V)


class PartialFitMixin:
    """What the online estimators share around partial_fit's device handles (`_partial`: a state and a scratch engine)"""

    def _end_partial(self):
        p = self.__dict__.pop("_partial", None)
        if p is not None:
            p["state"].close()
            p["engine"].close()

    def __getstate__(self):                      # device handles do not travel: a copy starts partial_fit afresh
        state = dict(self.__dict__)
        state.pop("_partial", None)
        return state

    def __del__(self):
        try:
            self._end_partial()
        except Exception:
            pass


class OnlinePLSA(PartialFitMixin, PLSA):
    """PLSA fitted by stepwise EM (plsa_fit_online; module docstring): `components_`, `embedding_`, `training_data_` as PLSA's,
    `n_iter_` = epochs run, `n_steps_` = steps taken, `online_info_` = plsa_fit_online's info.  transform, the scoring
    methods and the topic metrics are PLSA's.

    partial_fit(X) takes one step on the documents X and may be called any number of times: the first call fixes the
    vocabulary size and draws the starting topics as plsa_init(init="random") draws them (rng.rand(k, m), rows normalised)
    from `random_state`; every call uploads X to one scratch engine of the estimator's own, draws that batch's P(z|d) from
    the same stream as plsa_refit draws it, takes the step with rho of the step counter and scale = 1 / tokens of X, and
    updates `components_` and `n_steps_` (`embedding_`: that batch's P(z|d)).  n_batches, n_epochs, tolerance and
    shuffle_documents do not enter it.

    The defaults are this package's choices from a float64 model of the algorithm, not tuned on a device."""

    def __init__(self, n_components=10, init="random", n_batches=64, n_epochs=5, inner_iter=3, kappa=0.7, tau0=10.0, rho=None,
                 tolerance=0.001, shuffle_documents=True, e_step_thresh=1e-32, transform_random_seed=42, random_state=None,
                 device=None):
        self.n_components = n_components
        self.init = init
        self.n_batches = n_batches
        self.n_epochs = n_epochs
        self.inner_iter = inner_iter
        self.kappa = kappa
        self.tau0 = tau0
        self.rho = rho
        self.tolerance = tolerance
        self.shuffle_documents = shuffle_documents
        self.e_step_thresh = e_step_thresh
        self.transform_random_seed = transform_random_seed
        self.random_state = random_state
        self.device = device

    def _fit_factors(self, X, sample_weight):
        self._end_partial()
        U, V, info = plsa_fit_online(X, self.n_components, sample_weight, self.init, self.n_batches, self.n_epochs,
                                     self.inner_iter, self.kappa, self.tau0, self.rho, self.tolerance, self.shuffle_documents,
                                     self.e_step_thresh, self.random_state, device=self.device, return_info=True)
        self.n_steps_ = info["n_steps"]
        self.online_info_ = info
        return U, V, dict(n_iter=info["n_epochs"])

    # -- documents in pieces (PartialFitMixin) --------------------------------------------------------------------------
    def partial_fit(self, X, y=None, sample_weight=None):
        X = check_array(X, accept_sparse="csr")
        X = _csr(standardize_input(X))
        sample_weight = _check_sample_weight(sample_weight, X, dtype=np.float32)
        if np.any(X.data < 0):
            raise ValueError("PLSA is only valid for matrices with non-negative entries")
        n, m = X.shape
        k = int(self.n_components)
        p = self.__dict__.get("_partial")
        if p is None:
            rng = check_random_state(self.random_state)
            topics = rng.rand(k, m)
            normalize(topics, axis=1)
            engine = Engine(get_engine(self.device).device)
            p = self._partial = dict(rng=rng, engine=engine, m=m,
                                     schedule=OnlineSchedule(1, 1, self.kappa, self.tau0, self.rho, 0.0),
                                     state=OnlineState(engine, m, k).set_topics(topics.astype(np.float32)))
            self.components_ = p["state"].get_topics()
            self.n_steps_ = 0
        elif m != p["m"]:
            raise ValueError("partial_fit: X has %d words, the model was started with %d" % (m, p["m"]))
        sw = effective_weights(sample_weight)
        scale = _scale(block_tokens(X, sw), "the batch")
        eng = p["engine"]
        eng.upload_csr(X)
        init_refit_factors(eng, n, self.components_, p["rng"])
        p["state"].step(eng, p["schedule"].rho_at(self.n_steps_), scale, self.inner_iter, sw, self.e_step_thresh, False)
        self.components_ = p["state"].get_topics()
        self.embedding_ = eng.get_factors(want_v=False)[0]
        self.n_steps_ += 1
        return self
