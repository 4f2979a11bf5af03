"""Engine: one MI355X + one HIP stream + the device-resident corpus and factors.

Thin object wrapper over the C ABI (include/plsa_hip.h); every method is one or two ABI calls.
The reference keeps all of this state in NumPy arrays handed from function to function
(enstop/plsa.py:707-730); here it lives in HBM for the lifetime of the Engine.
"""
import ctypes as C
import os
import threading

import numpy as np

from . import _lib
from ._lib import (PLSA_FUSED, PLSA_REFERENCE_LL, PLSA_REFERENCE_SUMS, PLSA_SHARDED, PLSA_STOP_NO_ZERO_ARM, PLSA_SW_LL_ONLY,
                   PLSA_TRACE_LL, ptr)


class DeviceError(RuntimeError):
    pass


def default_device():
    """One process per GPU: LOCAL_RANK (torchrun / bench.py's spawner) selects the device unless
    ENSTOP_AMD_DEVICE overrides it; a launcher that narrows the visible devices to one per rank
    (HIP_VISIBLE_DEVICES) leaves only device 0."""
    if "ENSTOP_AMD_DEVICE" in os.environ:
        return int(os.environ["ENSTOP_AMD_DEVICE"])
    dev = int(os.environ.get("LOCAL_RANK", "0"))
    if dev > 0:
        cnt = C.c_int(0)
        if _lib.load().plsa_device_count(C.byref(cnt)) == 0 and 0 < cnt.value <= dev:
            if cnt.value != 1:
                raise RuntimeError("LOCAL_RANK=%d but only %d GPUs are visible: start one rank per visible GPU, "
                                   "narrow the devices to one per rank (HIP_VISIBLE_DEVICES), or set "
                                   "ENSTOP_AMD_DEVICE" % (dev, cnt.value))
            dev = 0
    return dev


def arithmetic_flags(arithmetic):
    """`arithmetic=` of the fit functions -> flag bits.  None / "default": the engine's own summation orders (float64
    norm_pwz and log-likelihood; more accurate than the reference).  "reference": PLSA_REFERENCE_SUMS -- every sum of the
    E- and M-step one float32 accumulator in the reference's loop order: the bits of enstop/plsa.py executed statement
    by statement; the log-likelihood stays float64-accumulated (what the numba-compiled reduction delivers to 1e-7).
    "reference_source": additionally PLSA_REFERENCE_LL -- the log-likelihood as ONE float32 running sum (plsa.py:322
    read literally, one thread).  An int passes through."""
    if arithmetic is None or arithmetic == "default":
        return 0
    if isinstance(arithmetic, (int, np.integer)):
        if int(arithmetic) & ~(PLSA_REFERENCE_SUMS | PLSA_REFERENCE_LL):
            raise ValueError("arithmetic bits must be PLSA_REFERENCE_SUMS | PLSA_REFERENCE_LL")
        return int(arithmetic)
    if arithmetic == "reference":
        return PLSA_REFERENCE_SUMS
    if arithmetic == "reference_source":
        return PLSA_REFERENCE_SUMS | PLSA_REFERENCE_LL
    raise ValueError('arithmetic must be None, "default", "reference" or "reference_source", not %r' % (arithmetic,))


def default_flags():
    """Fit schedule: fused (P(z|w,d) never touches HBM) unless ENSTOP_AMD_MATERIALISE=1, which
    follows the reference's E-step -> M-step kernel sequence through a materialised nnz x k array.
    ENSTOP_AMD_ARITHMETIC=reference / reference_source adds the reference's rounding (arithmetic_flags).
    These are the flags of a fit that is given none (_driver.resolve_flags); explicit `flags=` replace them, and
    StreamedPLSA starts from PLSA_FUSED without consulting either variable."""
    flags = 0 if os.environ.get("ENSTOP_AMD_MATERIALISE", "0") == "1" else PLSA_FUSED
    return flags | arithmetic_flags(os.environ.get("ENSTOP_AMD_ARITHMETIC") or None)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _mt19937_state(rng):
    """(uint32[625]: MT19937 key and position, which the device advances in place; put_back(): writes them into `rng`)"""
    kind, key, pos, has_gauss, cached = rng.get_state()
    if kind != "MT19937":
        raise ValueError("not an MT19937 RandomState")
    state = np.empty(625, np.uint32)
    state[:624] = key
    state[624] = pos
    return state, lambda: rng.set_state((kind, state[:624].copy(), int(state[624]), has_gauss, cached))


def _csr_arrays(X):
    """(indptr int32, indices int32, data float32), contiguous, of a scipy matrix (any dtype; values are cast like
    plsa.py:714).  The device layout is the reference's: int32 row pointers / indices (plsa.py:26 `i4[::1]`, its loop
    counters are uint32).  scipy switches to int64 index arrays on its own for large matrices: what does not fit is
    refused instead of letting the casts wrap around."""
    X = X.tocsr()
    n, m = X.shape
    if X.nnz > 2**31 - 64 or max(n, m) >= 2**31 - 1:
        raise ValueError("matrix too large for 32-bit indices: %d x %d with %d stored entries (limit 2^31 - 64 entries)"
                         % (n, m, X.nnz))
    return (np.ascontiguousarray(X.indptr, dtype=np.int32), np.ascontiguousarray(X.indices, dtype=np.int32), _f32(X.data))


def _csr_failure(msg, pointer_text_wins=False):
    """The exception for the error text of plsa_upload_csr / plsa_score_rows: a violated index contract (k_validate_csr,
    or the row pointers' ends) is the reference-style ValueError, everything else a DeviceError.  A bad column id reads
    "column index out of range" -- unless, for score_rows (pointer_text_wins), the row pointers are out of order as well."""
    if "column index" in msg or "indptr" in msg:
        short = "column index" in msg and not (pointer_text_wins and "indptr is" in msg)
        return ValueError("column index out of range" if short else msg)
    return DeviceError(msg)


class Engine:
    def __init__(self, device=None):
        self._L = _lib.load()
        self._h = C.c_void_p()
        dev = default_device() if device is None else int(device)
        if self._L.plsa_create(dev, C.byref(self._h)):
            raise DeviceError(self._L.plsa_last_error(None).decode())
        self.device = dev
        self.k = 0
        self.base_rows = 0
        self.p_budget = 0              # set_p_budget
        self.arithmetic_bits = 0       # set_arithmetic (the C context has no getter: this record is what scoped calls restore)
        # a context is not thread-safe: callers that share the process-wide engine (the reference is
        # driven from dask/joblib thread pools, enstop_.py:209-217) serialise on this lock
        self.lock = threading.RLock()
        self._member_batch = None      # cached MemberBatch (member_batch): its slots keep their buffers between ensembles

    # -- lifetime --------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            if getattr(self, "_member_batch", None) is not None:      # the batch borrows this context's streams and corpus
                self._member_batch.close()
                self._member_batch = None
            self._L.plsa_destroy(self._h)
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

    def _ok(self, rc):
        if rc:
            raise DeviceError(self._L.plsa_last_error(self._h).decode())

    def synchronize(self):
        self._ok(self._L.plsa_synchronize(self._h))

    def device_info(self):
        name, arch = C.create_string_buffer(64), C.create_string_buffer(64)
        cus, hbm = C.c_int(0), C.c_int64(0)
        self._ok(self._L.plsa_device_info(self._h, name, arch, C.byref(cus), C.byref(hbm)))
        return dict(name=name.value.decode(), arch=arch.value.decode(), cus=cus.value, hbm_bytes=hbm.value)

    # -- corpus ----------------------------------------------------------------------------------
    def upload_csr(self, X):
        """X: scipy CSR (any dtype; values are cast to float32 like plsa.py:714)."""
        n, m = X.shape
        indptr, indices, data = _csr_arrays(X)
        # the index contract (0 <= column < m, row pointers non-decreasing) is checked ON THE DEVICE by one streaming pass over
        # the copy (k_validate_csr): a host-side min() / max() over the indices of config 3 cost more than the upload itself
        # (62 ms for 100 M entries on the build container).  A violation is the reference-style ValueError either way.
        if self._L.plsa_upload_csr(self._h, indptr, indices, data, n, m, data.shape[0]):
            raise _csr_failure(self._L.plsa_last_error(self._h).decode())
        self.base_rows = n
        return self

    def generate_synthetic(self, n, m, nnz, zipf_s=1.07, seed=0, topics=0, alpha=0.1, background=0.25):
        """Synthetic bag-of-words corpus generated in HBM (becomes base + active matrix); returns the exact nnz.
        topics = 0: every token an independent Zipf draw.  topics = k0 > 0: documents are Dirichlet(alpha) mixtures
        of k0 latent topics with their own Zipf rankings plus a shared `background` ranking (text-like co-occurrence)."""
        out = C.c_int64(0)
        if topics:
            self._ok(self._L.plsa_generate_synthetic_topics(self._h, n, m, nnz, float(zipf_s), int(seed), int(topics),
                                                            float(alpha), float(background), C.byref(out)))
        else:
            self._ok(self._L.plsa_generate_synthetic(self._h, n, m, nnz, float(zipf_s), int(seed), C.byref(out)))
        self.base_rows = n
        return out.value

    def synthetic_dominant_topics(self):
        """Ground truth of the topical synthetic corpus held as the base matrix: the dominant latent topic of every document."""
        out = np.empty(self.base_rows, np.int32)
        self._ok(self._L.plsa_synthetic_dominant_topics(self._h, out))
        return out

    def bootstrap(self, idx):
        """active := base[idx] on the device (enstop_.py:87-88); idx=None restores the base."""
        if idx is None:
            self._ok(self._L.plsa_bootstrap(self._h, None, 0))
        else:
            idx = np.ascontiguousarray(idx, dtype=np.int64)
            self._ok(self._L.plsa_bootstrap(self._h, idx.ctypes.data, idx.shape[0]))
        return self

    @property
    def shape(self):
        n, m, nnz = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._ok(self._L.plsa_active_shape(self._h, C.byref(n), C.byref(m), C.byref(nnz)))
        return n.value, m.value, nnz.value

    def download_active_csr(self):
        import scipy.sparse as sp
        n, m, nnz = self.shape
        indptr = np.empty(n + 1, np.int32)
        indices = np.empty(max(nnz, 1), np.int32)
        data = np.empty(max(nnz, 1), np.float32)
        self._ok(self._L.plsa_download_active_csr(self._h, indptr, indices, data))
        return sp.csr_matrix((data[:nnz], indices[:nnz], indptr), shape=(n, m))

    # -- factors ---------------------------------------------------------------------------------
    def set_factors(self, p_z_given_d, p_w_given_z=None):
        U = _f32(p_z_given_d)
        n, k = U.shape
        _, m, _ = self.shape
        V = None
        if p_w_given_z is not None:
            V = _f32(p_w_given_z)
            if V.shape != (k, m):
                raise ValueError("p_w_given_z has shape %s, expected %s" % (V.shape, (k, m)))
        self._ok(self._L.plsa_set_factors(self._h, ptr(U), ptr(V), n, m, k))
        self.k = k
        return self

    def init_factors_device(self, k, seed=0):
        """Throughput-mode random init on the device (not the reference's MT19937 stream)."""
        self._ok(self._L.plsa_init_factors_device(self._h, int(k), int(seed) & (2 ** 64 - 1)))
        self.k = int(k)
        return self

    def init_factors_numpy_stream(self, k, rng, topics=None):
        """plsa_init(random) + float32 casts on the device, drawing from `rng` (a legacy
        numpy.random.RandomState, MT19937) exactly as rng.rand(k, m); rng.rand(n, k) would; `rng`
        is left in the state the host path would leave it in.  With `topics` ([k, m], fixed) only
        rng.rand(n, k) is drawn: the initialisation of plsa_refit (plsa.py:979-981)."""
        state, put_back = _mt19937_state(rng)
        if topics is None:
            self._ok(self._L.plsa_init_factors_mt19937(self._h, int(k), state))
        else:
            V = _f32(topics)
            if V.shape[0] != int(k):
                raise ValueError("topics have %d rows, expected k=%d" % (V.shape[0], int(k)))
            self._ok(self._L.plsa_refit_init_mt19937(self._h, ptr(V), V.shape[1], int(k), state))
        put_back()
        self.k = int(k)
        return self

    def mt_marginals(self):
        """float64 row sums of the topic draws of the last init_factors_numpy_stream call (diagnostics / tests)."""
        out = np.empty(self.k, np.float64)
        self._ok(self._L.plsa_mt_marginals(self._h, out, int(self.k)))
        return out

    def get_factors(self, want_u=True, want_v=True):
        n, m, _ = self.shape
        U = np.empty((n, self.k), np.float32) if want_u else None
        V = np.empty((self.k, m), np.float32) if want_v else None
        self._ok(self._L.plsa_get_factors(self._h, ptr(U), ptr(V)))
        return U, V

    def copy_components_to_device(self, device_ptr):
        self._ok(self._L.plsa_copy_components_to_device(self._h, int(device_ptr)))

    # -- KL-divergence NMF (include/plsa_hip_nmf.h) --------------------------------------------------
    def nmf_set_factors(self, W, H):
        W, H = _f32(W), _f32(H)
        n, k = W.shape
        _, m, _ = self.shape
        if H.shape != (k, m):
            raise ValueError("H has shape %s, expected %s" % (H.shape, (k, m)))
        self._ok(self._L.plsa_nmf_set_factors(self._h, W, H, n, m, k))
        self.k = k
        return self

    def nmf_get_factors(self, want_w=True, want_h=True):
        n, m, _ = self.shape
        W = np.empty((n, self.k), np.float32) if want_w else None
        H = np.empty((self.k, m), np.float32) if want_h else None
        self._ok(self._L.plsa_nmf_get_factors(self._h, ptr(W), ptr(H)))
        return W, H

    def nmf_update_w(self):
        self._ok(self._L.plsa_nmf_update_w(self._h))
        return self

    def nmf_update_h(self):
        self._ok(self._L.plsa_nmf_update_h(self._h))
        return self

    def nmf_divergence(self):
        """sqrt(2 D), D the generalised Kullback-Leibler divergence of the active matrix from W H"""
        out = C.c_double(0.0)
        self._ok(self._L.plsa_nmf_divergence(self._h, C.byref(out)))
        return out.value

    def nmf_fit(self, update_h=True, max_iter=200, tol=1e-4):
        """(n_iter, errors): errors[0] is the objective before the first update, then one entry per stopping test"""
        max_iter = int(max_iter)
        errors = np.zeros(max(max_iter, 0) // 10 + 2, np.float64)
        n_iter = C.c_int32(0)
        self._ok(self._L.plsa_nmf_fit(self._h, 1 if update_h else 0, max_iter, float(tol), C.byref(n_iter), ptr(errors),
                                      errors.shape[0]))
        tested = n_iter.value // 10 if tol > 0 else 0
        return n_iter.value, errors[:1 + tested].copy()

    # -- kernel-level operators --------------------------------------------------------------------
    def set_arithmetic(self, arithmetic=None):
        """Arithmetic of e_step / m_step / log_likelihood and of later fits on this engine (arithmetic_flags)."""
        bits = arithmetic_flags(arithmetic)
        self._ok(self._L.plsa_set_arithmetic(self._h, bits))
        self.arithmetic_bits = bits
        return self

    def e_step(self, thresh=1e-32, out=None, want_host_copy=True):
        _, _, nnz = self.shape
        if want_host_copy and out is None:
            out = np.empty((nnz, self.k), np.float32)
        self._ok(self._L.plsa_e_step(self._h, np.float32(thresh), ptr(out) if want_host_copy else None))
        return out

    def set_p(self, P):
        self._ok(self._L.plsa_set_p(self._h, _f32(P)))

    def m_step(self, sample_weight=None, update_v=True):
        n, _, _ = self.shape
        sw = None if sample_weight is None else _f32(sample_weight)
        npwz = np.zeros(self.k, np.float32)
        npdz = np.zeros(n, np.float32)
        self._ok(self._L.plsa_m_step(self._h, ptr(sw), int(update_v), ptr(npwz), ptr(npdz)))
        return npwz, npdz

    def log_likelihood(self, sample_weight=None):
        sw = None if sample_weight is None else _f32(sample_weight)
        out = C.c_double(0.0)
        self._ok(self._L.plsa_log_likelihood(self._h, ptr(sw), C.byref(out)))
        return out.value

    # -- held-out scoring (include/plsa_hip_score.h) ---------------------------------------------------
    def score_rows(self, other=None, sample_weight=None):
        """Per-document (ll, tokens, unscored), float64 [n] each, under the factors in force: the log-likelihood terms of
        log_likelihood summed per document over the entries with x > 0 and a positive model probability, the weighted
        count of those entries, and the weighted count of the entries whose word the model gives no mass.  other=None
        scores the active matrix; a scipy matrix of the active matrix's shape is scored against the same factors from
        scratch buffers and leaves the resident corpus, the factors and every derived structure as they were.  Values
        are cast to float32 like upload_csr's; a bad shape, column id or row pointer is a ValueError."""
        n, m, _ = self.shape
        sw = None if sample_weight is None else _f32(sample_weight)
        if sw is not None and sw.shape != (n,):
            raise ValueError("sample_weight has shape %s, expected (%d,)" % (sw.shape, n))
        indptr = indices = data = None
        nnz = 0
        if other is not None:
            if other.shape != (n, m):
                raise ValueError("the other matrix has shape %s, the active matrix (and the factors) %s"
                                 % (other.shape, (n, m)))
            indptr, indices, data = _csr_arrays(other)
            nnz = data.shape[0]
        ll, tokens, unscored = (np.empty(n, np.float64) for _ in range(3))
        if self._L.plsa_score_rows(self._h, ptr(indptr), ptr(indices), ptr(data), nnz, ptr(sw), ptr(ll), ptr(tokens),
                                   ptr(unscored)):
            raise _csr_failure(self._L.plsa_last_error(self._h).decode(), pointer_text_wins=True)
        return ll, tokens, unscored

    # -- EM drivers --------------------------------------------------------------------------------
    def _drive(self, fn, sample_weight, n_iter, n_iter_per_test, tolerance, thresh, flags, trace):
        sw = None if sample_weight is None else _f32(sample_weight)
        ll = np.zeros(n_iter + 2, np.float32)
        iters, nll = C.c_int32(0), C.c_int32(0)
        flags = default_flags() if flags is None else flags
        if trace:
            flags |= PLSA_TRACE_LL
        self._ok(fn(self._h, ptr(sw), int(n_iter), int(n_iter_per_test), float(tolerance),
                    np.float32(thresh), int(flags), C.byref(iters), ll.ctypes.data, C.byref(nll)))
        return iters.value, ll[: nll.value].copy()

    def fit(self, sample_weight=None, n_iter=100, n_iter_per_test=10, tolerance=0.001,
            e_step_thresh=1e-32, flags=None, trace=False):
        return self._drive(self._L.plsa_fit, sample_weight, n_iter, n_iter_per_test, tolerance,
                           e_step_thresh, flags, trace)

    def refit(self, sample_weight=None, n_iter=50, n_iter_per_test=10, tolerance=0.005,
              e_step_thresh=1e-32, flags=None, trace=False):
        return self._drive(self._L.plsa_refit, sample_weight, n_iter, n_iter_per_test, tolerance,
                           e_step_thresh, flags, trace)

    # -- tempered EM (include/plsa_hip_tempered.h) ----------------------------------------------------
    def fit_tempered(self, beta, sample_weight=None, n_iter=100, n_iter_per_test=10, tolerance=0.001,
                     e_step_thresh=1e-32, flags=None, trace=False):
        """fit() with the responsibilities flattened by the exponent 0 < beta <= 1: every iteration raises the factors to
        the power beta into two side tables and runs the fused iteration on those.  Same loop, stop rule and return
        values as fit; every likelihood is the likelihood of the true factors.  beta == 1.0 is fit().  Fused default
        arithmetic only: anything else is a DeviceError that launches nothing."""
        def fn(h, sw, *rest):
            return self._L.plsa_fit_tempered(h, sw, float(beta), *rest)
        return self._drive(fn, sample_weight, n_iter, n_iter_per_test, tolerance, e_step_thresh, flags, trace)

    def temper_factors(self, beta):
        """(P(z|d)^beta [n, k], P(w|z)^beta [k, m]): the side tables a tempered iteration at beta forms from the factors in
        force, which stay as they are (diagnostics / tests)."""
        n, m, _ = self.shape
        U, V = np.empty((n, self.k), np.float32), np.empty((self.k, m), np.float32)
        self._ok(self._L.plsa_temper_factors(self._h, float(beta), ptr(U), ptr(V)))
        return U, V

    def snapshot_factors(self):
        """Copy the factors in force into the engine's one snapshot slot (device to device)."""
        self._ok(self._L.plsa_factors_snapshot(self._h))
        return self

    def restore_factors(self):
        """The snapshot becomes the factors in force again; DeviceError without one, or after the shape or k changed."""
        self._ok(self._L.plsa_factors_restore(self._h))
        return self

    # -- smoothed (MAP) EM (include/plsa_hip_diag.h, its own section) ----------------------------------
    def fit_smoothed(self, doc_topic_smoothing=0.0, topic_word_smoothing=0.0, sample_weight=None, n_iter=100,
                     n_iter_per_test=10, tolerance=0.001, e_step_thresh=1e-32, flags=None, trace=False):
        """fit() with the pseudo-counts a = doc_topic_smoothing and b = topic_word_smoothing added to the expected counts of
        every M-step: P(z|d) = (n_dz + a) / (N_d + k a), P(w|z) = (n_wz + b) / (N_z + m b).  Same loop, stop rule and return
        values as fit; the trace holds the log posterior (log_posterior) where fit has the log-likelihood.  a == b == 0 is
        fit().  Fused default arithmetic on one GPU only: anything else is a DeviceError that launches nothing."""
        def fn(h, sw, *rest):
            return self._L.plsa_fit_smoothed(h, sw, float(doc_topic_smoothing), float(topic_word_smoothing), *rest)
        return self._drive(fn, sample_weight, n_iter, n_iter_per_test, tolerance, e_step_thresh, flags, trace)

    def refit_smoothed(self, doc_topic_smoothing=0.0, sample_weight=None, n_iter=50, n_iter_per_test=10, tolerance=0.005,
                       e_step_thresh=1e-32, flags=None, trace=False):
        """refit() with the document-side pseudo-count: only P(z|d) moves, the topics are never written.  0 is refit()."""
        def fn(h, sw, *rest):
            return self._L.plsa_refit_smoothed(h, sw, float(doc_topic_smoothing), *rest)
        return self._drive(fn, sample_weight, n_iter, n_iter_per_test, tolerance, e_step_thresh, flags, trace)

    def log_posterior(self, sample_weight=None, doc_topic_smoothing=0.0, topic_word_smoothing=0.0):
        """log_likelihood + a sum_d sw_d sum_z log P(z|d) + b sum_z sum_w log P(w|z) of the factors in force (float64): the
        objective a smoothed iteration does not decrease.  At a == b == 0 it has the bits of log_likelihood."""
        sw = None if sample_weight is None else _f32(sample_weight)
        out = C.c_double(0.0)
        self._ok(self._L.plsa_log_posterior(self._h, ptr(sw), float(doc_topic_smoothing), float(topic_word_smoothing),
                                            C.byref(out)))
        return out.value

    # -- variational Bayes LDA (include/plsa_hip_diag.h, its own section) --------------------------------------------------
    def _lda_drive(self, fn, n_iter, n_iter_per_test, tolerance, doc_iter, thresh, flags, trace):
        bound = np.zeros(n_iter + 2, np.float32)
        iters, count = C.c_int32(0), C.c_int32(0)
        flags = PLSA_FUSED if flags is None else flags
        if trace:
            flags |= PLSA_TRACE_LL
        self._ok(fn(int(n_iter), int(n_iter_per_test), float(tolerance), int(doc_iter), np.float32(thresh), int(flags),
                    C.byref(iters), bound.ctypes.data, C.byref(count)))
        return iters.value, bound[: count.value].copy()

    def lda_fit(self, doc_topic_prior, topic_word_prior, n_iter=100, n_iter_per_test=10, tolerance=0.001, doc_iter=1,
                e_step_thresh=1e-32, flags=None, trace=False):
        """Variational Bayes LDA from the state set_factors put on the engine, gamma [n, k] where P(z|d) lives and lambda [k, m]
        where P(w|z) lives: every iteration forms the exp-digamma tables of the state, runs the fused passes on them and
        adds the priors behind the passes.  fit()'s loop, stop rule and return values, with the bound (lda_bound) where fit
        has the log-likelihood.  doc_iter - 1 extra rounds per iteration update gamma alone.  Any priors > 0; fused default
        arithmetic on one GPU only: anything else is a DeviceError that launches nothing."""
        def fn(*rest):
            return self._L.plsa_lda_fit(self._h, float(doc_topic_prior), float(topic_word_prior), *rest)
        return self._lda_drive(fn, n_iter, n_iter_per_test, tolerance, doc_iter, e_step_thresh, flags, trace)

    def lda_refit(self, doc_topic_prior, n_iter=50, n_iter_per_test=10, tolerance=0.005, doc_iter=1, e_step_thresh=1e-32,
                  flags=None, trace=False):
        """The fold-in: only gamma moves, lambda is never written; the bound of the trace leaves the topic part out."""
        def fn(*rest):
            return self._L.plsa_lda_refit(self._h, float(doc_topic_prior), *rest)
        return self._lda_drive(fn, n_iter, n_iter_per_test, tolerance, doc_iter, e_step_thresh, flags, trace)

    def lda_bound(self, doc_topic_prior, topic_word_prior=None):
        """The variational bound of the state in force (float64); topic_word_prior=None leaves the topic part out."""
        out = C.c_double(0.0)
        eta = 1.0 if topic_word_prior is None else float(topic_word_prior)
        self._ok(self._L.plsa_lda_bound(self._h, float(doc_topic_prior), eta, 0 if topic_word_prior is None else 1, C.byref(out)))
        return out.value

    def lda_tables(self):
        """(A [n, k], B [k, m]): the exp-digamma tables an LDA iteration forms from the state in force, which stays as it is
        (diagnostics / tests)."""
        n, m, _ = self.shape
        A, B = np.empty((n, self.k), np.float32), np.empty((self.k, m), np.float32)
        self._ok(self._L.plsa_lda_tables(self._h, ptr(A), ptr(B)))
        return A, B

    # -- LDA with a vector document-topic prior and learned priors (enstop_amd/include/plsa_hip_lda_priors.h) -----------------
    def _prior_vector(self, doc_topic_prior):
        alpha = np.ascontiguousarray(doc_topic_prior, np.float64).copy()
        if alpha.shape != (self.k,):
            raise ValueError("doc_topic_prior has shape %s, expected (%d,)" % (alpha.shape, self.k))
        return alpha

    def lda_prior_fit(self, doc_topic_prior, topic_word_prior, learn=3, prior_start=20, prior_every=1, n_iter=100,
                      n_iter_per_test=10, tolerance=0.001, doc_iter=1, e_step_thresh=1e-32, flags=None, trace=False):
        """lda_fit with doc_topic_prior a vector [k] and with priors that are re-estimated behind the iterations prior_start,
        prior_start + prior_every, ... (counted from 1) by maximising the bound over them: learn bit 0 alpha, bit 1 eta, 0
        neither.  Returns (iterations, trace, alpha [k], eta): the priors in force at the end.  A due test of the bound cannot
        stop the loop before the first update.  lda_fit's refusals, and prior_start < 1, prior_every < 1."""
        alpha = self._prior_vector(doc_topic_prior)
        eta = C.c_double(float(topic_word_prior))

        def fn(*rest):
            return self._L.plsa_lda_prior_fit(self._h, ptr(alpha), C.byref(eta), int(learn), int(prior_start), int(prior_every),
                                              *rest)
        iters, bound = self._lda_drive(fn, n_iter, n_iter_per_test, tolerance, doc_iter, e_step_thresh, flags, trace)
        return iters, bound, alpha, eta.value

    def lda_prior_refit(self, doc_topic_prior, n_iter=50, n_iter_per_test=10, tolerance=0.005, doc_iter=1, e_step_thresh=1e-32,
                        flags=None, trace=False):
        """lda_refit under a vector prior [k]: only gamma moves, nothing is learned."""
        alpha = self._prior_vector(doc_topic_prior)

        def fn(*rest):
            return self._L.plsa_lda_prior_refit(self._h, ptr(alpha), *rest)
        return self._lda_drive(fn, n_iter, n_iter_per_test, tolerance, doc_iter, e_step_thresh, flags, trace)

    def lda_prior_bound(self, doc_topic_prior, topic_word_prior=None):
        """lda_bound under a vector prior [k]."""
        alpha = self._prior_vector(doc_topic_prior)
        out = C.c_double(0.0)
        eta = 1.0 if topic_word_prior is None else float(topic_word_prior)
        self._ok(self._L.plsa_lda_prior_bound(self._h, ptr(alpha), eta, 0 if topic_word_prior is None else 1, C.byref(out)))
        return out.value

    def lda_prior_stats(self):
        """(t_doc [k], t_topic [k]) float64: sum_d (psi(gamma_dz) - psi(S_d)) and sum_w (psi(lambda_zw) - psi(S_z)) of the state
        in force, the sums a prior update maximises over (diagnostics / tests)."""
        t_doc, t_topic = np.zeros(self.k, np.float64), np.zeros(self.k, np.float64)
        self._ok(self._L.plsa_lda_prior_stats(self._h, ptr(t_doc), ptr(t_topic)))
        return t_doc, t_topic

    # -- doc-sharded fit building blocks ---------------------------------------------------------------
    def em_accumulate(self, sample_weight=None, e_step_thresh=1e-32, want_ll=False, materialised=False):
        """materialised: the reference's kernel sequence over this context's rows (E-step into P(z|w,d), M-step from it)
        instead of the fused passes -- one doc block of a tiled materialised iteration (plsa_em_accumulate_materialised)."""
        sw = None if sample_weight is None else _f32(sample_weight)
        ll = C.c_double(0.0)
        fn = self._L.plsa_em_accumulate_materialised if materialised else self._L.plsa_em_accumulate
        self._ok(fn(self._h, ptr(sw), np.float32(e_step_thresh), C.addressof(ll) if want_ll else None))
        return ll.value if want_ll else None

    def p_bytes(self):
        """bytes of P(z|w,d) for the active matrix and the factors in force (one tile of slack included)"""
        n, m, nnz = self.shape
        return 4 * (nnz + 64) * ((self.k + 3) // 4 * 4)

    def set_p_budget(self, nbytes=0):
        """Bytes P(z|w,d) may take in fit / refit in the reference arithmetic (plsa_set_p_budget; 0 or None: no budget): the
        documents are then walked in blocks that fit, with the same bits as the unblocked step.  No effect on the default
        arithmetic (its fused schedule stores no P) nor on e_step / m_step / set_p, which hand the whole array in or out."""
        self._ok(self._L.plsa_set_p_budget(self._h, int(nbytes or 0)))
        self.p_budget = int(nbytes or 0)
        return self

    def p_block_info(self):
        """Of the last reference-arithmetic iteration of fit / refit (plsa_p_block_info): the budget in force, the blocks it ran
        in, the non-zeros of the largest block, the bytes allocated for P(z|w,d)."""
        a, b, c_, d = C.c_int64(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
        self._ok(self._L.plsa_p_block_info(self._h, C.byref(a), C.byref(b), C.byref(c_), C.byref(d)))
        return dict(budget=a.value, blocks=b.value, largest_block_nnz=c_.value, p_allocated_bytes=d.value)

    def p_reserve(self, nbytes):
        """own P(z|w,d) capacity of at least nbytes; returns its device address (for p_borrow on other contexts)"""
        out = C.c_void_p()
        self._ok(self._L.plsa_p_reserve(self._h, int(nbytes), C.byref(out)))
        return out.value

    def p_borrow(self, device_ptr, nbytes=0):
        """use another context's P(z|w,d) buffer (None: back to own allocations); sharers run one after the other"""
        self._ok(self._L.plsa_p_borrow(self._h, device_ptr, int(nbytes)))

    def em_finish(self):
        self._ok(self._L.plsa_em_finish(self._h))

    def set_sample_weight(self, sample_weight=None):
        """Make the document weights resident on the device (None: clear): later calls that pass no weights use
        them without a host copy -- the per-iteration calls of the doc-sharded loop stay enqueue-only."""
        sw = None if sample_weight is None else _f32(sample_weight)
        self._ok(self._L.plsa_set_sample_weight(self._h, ptr(sw)))

    def accumulator_device(self):
        p, n = C.c_void_p(), C.c_int64(0)
        self._ok(self._L.plsa_accumulator_device(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def accumulator_get(self):
        _, n = self.accumulator_device()
        out = np.empty(n, np.float32)
        self._ok(self._L.plsa_accumulator_get(self._h, out))
        return out

    def accumulator_set(self, a):
        self._ok(self._L.plsa_accumulator_set(self._h, _f32(a)))

    # -- multi-GPU exchange (RCCL through the C ABI; see comm.py) ------------------------------------------
    def comm_init(self, id_bytes, rank, world):
        if len(id_bytes) != 128:
            raise ValueError("the RCCL unique id has 128 bytes")
        self._ok(self._L.plsa_comm_init(self._h, bytes(id_bytes), int(rank), int(world)))

    def comm_destroy(self):
        self._ok(self._L.plsa_comm_destroy(self._h))

    def comm_info(self):
        r, w = C.c_int32(0), C.c_int32(1)
        self._ok(self._L.plsa_comm_info(self._h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def comm_barrier(self):
        self._ok(self._L.plsa_comm_barrier(self._h))

    def stack_reserve(self, slots, k, m):
        """Device block [slots][k][m] for the topic matrices of the members this process fits; returns its
        device address (slot s lives at base + 4 * s * k * m)."""
        base = C.c_void_p()
        self._ok(self._L.plsa_stack_reserve(self._h, int(slots), int(m), int(k), C.byref(base)))
        return int(base.value)

    def comm_allgather_stack(self, slots, k, m, copy=True, out=None):
        """[slots * world, k, m] float32 in run order (run r = slot r // world of rank r % world): one grouped
        ncclAllGather, then ONE device-to-host copy -- straight into `out` (a C-contiguous float32 array of that size the
        caller re-uses), into a fresh array (copy=True), or into the engine's page-locked buffer of which a VIEW is
        returned (copy=False: overwritten by the next call on this engine)."""
        _, world = self.comm_info()
        shape = (int(slots) * world, int(k), int(m))
        if out is None and copy:
            out = np.empty(shape, np.float32)
        if out is not None:
            if out.dtype != np.float32 or not out.flags.c_contiguous or out.size != shape[0] * shape[1] * shape[2]:
                raise ValueError("out must be a C-contiguous float32 array of %d elements" % (shape[0] * shape[1] * shape[2]))
            self._ok(self._L.plsa_comm_allgather_stack_to(self._h, int(slots), int(m), int(k), out.reshape(-1)))
            return out.reshape(shape)
        p = C.POINTER(C.c_float)()
        self._ok(self._L.plsa_comm_allgather_stack(self._h, int(slots), int(m), int(k), C.byref(p)))
        return np.ctypeslib.as_array(p, shape=shape)

    def comm_allgather_host(self, a):
        a = np.ascontiguousarray(a)
        _, world = self.comm_info()
        out = np.empty((world,) + a.shape, a.dtype)
        self._ok(self._L.plsa_comm_allgather_host(self._h, a.ctypes.data, a.nbytes, out.ctypes.data))
        return out

    def comm_allreduce_f64(self, values, op="sum"):
        a = np.atleast_1d(np.array(values, dtype=np.float64))
        self._ok(self._L.plsa_comm_allreduce_f64(self._h, a, a.size, {"sum": 0, "max": 1}[op]))
        return a

    def comm_broadcast_host(self, a, root=0):
        a = np.array(a, copy=True, order="C")
        self._ok(self._L.plsa_comm_broadcast_host(self._h, a.ctypes.data, a.nbytes, int(root)))
        return a

    def allreduce_accumulator(self):
        self._ok(self._L.plsa_allreduce_accumulator(self._h))

    def all_pairs_hellinger(self, topics):
        """[t, t] float64 Hellinger distances between the rows of `topics` [t, m] (enstop_.py:258-266)."""
        T = _f32(topics)
        if T.ndim != 2:
            raise ValueError("topics must be a 2-D array")
        t, m = T.shape
        D = np.empty((t, t), np.float64)
        self._ok(self._L.plsa_all_pairs_hellinger(self._h, ptr(T), t, m, D))
        return D

    def all_pairs_kl(self, topics):
        """[t, t] float64 KL(topic i || topic j) in bits (enstop_.py:234-253)."""
        T = _f32(topics)
        if T.ndim != 2:
            raise ValueError("topics must be a 2-D array")
        t, m = T.shape
        D = np.empty((t, t), np.float64)
        self._ok(self._L.plsa_all_pairs_kl(self._h, ptr(T), t, m, D))
        return D

    def cluster_representatives(self, topics, labels, weights=None):
        """Stable topic of every cluster (enstop_.py:299-308, 385-393): [n_clusters, m] float32."""
        T = _f32(topics)
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        t, m = T.shape
        if lab.shape != (t,):
            raise ValueError("labels must have one entry per topic")
        n_clusters = int(lab.max()) + 1 if lab.size and lab.max() >= 0 else 0
        out = np.empty((n_clusters, m), np.float32)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        self._ok(self._L.plsa_cluster_representatives(self._h, ptr(T), t, m, lab, ptr(w), n_clusters, out))
        return out

    def codocument_counts(self, words, max_sets_per_pass=0):
        """Co-document counts of word lists on the ACTIVE matrix (include/plsa_hip_metrics.h; enstop/utils.py:150-203).
        words: int [sets, nw], 2 <= nw <= 32, distinct ids per row.  -> (co [sets, nw, nw] int64: documents with a stored
        entry in both columns, the diagonal the column's stored entries; positive [sets, nw] int64: entries > 0).  Exact.
        max_sets_per_pass: cap of the sets whose document masks are held at once (0: chosen from the free memory)."""
        W = np.ascontiguousarray(words, dtype=np.int32)
        if W.ndim != 2:
            raise ValueError("words must be a 2-D array [sets, nw]")
        sets, nw = W.shape
        co = np.zeros((sets, nw, nw), np.int64)
        positive = np.zeros((sets, nw), np.int64)
        self._ok(self._L.plsa_codocument_counts(self._h, W.reshape(-1), sets, nw, int(max_sets_per_pass), co.reshape(-1),
                                                positive.reshape(-1)))
        return co, positive

    # -- the embedding of topic_combination="hellinger_umap" (include/plsa_hip_embed.h; enstop_.py:354-414) ------------
    def knn_membership(self, D, n_neighbors):
        """Nearest neighbours, bandwidths and directed membership strengths of a precomputed distance matrix D [t, t]
        (UMAP's first stage), one kernel launch.  n_neighbors counts the row's own entry and is capped at t - 1.
        -> (idx [t, k] int32: the k smallest entries of each row, ascending, ties towards the lower column;
        dist [t, k] float32; rho [t]; sigma [t]; member [t, k] float32)."""
        D = np.ascontiguousarray(D, dtype=np.float64)
        if D.ndim != 2 or D.shape[0] != D.shape[1]:
            raise ValueError("D must be a square distance matrix")
        t = D.shape[0]
        if t < 2:
            raise ValueError("an embedding needs at least 2 points, got %d" % t)
        if int(n_neighbors) < 1:
            raise ValueError("n_neighbors must be at least 1")
        k = min(int(n_neighbors), t - 1)
        idx = np.empty((t, k), np.int32)
        dist, member = np.empty((t, k), np.float32), np.empty((t, k), np.float32)
        rho, sigma = np.empty(t, np.float32), np.empty(t, np.float32)
        self._ok(self._L.plsa_knn_membership(self._h, D.reshape(-1), t, k, idx.reshape(-1), dist.reshape(-1), rho, sigma,
                                             member.reshape(-1)))
        return idx, dist, rho, sigma, member

    _LAYOUT_PATHS = {"auto": 0, "lds": 1, "epoch": 2, 0: 0, 1: 1, 2: 2}
    last_layout_path = None        # layout: "lds" | "epoch"
    last_embedding_info = None     # hellinger_embedding

    def layout(self, W_csr, init, n_epochs=None, a=None, b=None, negative_sample_rate=5, seed=0, path="auto"):
        """The force layout of the symmetric fuzzy graph W_csr [t, t] from the positions init [t, dim]: synchronous and
        deterministic (every vertex reads the epoch's starting positions and moves once), a function of the inputs and
        `seed`.  n_epochs: 500 up to 10 000 vertices, else 200; a, b: from min_dist = 0.1, spread = 1.
        path: "auto" | "lds" (1: one persistent workgroup, positions in LDS; DeviceError when 2 * t * dim * 4 bytes exceed
        64 KiB) | "epoch" (2: one launch per epoch); both give the same bits.  -> [t, dim] float32; the path taken is in
        `last_layout_path`."""
        from . import embedding
        import scipy.sparse as sp
        W = sp.csr_matrix(W_csr)
        W.sort_indices()
        Y = np.array(init, dtype=np.float32, order="C", copy=True)
        if Y.ndim != 2 or W.shape != (Y.shape[0], Y.shape[0]):
            raise ValueError("init must be [t, dim] for a [t, t] graph")
        t, dim = Y.shape
        if path not in self._LAYOUT_PATHS:
            raise ValueError('path must be "auto", "lds" (1) or "epoch" (2)')
        if a is None or b is None:
            a, b = embedding.find_ab_params()
        n_epochs = embedding.default_n_epochs(t) if n_epochs is None else int(n_epochs)
        code = self._LAYOUT_PATHS[path]
        self._ok(self._L.plsa_layout(self._h, np.ascontiguousarray(W.indptr, np.int32), np.ascontiguousarray(W.indices, np.int32),
                                     np.ascontiguousarray(W.data, np.float32), t, dim, Y.reshape(-1), n_epochs, float(a), float(b),
                                     int(negative_sample_rate), int(seed) & 0xFFFFFFFFFFFFFFFF, code))
        self.last_layout_path = "epoch" if code == 2 or (code == 0 and 2 * t * dim * 4 > 65536) else "lds"
        return Y

    def hellinger_embedding(self, topics, n_neighbors=15, n_components=5, seed=0):
        """UMAP of the rows of `topics` [t, m] under the Hellinger distance, natively (enstop_.py:354-414 calls
        umap.UMAP(n_neighbors, n_components, metric="hellinger")): all_pairs_hellinger -> knn_membership -> the symmetric
        fuzzy graph, its schedule and the initial layout on the host (embedding.py) -> layout.  -> [t, n_components]
        float32; `last_embedding_info` says what was done."""
        from . import embedding
        D = self.all_pairs_hellinger(topics)
        t = D.shape[0]
        idx, _, _, _, member = self.knn_membership(D, n_neighbors)
        n_epochs = embedding.default_n_epochs(t)
        W = embedding.prune_for_schedule(embedding.fuzzy_graph(idx, member), n_epochs)
        Y0, init, components = embedding.initial_layout(W, int(n_components), seed)
        Y = self.layout(W, Y0, n_epochs=n_epochs, negative_sample_rate=embedding.NEGATIVE_SAMPLE_RATE, seed=seed)
        self.last_embedding_info = dict(t=t, n_neighbors=idx.shape[1], components=components, init=init, n_epochs=n_epochs,
                                        edges=int(W.nnz), path=self.last_layout_path)
        return Y

    def reference_chain_info(self):
        """norm_pwz of the reference arithmetic (plsa_reference_chain_info): chunks of the parity-pair walk that took the slow way,
        chunks walked, and whether this context is on the serial chain for the current corpus."""
        a, b, c_ = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        self._ok(self._L.plsa_reference_chain_info(self._h, C.byref(a), C.byref(b), C.byref(c_)))
        return dict(slow_chunks=a.value, chunks=b.value, serial_chain_now=bool(c_.value))

    def placement_info(self):
        n, a, b = C.c_int32(0), C.c_double(0.0), C.c_double(0.0)
        self._ok(self._L.plsa_placement_info(self._h, C.byref(n), C.byref(a), C.byref(b)))
        return dict(candidates=n.value, kept_fill_GBps=round(a.value, 1), worst_fill_GBps=round(b.value, 1))

    def balance_info(self):
        """Column-pass schedule of the current structure: measured chunk boundaries per XCD, per-XCD finish times of
        the last timed launch, timed launches spent, item length, number of items."""
        lo = (C.c_int32 * 9)(); t = (C.c_double * 8)()
        n, seg, items = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        self._ok(self._L.plsa_schedule_info(self._h, lo, t, C.byref(n), C.byref(seg), C.byref(items)))
        return dict(xcd_chunk_boundaries=list(lo), xcd_finish_us=[round(v, 1) for v in t], timed_launches=n.value,
                    item_entries=seg.value, n_items=items.value)

    def packed_info(self):
        """Index stream of each fused pass for the current structure: 'packed', 'arrays' or None (not built yet)."""
        a, b = C.c_int32(0), C.c_int32(0)
        self._ok(self._L.plsa_packed_info(self._h, C.byref(a), C.byref(b)))
        name = {1: "packed", 0: "arrays", -1: None}
        return dict(csr=name[a.value], csc=name[b.value])

    def pass_info(self):
        """Instantiation each fused pass takes for the factors in force: lane shape (lpn, ch, full) of the column pass
        (the E-step and the log-likelihood share it) and of the document pass, and whether each gathers with 64-bit
        row addresses (a wide pass runs the run-time-kp instantiation whatever `full` says)."""
        col, row, wide = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(2, np.int32)
        self._ok(self._L.plsa_pass_info(self._h, col, row, wide))
        return dict(col=(int(col[0]), int(col[1]), bool(col[2])), row=(int(row[0]), int(row[1]), bool(row[2])),
                    row_wide=bool(wide[0]), col_wide=bool(wide[1]))

    def fit_info(self):
        """How the last fit / refit on this engine ran: fused loop, pipelined (two event-linked streams), speculated (an
        iteration enqueued ahead of an unread likelihood test), hipGraph launches, column tail ('sweep': k_col_reduce_norm,
        'four_kernels': the doc-sharded form, None: none ran), two-stage norm_pwz, XCD split of the last column pass.  The
        last three are written by the column pass and its tail, so after m_step they describe that call's."""
        a = np.zeros(7, np.int32)
        self._ok(self._L.plsa_fit_info(self._h, a))
        return dict(fused=bool(a[0]), pipelined=bool(a[1]), speculated=bool(a[2]), graph_launches=int(a[3]),
                    col_tail={0: None, 1: "sweep", 2: "four_kernels"}[int(a[4])], two_stage_norm=bool(a[5]),
                    xcd_split=bool(a[6]))

    def release_scratch(self):
        """Free the materialised P and other large scratch buffers (re-created on demand), and the buffers of the cached
        member batch."""
        if self._member_batch is not None:
            self._member_batch.release()
        self._ok(self._L.plsa_release_scratch(self._h))

    def member_capacity(self, k):
        """members of k topics over the resident corpus that fit into half of the free HBM (at most 64)"""
        out = C.c_int32(0)
        self._ok(self._L.plsa_members_capacity(self._h, int(k), C.byref(out)))
        return out.value

    def member_batch(self, n_members):
        """The engine's cached MemberBatch with at least `n_members` slots (grown by re-creation when too small)."""
        b = self._member_batch
        if b is None or b.n_members < n_members:
            if b is not None:
                b.close()
            b = self._member_batch = MemberBatch(self, n_members)
        return b

    # -- measurement ---------------------------------------------------------------------------------
    def timing(self, on=True):
        self._ok(self._L.plsa_timing_enable(self._h, int(on)))
        self.timing_on = bool(on)

    def timing_reset(self):
        self._ok(self._L.plsa_timing_reset(self._h))

    def timing_get(self, prefix):
        ms, n = C.c_double(0.0), C.c_int64(0)
        self._ok(self._L.plsa_timing_get(self._h, prefix.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def stream_bandwidth(self, nbytes=1 << 32, kind=0, reps=5):
        """GB/s of a fill (kind 0 non-temporal, 1 plain) or copy (2) over `nbytes` of scratch HBM."""
        out = C.c_double(0.0)
        self._ok(self._L.plsa_measure_stream_bandwidth(self._h, int(nbytes), int(kind), int(reps), C.byref(out)))
        return out.value

    def timing_report(self):
        buf = C.create_string_buffer(8192)
        self._ok(self._L.plsa_timing_report(self._h, buf, 8192))
        out = {}
        for line in buf.value.decode().splitlines():
            name, cnt, ms = line.rsplit(" ", 2)
            out[name] = (int(cnt), float(ms))
        return out


class _MemberView(Engine):
    """A batch member's own context, borrowed from its MemberBatch: the read-only reports and read-backs of Engine
    (shape, get_factors, pass_info, packed_info, balance_info) apply to it; it is never closed from here."""

    def __init__(self, leader, handle):
        self._L = leader._L
        self._h = handle
        self.device = leader.device
        self.k = 0
        self.base_rows = leader.base_rows
        self.lock = leader.lock
        self._member_batch = None

    def close(self):
        self._h = C.c_void_p()


class MemberBatch:
    """Up to 64 ensemble members (bootstrap resamples of the corpus resident on `eng`) that advance through the fused EM
    schedule together, every kernel of an iteration launched once for all of them (include/plsa_hip_members.h, DESIGN.md
    section 10).  Each member is bit-identical to its standalone fit; the likelihood test is per member.

        batch = MemberBatch(eng, 32)
        for r in range(32):
            batch.prepare(r, k, idx=idx_r, rng=rng_r)        # or U=..., V=... (host factors)
        iters, traces = batch.fit(32, n_iter=50, trace=True)
        batch.copy_components(r, stack_dst)                  # or batch.components(r)
    """

    def __init__(self, eng, n_members):
        if not 1 <= int(n_members) <= _lib.MEMBERS_MAX:
            raise ValueError("a batch holds 1 to %d members, not %r" % (_lib.MEMBERS_MAX, n_members))
        self.eng = eng
        self._L = eng._L
        self._b = C.c_void_p()
        self.n_members = int(n_members)
        self.k = 0
        self.last_batched = 0
        eng._ok(self._L.plsa_members_create(eng._h, self.n_members, C.byref(self._b)))

    def close(self):
        if getattr(self, "_b", None) is not None and self._b.value:
            if self.eng._h.value:                  # (a batch dies with its engine: Engine.close closes it first)
                self._L.plsa_members_destroy(self._b)
            self._b = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def release(self):
        """free the members' device buffers (the slots stay usable)"""
        self.eng._ok(self._L.plsa_members_release(self._b))

    def prepare(self, member, k, idx=None, rng=None, U=None, V=None):
        """member := corpus[idx] (None: the corpus itself) with k topics drawn on the device from `rng` (a legacy
        RandomState, advanced exactly as plsa_init(random) advances it) or taken from the host factors U [n, k], V [k, m]."""
        ip = None
        n_out = 0
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.int64)
            ip, n_out = idx.ctypes.data, idx.shape[0]
        if rng is not None:
            state, put_back = _mt19937_state(rng)
            self.eng._ok(self._L.plsa_members_prepare(self._b, int(member), ip, n_out, int(k), state.ctypes.data, None, None))
            put_back()
        else:
            U, V = _f32(U), _f32(V)
            if U.ndim != 2 or V.ndim != 2 or U.shape[1] != int(k) or V.shape[0] != int(k):
                raise ValueError("host factors must be U [n, k] and V [k, m]")
            self.eng._ok(self._L.plsa_members_prepare(self._b, int(member), ip, n_out, int(k), None, ptr(U), ptr(V)))
        self.k = int(k)

    def fit(self, n_active=None, n_iter=100, n_iter_per_test=10, tolerance=0.001, e_step_thresh=1e-32, flags=None, trace=False):
        """-> (iteration count per member [n_active], list of float32 likelihood traces); `last_batched`: how many of the
        members went through batched launches (the others through the classic loop: same results)."""
        n_active = self.n_members if n_active is None else int(n_active)
        flags = default_flags() if flags is None else int(flags)
        if trace:
            flags |= PLSA_TRACE_LL
        cap = int(n_iter) + 2
        iters, nll = np.zeros(n_active, np.int32), np.zeros(n_active, np.int32)
        ll = np.zeros((n_active, cap), np.float32)
        nb = C.c_int32(0)
        self.eng._ok(self._L.plsa_members_fit(self._b, n_active, int(n_iter), int(n_iter_per_test), float(tolerance),
                                              np.float32(e_step_thresh), flags, iters, ll.ctypes.data, cap, nll, C.byref(nb)))
        self.last_batched = nb.value
        return iters, [ll[r, :nll[r]].copy() for r in range(n_active)]

    def copy_components(self, member, device_ptr):
        self.eng._ok(self._L.plsa_members_copy_components(self._b, int(member), int(device_ptr)))

    def member(self, member):
        """the member's context as a borrowed Engine view (get_factors, shape, pass_info, packed_info, ...)"""
        h = C.c_void_p()
        self.eng._ok(self._L.plsa_members_context(self._b, int(member), C.byref(h)))
        view = _MemberView(self.eng, h)
        view.k = self.k
        return view

    def components(self, member):
        """P(w|z) [k, m] of a member on the host"""
        return self.member(member).get_factors(want_u=False)[1]

    def last_ll(self, member):
        """the float64 log-likelihood behind the member's last likelihood test (the traces hold float32, like the reference)"""
        out = C.c_double(0.0)
        self.eng._ok(self._L.plsa_members_last_ll(self._b, int(member), C.byref(out)))
        return out.value

    def info(self, member):
        """how the member ran in the last fit: launch group (-1: classic loop), members in the group, row items in use and
        their length, chunk rows of the column pass, heavy columns, document-pass grid, first norm stage's grid"""
        a = np.zeros(8, np.int32)
        self.eng._ok(self._L.plsa_members_info(self._b, int(member), a))
        keys = ("group", "group_size", "row_items", "row_item_entries", "col_chunks", "heavy_columns", "row_grid", "norm_blocks")
        out = dict(zip(keys, (int(v) for v in a)))
        out["row_items"] = bool(out["row_items"])
        return out


_engines = {}


def get_engine(device=None):
    """Process-wide Engine per device (buffers are reused across fits)."""
    dev = default_device() if device is None else int(device)
    eng = _engines.get(dev)
    if eng is None:
        eng = _engines[dev] = Engine(dev)
    return eng


_member_engines = {}


def get_member_engines(device=None, jobs=1):
    """`jobs` engines on one device for ensemble members fitted concurrently (each context has its own
    HIP streams and buffers): the process-wide engine of the device first, then cached extra ones."""
    first = get_engine(device)
    extra = _member_engines.setdefault(first.device, [])
    while len(extra) < jobs - 1:
        extra.append(Engine(first.device))
    return [first] + extra[:max(jobs - 1, 0)]


def reset_engines():
    """Close the cached per-device engines (tools / tests that change PLSA_* knobs, which a context
    reads when it is created)."""
    for eng in list(_engines.values()):
        eng.close()
    _engines.clear()
    for lst in _member_engines.values():
        for eng in lst:
            eng.close()
    _member_engines.clear()


def host_normalize_rows(a):
    """enstop/utils.py:8-41 normalize(a, axis=1), in place on a C-contiguous float64 array."""
    L = _lib.load()
    assert a.dtype == np.float64 and a.flags.c_contiguous and a.ndim == 2
    L.plsa_host_normalize_rows(a, a.shape[0], a.shape[1])
    return a
