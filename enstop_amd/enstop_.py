"""Ensemble of bootstrapped pLSA fits on MI355X behind the reference's interface
(enstop/enstop_.py:56-115 plsa_topics, :164-231 ensemble_of_topics).

The reference fans the members out over dask/joblib *threads* of one process.  Here a member is one
fit on one GPU: within a process the members assigned to it run back to back on its device (the
corpus is uploaded once, each bootstrap resample is a device-side row gather); across GPUs the
launcher starts one process per device (torchrun); every member's topics go into the process' device stack and the
stacks are all-gathered over RCCL (`distributed.gather_stack`).  Members are dealt round-robin, run r -> rank r mod world_size, and
each member draws from its own RandomState stream so the stack does not depend on the device count.
"""
import numpy as np
from scipy.sparse import issparse, csr_matrix
from sklearn.utils import check_random_state

import os
import threading

from ._driver import apply_init_slot, plan_init, resolve_flags
from .engine import get_engine, get_member_engines
from .plsa import _fit_on_engine, _locked

# A corpus this small leaves most of the GPU idle during one fit (0.15 ms per EM iteration at the 20NG
# shape, a handful of short dependent kernels): members are then fitted concurrently, like the reference's
# thread pool of nogil fits (enstop_.py:209-217).  Measured on MI355X, 32 members x 50 iterations on the
# 20NG-shaped corpus: 4960 fits/min with one member at a time, 7050 with two, 7470 with three, flat beyond
# (profiles/r02_ensemble_concurrent_members_cfg1.jsonl); config 2 (10 M nnz) +22 %; nothing to gain once a
# single fit saturates the memory system.  Round 4: the member contexts need their own hardware queues (libplsa_hip.so asks
# for 8 at load time, see include/plsa_hip.h): 7 370-7 520 -> 8 070-8 290 fits/min with four members in flight; six or eight
# in flight are slower (profiles/r04_hw_queues_api_jobs_6_8.txt), hence the cap (ENSTOP_AMD_CONCURRENT_MEMBERS_MAX: experiments).
# The GPU-native counterpart of that thread pool is ONE launch chain that carries all members: parallelism="batched"
# (`_fit_members_batched` below); opt-in, the contexts stay the default.
CONCURRENT_MEMBERS_MAX = int(os.environ.get("ENSTOP_AMD_CONCURRENT_MEMBERS_MAX", "4"))
CONCURRENT_MEMBERS_CELLS = float(os.environ.get("ENSTOP_AMD_CONCURRENT_MEMBERS_CELLS", "2e9"))   # nnz * k below which members run concurrently


def _member_flags(kwargs):
    """`flags=` and / or `arithmetic=` of plsa_topics / ensemble_of_topics -> the flags of the members' fits"""
    return resolve_flags(kwargs.get("flags", None), kwargs.get("arithmetic", None))


def concurrent_members(nnz, k, n_jobs):
    if n_jobs is None or n_jobs < 1 or nnz * float(k) >= CONCURRENT_MEMBERS_CELLS:
        return 1
    return int(min(n_jobs, CONCURRENT_MEMBERS_MAX))


last_ensemble_timing = {}      # seconds spent by the last multi-member call of this process (bench.py reports it);
                               # path: "batched" | "contexts", batch: members per launch, groups: launch groups per batch

PARALLELISM = ("dask", "joblib", "none", "batched")


def _batched_requested(parallelism):
    """parallelism="batched", or ENSTOP_AMD_ENSEMBLE=batched for the reference's "dask" / "joblib" (A/B measurement through
    unmodified callers)."""
    return parallelism == "batched" or (parallelism in ("dask", "joblib") and
                                        os.environ.get("ENSTOP_AMD_ENSEMBLE", "") == "batched")


def batch_members_cap():
    """ENSTOP_AMD_BATCH_MEMBERS: members per launch (default 32, at most 64)"""
    from ._lib import MEMBERS_MAX
    return max(1, min(MEMBERS_MAX, int(os.environ.get("ENSTOP_AMD_BATCH_MEMBERS", "32"))))


def _batch_eligible(eng, A, k, member_kw):
    """What a batch carries: the fused schedule in the engine's own arithmetic, eager and untimed, on a corpus small
    enough that one fit leaves the GPU idle.  Everything else takes the contexts (same results)."""
    from ._lib import PLSA_FUSED, PLSA_GRAPH, PLSA_REFERENCE_LL, PLSA_REFERENCE_SUMS, PLSA_SHARDED
    flags = resolve_flags(member_kw.get("flags"))
    if not flags & PLSA_FUSED or flags & (PLSA_REFERENCE_SUMS | PLSA_REFERENCE_LL | PLSA_SHARDED | PLSA_GRAPH):
        return False
    if os.environ.get("PLSA_GRAPH", "0") not in ("", "0") or getattr(eng, "timing_on", False):
        return False
    if A.nnz * float(k) >= CONCURRENT_MEMBERS_CELLS or A.nnz == 0:
        return False
    init = member_kw.get("init", "random")
    if isinstance(init, str) and init == "device_random":
        return False
    return member_kw.get("n_iter", 100) > 0


def _bootstrap_rows(n_base, bootstrap, random_state):
    """The member's resample of the corpus rows, the first draw of its stream (enstop_.py:86-87); None: the corpus itself"""
    return check_random_state(random_state).randint(0, n_base, size=n_base) if bootstrap else None


def _prepare_member(batch, j, eng, k, bootstrap=True, random_state=None, init="random", **_unused):
    """What `_member_on_engine` does before its fit, for slot j of a batch: the bootstrap draw, then the same stream into
    the initialisation plsa_fit would choose (_driver.plan_init)."""
    idx = _bootstrap_rows(eng.base_rows, bootstrap, random_state)
    plan = plan_init(eng.base_rows, batch.eng.shape[1], k, init, check_random_state(random_state))
    apply_init_slot(batch, j, k, plan, idx)


def _fit_members_batched(eng, A, k, runs, seeds, member_kw, world, n_runs, B, slots_wanted=0):
    """The batched branch of `_fit_members`: the runs of this rank in successive batches of at most B members, each batch
    one launch chain (engine.MemberBatch); run r draws from RandomState(seeds[r]) and lands in slot r // world."""
    m = A.shape[1]
    slots = max(1, max((r // world for r in runs), default=0) + 1) if n_runs is None else max(1, (n_runs + world - 1) // world)
    base = eng.stack_reserve(slots, k, m)
    batch = eng.member_batch(max(B, slots_wanted))       # (idle slots cost nothing; a later, larger ensemble re-uses them)
    groups = []
    for start in range(0, len(runs), B):
        chunk = runs[start:start + B]
        for j, r in enumerate(chunk):
            _prepare_member(batch, j, eng, k, random_state=np.random.RandomState(seeds[r]), **member_kw)
        batch.fit(len(chunk), member_kw["n_iter"], member_kw["n_iter_per_test"], member_kw["tolerance"],
                  member_kw["e_step_thresh"], member_kw["flags"])
        for j, r in enumerate(chunk):
            batch.copy_components(j, base + 4 * (r // world) * k * m)
        sizes = {}
        for j in range(len(chunk)):
            g = batch.info(j)["group"]
            sizes[g if g >= 0 else -1 - j] = sizes.get(g if g >= 0 else -1 - j, 0) + 1
        groups.append(sorted(sizes.values(), reverse=True))
    last_ensemble_timing.update(groups=groups)
    return eng


def _fit_members(A, k, runs, seeds, member_kw, device, n_jobs, world=1, n_runs=None, batched=0):
    """Fits the given runs of an ensemble on this process' GPU and leaves their topic matrices in the device
    stack of the process-wide engine (run r -> slot r // world); run r draws from RandomState(seeds[r]) whichever
    engine or thread fits it, so the result does not depend on `n_jobs`.  Returns the engine that holds the stack.
    `batched` ((members per launch, slots to keep) or 0: off): the runs go through one launch chain per batch instead of `n_jobs` contexts."""
    if batched:
        return _fit_members_batched(get_engine(device), A, k, runs, seeds, member_kw, world, n_runs, batched[0], batched[1])
    jobs = min(concurrent_members(A.nnz, k, n_jobs), max(len(runs), 1))
    engines = get_member_engines(device, jobs)
    for e in engines[1:]:
        e.upload_csr(A)                  # (the first one holds the corpus already; uploading inside the worker threads
                                         #  instead measured no better: 9 130 against 8 950 fits/min at the 20NG shape)
    m = A.shape[1]
    # every rank reserves the same number of slots (the all-gather is slot by slot), filled or not
    slots = max(1, max((r // world for r in runs), default=0) + 1) if n_runs is None else max(1, (n_runs + world - 1) // world)
    base = engines[0].stack_reserve(slots, k, m)
    errors = []

    def work(j):
        try:
            for r in runs[j::jobs]:
                _member_on_engine(engines[j], k, random_state=np.random.RandomState(seeds[r]),
                                  stack_dst=base + 4 * (r // world) * k * m, **member_kw)
        except BaseException as e:       # re-raised in the caller's thread
            errors.append(e)
    if jobs == 1:
        work(0)
    else:
        threads = [threading.Thread(target=work, args=(j,)) for j in range(jobs)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    if errors:
        raise errors[0]
    return engines[0]


def _member_on_engine(eng, k, bootstrap=True, random_state=None, init="random", n_iter=100,
                      n_iter_per_test=10, tolerance=0.001, e_step_thresh=1e-16, flags=None, stack_dst=None):
    """One ensemble member on a corpus already uploaded to `eng`; returns P(w|z) [k, m] -- or, with
    `stack_dst` (a device address), leaves it there and returns None."""
    eng.bootstrap(_bootstrap_rows(eng.base_rows, bootstrap, random_state))   # enstop_.py:88, on the device
    # sample_weight is all ones (enstop_.py:91); random_state is passed on unchanged, so a
    # RandomState instance continues its stream into the factor initialisation while an int
    # re-seeds it (enstop_.py:101,113 + plsa.py:707)
    _fit_on_engine(eng, k, None, init, n_iter, n_iter_per_test, tolerance, e_step_thresh,
                   random_state, flags)
    if stack_dst is not None:
        eng.copy_components_to_device(stack_dst)
        return None
    _, V = eng.get_factors(want_u=False)
    return V


@_locked
def plsa_topics(X, k, **kwargs):
    """Bootstrap-resample the documents of X and fit pLSA; returns the (k, n_words) topic matrix.
    Keyword arguments as the reference: bootstrap, random_state, init, n_iter, n_iter_per_test,
    tolerance, e_step_thresh (default 1e-16 here, enstop_.py:99,111); plus device, flags, arithmetic ("reference": the
    reference's float32 sums, rounding for rounding -- engine.arithmetic_flags)."""
    A = X.tocsr() if issparse(X) else csr_matrix(X)
    eng = get_engine(kwargs.get("device", None))
    eng.upload_csr(A)
    return _member_on_engine(
        eng, k, bootstrap=kwargs.get("bootstrap", True), random_state=kwargs.get("random_state", None),
        init=kwargs.get("init", "random"), n_iter=kwargs.get("n_iter", 100),
        n_iter_per_test=kwargs.get("n_iter_per_test", 10), tolerance=kwargs.get("tolerance", 0.001),
        e_step_thresh=kwargs.get("e_step_thresh", 1e-16), flags=_member_flags(kwargs))


last_nmf_path = None          # "host" / "device": where the last nmf_topics / ensemble member / NMF refit ran


def _nmf_config(kwargs):
    return dict(init=kwargs.get("init", "nndsvd"), beta_loss=kwargs.get("beta_loss", 1), solver=kwargs.get("solver", "mu"),
                alpha=kwargs.get("alpha", 0.0))


def _nmf_topics_host(A, k, kwargs):
    from sklearn.decomposition import NMF
    if kwargs.get("bootstrap", True):
        rng = check_random_state(kwargs.get("random_state", None))
        A = A[rng.randint(0, A.shape[0], size=A.shape[0])]
    nmf = NMF(n_components=k, init=kwargs.get("init", "nndsvd"), beta_loss=kwargs.get("beta_loss", 1),
              alpha_W=kwargs.get("alpha", 0.0), solver=kwargs.get("solver", "mu"),
              random_state=kwargs.get("random_state", None)).fit(A)
    return nmf.components_


def _nmf_topics_on_engine(eng, A, k, kwargs):
    """One member on a corpus already uploaded to `eng`: the same bootstrap draw, resampled on the device; the starting
    factors from the resampled matrix on the host (public APIs), the fit on the device."""
    from . import nmf as _nmf
    random_state = kwargs.get("random_state", None)
    if kwargs.get("bootstrap", True):
        rng = check_random_state(random_state)
        idx = rng.randint(0, A.shape[0], size=A.shape[0])
        eng.bootstrap(idx)
        A = A[idx]
    else:
        eng.bootstrap(None)
    W0, H0 = _nmf.nmf_init(A, k, kwargs.get("init", "nndsvd"), random_state)
    _nmf.fit_on_engine(eng, W0, H0, True, 200, 1e-4)           # NMF's defaults: max_iter=200, tol=1e-4
    _, H = eng.nmf_get_factors(want_w=False)
    return H


def nmf_topics(X, k, **kwargs):
    """enstop_.py:118-161: bootstrap-resample the documents, fit NMF (Kullback-Leibler, multiplicative updates), return
    the L1-row-normalised components.  `backend`: "host" (scikit-learn's NMF, exactly as the reference calls it; `alpha`
    maps to `alpha_W`, scikit-learn renamed the parameter in 1.0), "device" (enstop_amd.nmf: the same arithmetic on the
    GPU; ValueError for what it does not carry: another beta_loss / solver / init, alpha != 0) or None: ENSTOP_AMD_NMF =
    host | device | auto, default host.  `last_nmf_path` says what ran."""
    global last_nmf_path
    from .utils import normalize
    from . import nmf as _nmf
    on_device = _nmf.use_device(kwargs.get("backend", None), kwargs.get("device", None), **_nmf_config(kwargs))
    A = X.tocsr() if issparse(X) else csr_matrix(X)
    if on_device:
        eng = get_engine(kwargs.get("device", None))
        with eng.lock:
            A = A.astype(np.float32, copy=False)
            eng.upload_csr(A)
            try:
                components = _nmf_topics_on_engine(eng, A, k, kwargs)
            finally:
                eng.bootstrap(None)          # the context is left on the corpus, not on the resample
    else:
        components = _nmf_topics_host(A, k, kwargs)
    last_nmf_path = "device" if on_device else "host"
    topics = np.array(components, dtype=np.float64, order="C")
    normalize(topics, axis=1)
    return topics


def _ensemble_of_nmf_topics(X, k, n_runs, **kwargs):
    """model="nmf" branch of ensemble_of_topics (enstop_.py:199-231): the members one after the other, on the host or --
    one upload for all of them -- on one device context."""
    global last_nmf_path
    from .utils import normalize
    from . import nmf as _nmf
    kw = {key: kwargs[key] for key in ("bootstrap", "random_state", "init", "beta_loss", "alpha", "solver")
          if key in kwargs}
    backend, device = kwargs.get("nmf_backend", None), kwargs.get("device", None)
    if not _nmf.use_device(backend, device, **_nmf_config(kw)):
        return np.vstack([nmf_topics(X, k, backend="host", **kw) for _ in range(n_runs)])
    A = (X.tocsr() if issparse(X) else csr_matrix(X)).astype(np.float32, copy=False)
    eng = get_engine(device)
    out = []
    with eng.lock:
        eng.upload_csr(A)
        try:
            for _ in range(n_runs):
                topics = np.array(_nmf_topics_on_engine(eng, A, k, kw), dtype=np.float64, order="C")
                normalize(topics, axis=1)
                out.append(topics)
        finally:
            eng.bootstrap(None)
    last_nmf_path = "device"
    return np.vstack(out)


def ensemble_of_topics(X, k, model="plsa", n_jobs=4, n_runs=16, parallelism="dask", **kwargs):
    """All topics of `n_runs` bootstrapped fits stacked to (n_runs * k, n_words), enstop_.py:164-231.
    model="plsa": on the GPU(s), see `_ensemble_of_plsa_topics`; model="nmf": scikit-learn on the host, or the device with
    nmf_backend="device" / ENSTOP_AMD_NMF (see `nmf_topics`)."""
    if model == "nmf":
        return _ensemble_of_nmf_topics(X, k, n_runs, **kwargs)
    if model != "plsa":
        raise ValueError('Model must be one of "plsa" or "nmf"')
    return _ensemble_of_plsa_topics(X, k, n_jobs, n_runs, parallelism, **kwargs)


@_locked
def _ensemble_of_plsa_topics(X, k, n_jobs=4, n_runs=16, parallelism="dask", **kwargs):
    """All topics of `n_runs` bootstrapped fits stacked to (n_runs * k, n_words), enstop_.py:164-231.

    `parallelism`:
      "none"            members run serially on this process' GPU sharing `random_state` exactly
                        like the reference's serial branch (enstop_.py:220-223).
      "batched"         like "dask", but the members of a rank advance through the fused EM schedule TOGETHER: every kernel
                        of an iteration is launched once for up to ENSTOP_AMD_BATCH_MEMBERS (32) members, each member
                        bit-identical to its fit under "dask", the likelihood test per member.
                        Calls a batch cannot carry (reference arithmetic, materialised schedule, nnz * k >= 2e9, ...)
                        silently take the "dask" path; `last_ensemble_timing["path"]` says which ran.
                        ENSTOP_AMD_ENSEMBLE=batched sends "dask" / "joblib" this way too (A/B measurement).
      "dask" / "joblib" accepted for drop-in compatibility; the thread fan-out they name is
                        replaced by the one-GPU-per-process model: after
                        `enstop_amd.distributed.init()` under a launcher that sets RANK / WORLD_SIZE
                        (torchrun, `bench.py --gpus N`) run r executes on rank r % world_size and
                        the stack is all-gathered over RCCL.  `n_jobs`: members fitted CONCURRENTLY on this
                        process' GPU (at most 4 contexts, and 1 once a single fit fills the GPU:
                        nnz * k >= 2e9); the stack does not depend on it.
    Per-run streams: with an int (or None) `random_state` run r uses seed `random_state + r`
    (reference: every thread re-seeds with the same int, producing identical members,
    enstop_.py:86 -- a documented defect, not reproduced).
    """
    if parallelism not in PARALLELISM:
        raise ValueError("Unrecognized parallelism {}; should be one of {}".format(parallelism, PARALLELISM))
    A = X.tocsr() if issparse(X) else csr_matrix(X)
    eng = get_engine(kwargs.get("device", None))
    eng.upload_csr(A)
    member_kw = dict(bootstrap=kwargs.get("bootstrap", True), init=kwargs.get("init", "random"),
                     n_iter=kwargs.get("n_iter", 100), n_iter_per_test=kwargs.get("n_iter_per_test", 10),
                     tolerance=kwargs.get("tolerance", 0.001),
                     e_step_thresh=kwargs.get("e_step_thresh", 1e-16), flags=_member_flags(kwargs))
    random_state = kwargs.get("random_state", None)

    if parallelism == "none":
        topics = [_member_on_engine(eng, k, random_state=random_state, **member_kw) for _ in range(n_runs)]
        return np.vstack(topics)

    from . import distributed
    rank, world = distributed.rank_world()
    if isinstance(random_state, np.random.RandomState):
        # one shared stream cannot be split deterministically across processes: derive per-run seeds
        base_seed = int(random_state.randint(0, 2 ** 31 - 1))
    elif random_state is None:
        base_seed = int(np.random.randint(0, 2 ** 31 - 1)) if world == 1 else distributed.broadcast_seed()
    else:
        base_seed = int(random_state)
    runs = list(range(rank, n_runs, world))
    import time
    t0 = time.perf_counter()
    # the result array is allocated now and its pages are touched by a side thread while the members are fitted (the fill
    # releases the GIL): the one device-to-host copy of the stack then lands in resident pages -- a fresh 424 MB array
    # costs that copy 17.6 ms in page faults against 7.9 ms (profiles/r04_member_stack_to_host_paths.md)
    out, toucher = None, None
    if n_runs % world == 0:
        out = np.empty((n_runs * k, A.shape[1]), np.float32)
        toucher = threading.Thread(target=out.fill, args=(0.0,), daemon=True)
        toucher.start()
    batched = 0
    if _batched_requested(parallelism) and runs and _batch_eligible(eng, A, k, member_kw):
        room = min(batch_members_cap(), eng.member_capacity(k))
        batched = min(room, len(runs))
    stack_eng = _fit_members(A, k, runs, {r: base_seed + r for r in runs}, member_kw, kwargs.get("device", None),
                             n_jobs, world, n_runs, (batched, room) if batched else 0)
    t1 = time.perf_counter()
    if toucher is not None:
        toucher.join()
    out = distributed.gather_stack(stack_eng, n_runs, k, A.shape[1], out=out)
    last_ensemble_timing.update(fit_s=t1 - t0, gather_s=time.perf_counter() - t1, members=len(runs), rank=rank, world=world,
                                path="batched" if batched else "contexts", batch=batched if batched else 1)
    if not batched:
        last_ensemble_timing.pop("groups", None)
    return out
