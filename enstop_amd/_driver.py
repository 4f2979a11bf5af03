"""What every Python driver of a fit decides before the device runs, each rule written once: which flag bits the fit runs
with, whether sample weights reach the engine at all, how the starting factors get onto the device, and how a setting of
the shared engine is scoped to one call.  The functions take the engine (or a MemberBatch) as an argument and never load
the library, so a recording fake exercises them on a CPU (tests/test_driver_host.py)."""
import os
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np

from .engine import PLSA_FUSED, PLSA_REFERENCE_LL, PLSA_REFERENCE_SUMS, arithmetic_flags, default_flags
from .utils import normalize

DEVICE_INIT_MIN_CELLS = 262_144        # factor cells from which ENSTOP_AMD_HOST_INIT=auto initialises on the device


def resolve_flags(flags=None, arithmetic=None, extra=0, base=None):
    """The flag bits of one fit: `flags` as given -- None: `base`, and default_flags() (ENSTOP_AMD_MATERIALISE,
    ENSTOP_AMD_ARITHMETIC) when there is no base either -- with arithmetic_flags(arithmetic) and `extra` ORed in.
    The one caller with a base of its own is the streamed module's stand-in (StreamedPLSA._flags: base=PLSA_FUSED): it
    never consults the environment, which tests/golden/streamfit_* pin; the doc-sharded in-loop fit does the same."""
    if flags is None:
        flags = default_flags() if base is None else base
    return int(flags) | arithmetic_flags(arithmetic) | extra


def effective_weights(sample_weight):
    """None when there are no weights or all of them are 1 (compared as given, before the cast: plsa.py:712), else the
    weights as float32.  Callers that cast first (the *_inner functions) hand in the cast array."""
    weighted = sample_weight is not None and np.any(np.asarray(sample_weight) != 1.0)
    return np.asarray(sample_weight, np.float32) if weighted else None


def resolve_smoothing(name, value):
    """A pseudo-count of smoothed EM (smoothed.py) as a float: None is 0.0 (off); anything that is not a finite number >= 0
    is a ValueError that names the parameter.  Called before an engine is touched."""
    if value is None:
        return 0.0
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError("%s must be None or a finite number >= 0, not %r" % (name, value)) from None
    if not (v >= 0.0 and np.isfinite(v)) or isinstance(value, (bool, np.bool_)):
        raise ValueError("%s must be None or a finite number >= 0, not %r" % (name, value))
    return v


def smoothed_flags(flags):
    """The flag bits of a smoothed fit, refused where smoothed EM has no form: it runs the fused schedule in the default
    arithmetic only."""
    flags = resolve_flags(flags)
    if not flags & PLSA_FUSED:
        raise ValueError("smoothed EM runs the fused schedule only (ENSTOP_AMD_MATERIALISE / flags without PLSA_FUSED)")
    if flags & (PLSA_REFERENCE_SUMS | PLSA_REFERENCE_LL):
        raise ValueError("smoothed EM has no form in the reference arithmetic (ENSTOP_AMD_ARITHMETIC / flags=%d)" % flags)
    return flags


def device_init_wanted(cells):
    """ENSTOP_AMD_HOST_INIT: "0" the device, "1" the host, "auto" (default) the device from DEVICE_INIT_MIN_CELLS factor
    cells on -- tiny problems stay on the host.  cells: k * (n + m) for a fit, k * n for a refit."""
    mode = os.environ.get("ENSTOP_AMD_HOST_INIT", "auto")
    return mode == "0" or (mode == "auto" and cells >= DEVICE_INIT_MIN_CELLS)


def host_factors(k, init, rng, shape=None, X=None):
    """plsa_init's (P(z|d), P(w|z)) as C-ordered float32 (plsa.py:709-710); "random" and tuple inits need only X's shape"""
    from .plsa import plsa_init
    U, V = plsa_init(SimpleNamespace(shape=shape) if X is None else X, k, init=init, rng=rng)
    return U.astype(np.float32, order="C"), V.astype(np.float32, order="C")


def plan_init(n, m, k, init, rng, X=None):
    """Which way the starting factors of a fit take, with whatever that way draws from `rng` on the host already drawn:
      ("device_random", seed)  additive, non-reference: counter-based RNG on the GPU, seeded by one rng.randint(0, 2^31 - 1)
                               (host MT19937 draws cost ~1 s for 1M x 64 + 64 x 100k, four times the 50-iteration fit)
      ("stream", rng)          init="random", a legacy RandomState, device_init_wanted(k * (n + m)): plsa_init's draws,
                               normalisation and casts replayed on the device from rng's own MT19937 state, bit-identical
                               (config 3: 8 ms against 0.45 s); the engine advances the untouched rng when it applies the plan
      ("host", U, V)           everything else: host_factors (rng.rand(k, m) first, rng.rand(n, k) second)"""
    if isinstance(init, str) and init == "device_random":
        return ("device_random", int(rng.randint(0, 2 ** 31 - 1)))
    if (isinstance(init, str) and init == "random" and isinstance(rng, np.random.RandomState)
            and device_init_wanted(k * (n + m))):
        return ("stream", rng)
    return ("host",) + host_factors(k, init, rng, (n, m), X)


def apply_init_slot(batch, j, k, plan, idx=None):
    """Carries a plan out on slot j of a MemberBatch, whose member is corpus[idx]."""
    if plan[0] == "stream":
        batch.prepare(j, k, idx=idx, rng=plan[1])
    elif plan[0] == "host":
        batch.prepare(j, k, idx=idx, U=plan[1], V=plan[2])
    else:
        raise ValueError("a member batch has no %s initialisation" % plan[0])


def init_factors(eng, k, init, rng, X=None):
    """The starting factors of plsa_fit for the matrix active on `eng`, planned and put there; nothing is fitted."""
    n, m, _ = eng.shape
    plan = plan_init(n, m, k, init, rng, X)
    if plan[0] == "device_random":
        eng.init_factors_device(k, plan[1])
    elif plan[0] == "stream":
        eng.init_factors_numpy_stream(k, plan[1])
    else:
        eng.set_factors(plan[1], plan[2])


def init_refit_factors(eng, n, topics, rng):
    """The start of plsa_refit (plsa.py:979-981) for n documents: rng.rand(n, k), float64 row normalisation, float32 cast,
    beside the fixed `topics` -- replayed on the device from a RandomState's own stream when device_init_wanted(k * n)
    (bit-identical, 0.22 s of host draws saved at 1 M documents x 64), else on the host."""
    topics = np.asarray(topics)
    k = topics.shape[0]
    if isinstance(rng, np.random.RandomState) and device_init_wanted(k * n):
        eng.init_factors_numpy_stream(k, rng, topics=topics)
    else:
        p_z_given_d = rng.rand(n, k)
        normalize(p_z_given_d, axis=1)
        eng.set_factors(p_z_given_d.astype(np.float32), topics.astype(np.float32))


@contextmanager
def _scoped(eng, setter, recorded, value):
    """One setting of the shared engine for a with-block: `value` goes in through the setter, what the engine had recorded
    comes back on the way out (an exception included).  None touches nothing."""
    if value is not None:
        before = getattr(eng, recorded, 0)
        getattr(eng, setter)(value)
    try:
        yield
    finally:
        if value is not None:
            getattr(eng, setter)(before)


def scoped_arithmetic(eng, arithmetic):
    """`arithmetic=` of ONE kernel-level call on the shared engine (None: ENSTOP_AMD_ARITHMETIC; unset too: the engine's
    mode stays).  "reference" presupposes the reference's entry order: re-sorted triplets are summed in row-major order."""
    if arithmetic is None:
        arithmetic = os.environ.get("ENSTOP_AMD_ARITHMETIC") or None
    return _scoped(eng, "set_arithmetic", "arithmetic_bits", None if arithmetic is None else arithmetic_flags(arithmetic))


def scoped_p_budget(eng, p_budget):
    """`p_budget=` of ONE fit / refit on the shared engine: bytes P(z|w,d) may take in the reference arithmetic
    (Engine.set_p_budget; no effect outside it).  None: ENSTOP_AMD_P_BUDGET_MB; unset too: the engine's budget stays."""
    if p_budget is None:
        mb = os.environ.get("ENSTOP_AMD_P_BUDGET_MB") or None
        p_budget = None if mb is None else int(float(mb) * (1 << 20))
    return _scoped(eng, "set_p_budget", "p_budget", p_budget)
