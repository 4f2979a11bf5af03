"""The decisions every Python driver takes before the device runs (enstop_amd/_driver.py): flag bits, whether sample weights
reach the engine, how the starting factors get onto the device, scoped engine settings -- and the CSR staging and error
mapping that Engine.upload_csr and Engine.score_rows share.  No GPU and no library: a recording fake engine and a fake
member batch note each method called and its arguments; loading libplsa_hip.so fails the test.  Expected values are written
out from the header's bit values and from NumPy."""
import itertools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED, SW_LL_ONLY, NO_ZERO_ARM, GRAPH, SUMS, LL = 1, 8, 16, 128, 256, 512
N, M, K = 5, 7, 3


def numpy_normalize_rows(a):
    s = a.sum(axis=1, keepdims=True)
    np.divide(a, s, out=a, where=s > 0)
    return a


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    """utils.normalize divides in NumPy here instead of in the library's host routine, and nothing may load the library"""
    from enstop_amd import _lib, utils

    def refuse():
        raise AssertionError("the driver rules loaded libplsa_hip.so")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(utils, "host_normalize_rows", numpy_normalize_rows)
    for name in ("ENSTOP_AMD_ARITHMETIC", "ENSTOP_AMD_MATERIALISE", "ENSTOP_AMD_HOST_INIT", "ENSTOP_AMD_P_BUDGET_MB"):
        monkeypatch.delenv(name, raising=False)


class FakeEngine:
    def __init__(self, n=N, m=M, arithmetic_bits=0, p_budget=0):
        self.calls = []
        self.shape = (n, m, 20)
        self.base_rows = n
        self.arithmetic_bits = arithmetic_bits
        self.p_budget = p_budget

    def _note(self, name, *args, **kwargs):
        self.calls.append((name, args, kwargs))

    def upload_csr(self, X):
        self._note("upload_csr", X)

    def init_factors_device(self, k, seed=0):
        self._note("init_factors_device", k, seed)

    def init_factors_numpy_stream(self, k, rng, topics=None):
        self._note("init_factors_numpy_stream", k, rng, topics=topics)

    def set_factors(self, U, V=None):
        self._note("set_factors", U, V)

    def set_arithmetic(self, arithmetic=None):
        self._note("set_arithmetic", arithmetic)
        self.arithmetic_bits = arithmetic

    def set_p_budget(self, nbytes=0):
        self._note("set_p_budget", nbytes)
        self.p_budget = nbytes

    def fit(self, *args, **kwargs):
        self._note("fit", *args, **kwargs)
        return 0, np.zeros(1, np.float32)

    def refit(self, *args, **kwargs):
        self._note("refit", *args, **kwargs)
        return 0, np.zeros(1, np.float32)


class FakeBatch:
    def __init__(self, eng):
        self.eng = eng
        self.calls = []

    def prepare(self, member, k, idx=None, rng=None, U=None, V=None):
        self.calls.append(dict(member=member, k=k, idx=idx, rng=rng, U=U, V=V))


class NotARandomState:
    """a generator object that draws what RandomState(seed) draws without being one"""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)

    def rand(self, *shape):
        return self.rs.rand(*shape)

    def randint(self, *args, **kwargs):
        return self.rs.randint(*args, **kwargs)


def same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


def host_start(rng, n=N, m=M, k=K):
    """plsa_init(random) + the float32 casts, in NumPy: rand(k, m) first, rand(n, k) second"""
    V = numpy_normalize_rows(rng.rand(k, m))
    U = numpy_normalize_rows(rng.rand(n, k))
    return U.astype(np.float32), V.astype(np.float32)


# ------------------------------------------------------------------------------------------------
# flags
# ------------------------------------------------------------------------------------------------
def test_the_bit_values_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "plsa_hip.h")).read()
    for name, value in (("PLSA_FUSED", FUSED), ("PLSA_SW_LL_ONLY", SW_LL_ONLY), ("PLSA_STOP_NO_ZERO_ARM", NO_ZERO_ARM),
                        ("PLSA_GRAPH", GRAPH), ("PLSA_REFERENCE_SUMS", SUMS), ("PLSA_REFERENCE_LL", LL)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, value), hdr), name


ARITHMETIC_BITS = ((None, 0), ("default", 0), ("reference", SUMS), ("reference_source", SUMS | LL), (512, LL))


@pytest.mark.parametrize("env_arithmetic, env_materialise", itertools.product((None, "reference"), (None, "1")))
def test_flag_resolution_table(monkeypatch, env_arithmetic, env_materialise):
    from enstop_amd import PLSA, BlockParallelPLSA, StreamedPLSA
    from enstop_amd._driver import resolve_flags
    from enstop_amd.enstop_ import _member_flags
    if env_arithmetic is not None:
        monkeypatch.setenv("ENSTOP_AMD_ARITHMETIC", env_arithmetic)
    if env_materialise is not None:
        monkeypatch.setenv("ENSTOP_AMD_MATERIALISE", env_materialise)
    default = (0 if env_materialise == "1" else FUSED) | (SUMS if env_arithmetic == "reference" else 0)
    for arithmetic, bits in ARITHMETIC_BITS:
        for flags in (None, 0, FUSED, FUSED | NO_ZERO_ARM):
            want = (default if flags is None else flags) | bits
            tag = (flags, arithmetic)
            assert resolve_flags(flags, arithmetic) == want, tag
            assert _member_flags(dict(flags=flags, arithmetic=arithmetic)) == want, tag
            assert resolve_flags(flags, arithmetic, extra=SW_LL_ONLY) == want | SW_LL_ONLY, tag
            # a base stands in for the environment's defaults, never for flags that were given
            assert resolve_flags(flags, arithmetic, NO_ZERO_ARM, FUSED) == (FUSED if flags is None else flags) | bits | NO_ZERO_ARM
        assert PLSA(arithmetic=arithmetic)._flags() == default | bits, arithmetic
        assert BlockParallelPLSA(arithmetic=arithmetic)._flags() == default | NO_ZERO_ARM | bits, arithmetic
        # the streamed stand-in: neither variable has an effect
        assert StreamedPLSA(arithmetic=arithmetic)._flags() == FUSED | NO_ZERO_ARM | bits, arithmetic
    assert isinstance(resolve_flags(np.int64(FUSED)), int) and _member_flags({}) == default


def test_a_batch_refuses_the_graph_flag_of_the_header(monkeypatch):
    from enstop_amd.enstop_ import _batch_eligible
    monkeypatch.delenv("PLSA_GRAPH", raising=False)
    eng, A = SimpleNamespace(), SimpleNamespace(nnz=100)
    assert _batch_eligible(eng, A, K, dict(flags=FUSED, n_iter=10))
    assert _batch_eligible(eng, A, K, dict(flags=None, n_iter=10))
    assert not _batch_eligible(eng, A, K, dict(flags=FUSED | GRAPH, n_iter=10))
    assert not _batch_eligible(eng, A, K, dict(flags=FUSED | SUMS, n_iter=10))
    assert not _batch_eligible(eng, A, K, dict(flags=0, n_iter=10))


# ------------------------------------------------------------------------------------------------
# weights
# ------------------------------------------------------------------------------------------------
def test_effective_weights():
    from enstop_amd._driver import effective_weights
    assert effective_weights(None) is None
    for ones in (np.ones(4, np.int64), np.ones(4, np.float32), np.ones(4, np.float64), [1, 1, 1, 1]):
        assert effective_weights(ones) is None
    nearly = np.array([1.0, 1.0 + 1e-12, 1.0])
    assert nearly[1] != 1.0 and np.float32(nearly[1]) == 1.0
    got = effective_weights(nearly)                               # compared before the cast: an array of float32 ones
    assert got.dtype == np.float32 and np.array_equal(got, np.ones(3, np.float32))
    assert effective_weights(np.asarray(nearly, np.float32)) is None          # the *_inner order: cast first
    got = effective_weights(np.array([0.5, 1.0, 2.0]))
    assert got.dtype == np.float32 and np.array_equal(got, np.array([0.5, 1.0, 2.0], np.float32))


def test_fit_on_engine_initialises_weighs_once_and_fits(monkeypatch):
    from enstop_amd.plsa import _fit_on_engine
    monkeypatch.setenv("ENSTOP_AMD_HOST_INIT", "0")
    eng = FakeEngine()
    _fit_on_engine(eng, K, np.array([1.0, 2.0, 1.0, 1.0, 1.0]), "random", 9, 3, 0.01, 1e-16, np.random.RandomState(4), FUSED,
                   trace=True)
    assert [c[0] for c in eng.calls] == ["init_factors_numpy_stream", "fit"]
    args, kwargs = eng.calls[1][1:]
    assert args[0].dtype == np.float32 and np.array_equal(args[0], [1, 2, 1, 1, 1])
    assert args[1:] == (9, 3, 0.01, 1e-16, FUSED) and kwargs == dict(trace=True)
    eng = FakeEngine()
    _fit_on_engine(eng, K, np.ones(N), "device_random", 9, 3, 0.01, 1e-16, 4)
    assert [c[0] for c in eng.calls] == ["init_factors_device", "fit"] and eng.calls[1][1][0] is None
    assert eng.calls[1][1][5] is None                             # no flags given: the engine resolves them


# ------------------------------------------------------------------------------------------------
# the device-init rule
# ------------------------------------------------------------------------------------------------
def test_device_init_rule(monkeypatch):
    from enstop_amd import _driver
    assert _driver.DEVICE_INIT_MIN_CELLS == 262_144
    k, n, m = 64, 3000, 1096                                      # k * (n + m) = 262 144; the refit's cells are k * n
    assert k * (n + m) == 262_144 and 64 * 4096 == 262_144
    for mode, below, at in (("0", True, True), ("1", False, False), ("auto", False, True), (None, False, True)):
        if mode is None:
            monkeypatch.delenv("ENSTOP_AMD_HOST_INIT", raising=False)
        else:
            monkeypatch.setenv("ENSTOP_AMD_HOST_INIT", mode)
        assert _driver.device_init_wanted(262_143) is below and _driver.device_init_wanted(262_144) is at, mode
        for cells_n, cells_m, want in ((n, m, at), (n, m - 1, below)):          # a fit: k * (n + m)
            plan = _driver.plan_init(cells_n, cells_m, k, "random", np.random.RandomState(0))
            assert (plan[0] == "stream") is want, (mode, cells_n, cells_m)
        for rows, want in ((4096, at), (4095, below)):                          # a refit: k * n
            eng = FakeEngine(rows, m)
            _driver.init_refit_factors(eng, rows, np.full((k, m), 1.0 / m), np.random.RandomState(0))
            assert (eng.calls[0][0] == "init_factors_numpy_stream") is want, (mode, rows)


# ------------------------------------------------------------------------------------------------
# initialisation paths
# ------------------------------------------------------------------------------------------------
SEED = 12


def _corpus():
    rs = np.random.RandomState(1)
    return np.ceil(rs.rand(N, M) * 3) * (rs.rand(N, M) < 0.6)


@pytest.mark.parametrize("mode", ["0", "1"])
def test_device_random_draws_one_seed(monkeypatch, mode):
    from enstop_amd._driver import init_factors
    monkeypatch.setenv("ENSTOP_AMD_HOST_INIT", mode)
    eng, rng = FakeEngine(), np.random.RandomState(SEED)
    init_factors(eng, K, "device_random", rng)
    want = np.random.RandomState(SEED)
    assert eng.calls == [("init_factors_device", (K, int(want.randint(0, 2 ** 31 - 1))), {})]
    assert same_state(rng, want)


def test_stream_path_hands_the_untouched_generator_over(monkeypatch):
    from enstop_amd._driver import init_factors
    monkeypatch.setenv("ENSTOP_AMD_HOST_INIT", "0")
    eng, rng = FakeEngine(), np.random.RandomState(SEED)
    init_factors(eng, K, "random", rng)
    assert len(eng.calls) == 1 and eng.calls[0][0] == "init_factors_numpy_stream"
    assert eng.calls[0][1][0] == K and eng.calls[0][1][1] is rng and eng.calls[0][2] == dict(topics=None)
    assert same_state(rng, np.random.RandomState(SEED))


def _assert_host_call(eng, U, V):
    assert len(eng.calls) == 1 and eng.calls[0][0] == "set_factors"
    got_u, got_v = eng.calls[0][1]
    for got, want in ((got_u, U), (got_v, V)):
        assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(got, want)


def test_host_path_is_plsa_init_cast_to_float32(monkeypatch):
    from enstop_amd._driver import init_factors
    from enstop_amd.plsa import plsa_init
    monkeypatch.setenv("ENSTOP_AMD_HOST_INIT", "1")
    eng, rng, twin = FakeEngine(), np.random.RandomState(SEED), np.random.RandomState(SEED)
    init_factors(eng, K, "random", rng)
    U, V = plsa_init(SimpleNamespace(shape=(N, M)), K, "random", twin)
    _assert_host_call(eng, U.astype(np.float32), V.astype(np.float32))
    assert same_state(rng, twin)
    U, V = host_start(np.random.RandomState(SEED))                # and plsa_init draws rand(k, m) first, rand(n, k) second
    _assert_host_call(eng, U, V)


@pytest.mark.parametrize("mode", ["0", "1", "auto"])
def test_everything_else_takes_the_host_whatever_the_size_rule_says(monkeypatch, mode):
    from enstop_amd._driver import init_factors
    from enstop_amd.plsa import plsa_init
    monkeypatch.setenv("ENSTOP_AMD_HOST_INIT", mode)
    X = _corpus()
    eng = FakeEngine()                                            # a generator that is no RandomState
    init_factors(eng, K, "random", NotARandomState(SEED))
    _assert_host_call(eng, *host_start(np.random.RandomState(SEED)))
    np.random.seed(3)                                             # nndsvd: randomized_svd draws from NumPy's global stream
    U, V = plsa_init(X, K, "nndsvd", np.random.RandomState(SEED))
    eng = FakeEngine()
    np.random.seed(3)
    init_factors(eng, K, "nndsvd", np.random.RandomState(SEED), X)
    _assert_host_call(eng, U.astype(np.float32), V.astype(np.float32))
    U0, V0 = np.arange(1.0, N * K + 1).reshape(N, K), np.arange(1.0, K * M + 1).reshape(K, M)       # a tuple of factors
    eng, rng = FakeEngine(), np.random.RandomState(SEED)
    init_factors(eng, K, (U0, V0), rng)
    _assert_host_call(eng, (U0 / U0.sum(1, keepdims=True)).astype(np.float32), (V0 / V0.sum(1, keepdims=True)).astype(np.float32))
    assert same_state(rng, np.random.RandomState(SEED))


@pytest.mark.parametrize("bootstrap", [True, False])
def test_a_batch_slot_takes_the_same_paths(monkeypatch, bootstrap):
    from enstop_amd.enstop_ import _prepare_member

    def prepared(mode, random_state, init="random"):
        monkeypatch.setenv("ENSTOP_AMD_HOST_INIT", mode)
        eng = FakeEngine()
        batch = FakeBatch(eng)
        _prepare_member(batch, 2, eng, K, bootstrap=bootstrap, random_state=random_state, init=init,
                        n_iter=10, flags=FUSED)              # (the fit's keywords are passed along and ignored)
        (call,) = batch.calls
        assert call["member"] == 2 and call["k"] == K
        return call

    def twin_and_idx():
        twin = np.random.RandomState(SEED)                        # the bootstrap is the first draw of the member's stream
        return twin, (twin.randint(0, N, size=N) if bootstrap else None)

    rng = np.random.RandomState(SEED)
    call = prepared("0", rng)
    twin, idx = twin_and_idx()
    assert call["rng"] is rng and call["U"] is None and call["V"] is None and same_state(rng, twin)
    assert np.array_equal(call["idx"], idx) if bootstrap else call["idx"] is None

    rng = np.random.RandomState(SEED)
    call = prepared("1", rng)
    twin, idx = twin_and_idx()
    U, V = host_start(twin)
    assert call["rng"] is None and same_state(rng, twin)
    assert np.array_equal(call["idx"], idx) if bootstrap else call["idx"] is None
    for got, want in ((call["U"], U), (call["V"], V)):
        assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(got, want)

    U0, V0 = np.ones((N, K)), np.ones((K, M))                     # a tuple: the host whatever the rule says
    call = prepared("0", np.random.RandomState(SEED), init=(U0, V0))
    assert call["rng"] is None and np.array_equal(call["U"], np.full((N, K), 1 / K, np.float32))
    assert np.array_equal(call["V"], np.full((K, M), 1 / M, np.float32))
    assert np.array_equal(call["idx"], twin_and_idx()[1]) if bootstrap else call["idx"] is None

    from enstop_amd._driver import apply_init_slot
    with pytest.raises(ValueError, match="device_random"):       # (not eligible for a batch: enstop_._batch_eligible)
        apply_init_slot(FakeBatch(FakeEngine()), 0, K, ("device_random", 1))


def test_refit_initialisation(monkeypatch):
    from enstop_amd._driver import init_refit_factors
    from enstop_amd.plsa import _refit_on_engine
    topics = numpy_normalize_rows(np.random.RandomState(2).rand(K, M))
    monkeypatch.setenv("ENSTOP_AMD_HOST_INIT", "0")
    eng, rng = FakeEngine(), np.random.RandomState(SEED)
    init_refit_factors(eng, N, topics, rng)
    (name, args, kwargs), = eng.calls
    assert name == "init_factors_numpy_stream" and args[0] == K and args[1] is rng and np.array_equal(kwargs["topics"], topics)
    assert same_state(rng, np.random.RandomState(SEED))
    want = numpy_normalize_rows(np.random.RandomState(SEED).rand(N, K)).astype(np.float32)
    for mode, generator in (("1", np.random.RandomState(SEED)), ("0", NotARandomState(SEED))):
        monkeypatch.setenv("ENSTOP_AMD_HOST_INIT", mode)
        eng = FakeEngine()
        init_refit_factors(eng, N, topics, generator)
        _assert_host_call(eng, want, topics.astype(np.float32))
    twin = np.random.RandomState(SEED)
    twin.rand(N, K)
    assert same_state(generator.rs, twin)
    # plsa_refit's body: upload, initialise, then one refit with the weights decided once
    monkeypatch.setenv("ENSTOP_AMD_HOST_INIT", "1")
    eng, X = FakeEngine(), SimpleNamespace(shape=(N, M))
    _refit_on_engine(eng, X, topics, np.ones(N), 50, 5, 0.001, 1e-32, np.random.RandomState(SEED), FUSED, trace=True)
    assert [c[0] for c in eng.calls] == ["upload_csr", "set_factors", "refit"] and eng.calls[0][1][0] is X
    assert eng.calls[2][1] == (None, 50, 5, 0.001, 1e-32, FUSED) and eng.calls[2][2] == dict(trace=True)


# ------------------------------------------------------------------------------------------------
# scoped settings
# ------------------------------------------------------------------------------------------------
def test_scoped_arithmetic_restores_what_the_engine_recorded(monkeypatch):
    from enstop_amd._driver import scoped_arithmetic
    eng = FakeEngine(arithmetic_bits=256)
    with scoped_arithmetic(eng, None):
        pass
    assert eng.calls == [] and eng.arithmetic_bits == 256
    with scoped_arithmetic(eng, "reference_source"):
        assert eng.arithmetic_bits == 768
    assert eng.calls == [("set_arithmetic", (768,), {}), ("set_arithmetic", (256,), {})]
    eng = FakeEngine(arithmetic_bits=256)
    with pytest.raises(KeyError):
        with scoped_arithmetic(eng, "reference_source"):
            raise KeyError("inside")
    assert eng.calls == [("set_arithmetic", (768,), {}), ("set_arithmetic", (256,), {})]
    eng = FakeEngine(arithmetic_bits=256)                         # "default" is a mode that was asked for
    with scoped_arithmetic(eng, "default"):
        assert eng.arithmetic_bits == 0
    assert eng.calls == [("set_arithmetic", (0,), {}), ("set_arithmetic", (256,), {})]
    monkeypatch.setenv("ENSTOP_AMD_ARITHMETIC", "reference")      # None consults the variable
    eng = FakeEngine(arithmetic_bits=0)
    with scoped_arithmetic(eng, None):
        assert eng.arithmetic_bits == 256
    assert eng.calls == [("set_arithmetic", (256,), {}), ("set_arithmetic", (0,), {})]


def test_scoped_p_budget_restores_what_the_engine_recorded(monkeypatch):
    from enstop_amd._driver import scoped_p_budget
    eng = FakeEngine(p_budget=4096)
    with scoped_p_budget(eng, None):
        pass
    assert eng.calls == [] and eng.p_budget == 4096
    with scoped_p_budget(eng, 1 << 20):
        assert eng.p_budget == 1 << 20
    assert eng.calls == [("set_p_budget", (1 << 20,), {}), ("set_p_budget", (4096,), {})]
    eng = FakeEngine(p_budget=4096)
    with pytest.raises(KeyError):
        with scoped_p_budget(eng, 0):                             # 0 is a budget that was asked for: none
            assert eng.p_budget == 0
            raise KeyError("inside")
    assert eng.calls == [("set_p_budget", (0,), {}), ("set_p_budget", (4096,), {})]
    monkeypatch.setenv("ENSTOP_AMD_P_BUDGET_MB", "1.5")
    eng = FakeEngine(p_budget=0)
    with scoped_p_budget(eng, None):
        assert eng.p_budget == 3 << 19
    assert eng.calls == [("set_p_budget", (3 << 19,), {}), ("set_p_budget", (0,), {})]


def test_the_engine_records_the_arithmetic_it_installed():
    """Engine.set_arithmetic over a stand-in for the library: the bits go to the C call and into `arithmetic_bits`"""
    from enstop_amd.engine import Engine
    seen = []
    eng = object.__new__(Engine)
    eng._h = None
    eng._L = SimpleNamespace(plsa_set_arithmetic=lambda h, bits: seen.append(bits) or 0)
    assert eng.set_arithmetic("reference_source") is eng and eng.arithmetic_bits == 768
    assert eng.set_arithmetic(None) is eng and eng.arithmetic_bits == 0 and seen == [768, 0]


# ------------------------------------------------------------------------------------------------
# CSR staging and error mapping
# ------------------------------------------------------------------------------------------------
class CsrStub:
    """says how large it is without being that large"""

    def __init__(self, shape, nnz):
        self.shape, self.nnz = shape, nnz
        self.indptr, self.indices, self.data = np.array([0, 1, 2], np.int64), np.array([0, 1], np.int64), np.array([1.0, 2.0])

    def tocsr(self):
        return self


def test_csr_staging_checks_and_casts():
    from enstop_amd.engine import _csr_arrays
    for shape, nnz in (((10, 10), 2 ** 31 - 63), ((2 ** 31 - 1, 5), 3), ((5, 2 ** 31 - 1), 3)):
        with pytest.raises(ValueError, match=r"matrix too large for 32-bit indices: %d x %d with %d stored entries \(limit 2\^31 - 64 "
                                             r"entries\)" % (shape + (nnz,))):
            _csr_arrays(CsrStub(shape, nnz))
    for shape, nnz in (((10, 10), 2 ** 31 - 64), ((2 ** 31 - 2, 2 ** 31 - 2), 3)):
        indptr, indices, data = _csr_arrays(CsrStub(shape, nnz))
        assert indptr.dtype == np.int32 and indices.dtype == np.int32 and data.dtype == np.float32
        assert all(a.flags.c_contiguous for a in (indptr, indices, data))
        assert indptr.tolist() == [0, 1, 2] and indices.tolist() == [0, 1] and data.tolist() == [1.0, 2.0]
    import scipy.sparse as sp
    X = sp.coo_matrix(np.array([[0, 2.5, 0], [1, 0, 3]]))         # any scipy matrix: converted to CSR
    indptr, indices, data = _csr_arrays(X)
    assert indptr.tolist() == [0, 1, 3] and indices.tolist() == [1, 0, 2] and data.tolist() == [2.5, 1.0, 3.0]


UPLOAD, SCORE, CORE = "enstop_amd/csrc/plsa_hip.hip", "enstop_amd/csrc/plsa_score.hpp", "enstop_amd/csrc/plsa_hip.hip"
PTR, COL = "indptr is not non-decreasing within [0, nnz]", "column index outside [0, m)"
SHORT = "column index out of range"
# (source file, line at the time of writing, text that stands in the source, a message as it arrives, exception, its text --
#  None: the message itself).  What each message mapped to before the two mappings were merged.
UPLOAD_MESSAGES = [
    (UPLOAD, 1210, "plsa_upload_csr: bad shape n=", "plsa_upload_csr: bad shape n=0 m=5 nnz=0", "DeviceError", None),
    (UPLOAD, 1213, "plsa_upload_csr: n, m and nnz must each be < 2^31", None, "DeviceError", None),
    (UPLOAD, 1214, "plsa_upload_csr: indptr[0] != 0 or indptr[n] != nnz", None, "ValueError", None),
    (UPLOAD, 1237, PTR, "plsa_upload_csr: " + PTR, "ValueError", None),
    (UPLOAD, 1238, COL, "plsa_upload_csr: " + COL, "ValueError", SHORT),
    (UPLOAD, 1238, 'bad == 3 ? "; " : ""', "plsa_upload_csr: " + PTR + "; " + COL, "ValueError", SHORT),
    # HIPCHK (:339) quotes the failed expression, and this one names the row pointers
    (UPLOAD, 1218, "hipMemcpyAsync(c->b_indptr.p, indptr,",
     "hipMemcpyAsync(c->b_indptr.p, indptr, sizeof(int) * (size_t)(n + 1), hipMemcpyHostToDevice, c->stream) failed: "
     "out of memory (plsa_hip.hip:1218)", "ValueError", None),
    (UPLOAD, 1216, "CHK(ensure(c, c->b_col,", "hipMalloc(&p, bytes) failed: out of memory (plsa_hip.hip:380)", "DeviceError", None),
    (UPLOAD, 647, "launch of %s failed: %s", "launch of k_validate_csr failed: invalid configuration argument", "DeviceError", None),
]
SCORE_MESSAGES = [
    (SCORE, 55, "plsa_score_rows: no corpus uploaded", None, "DeviceError", None),
    (CORE, 687, "factors not set (call plsa_set_factors)", None, "DeviceError", None),
    (CORE, 690, "factors were set for a %lld x %lld matrix but the active matrix is",
     "factors were set for a 9 x 7 matrix but the active matrix is 5 x 7 (call plsa_set_factors after plsa_upload_csr / "
     "plsa_bootstrap)", "DeviceError", None),
    (SCORE, 57, "plsa_score_rows: k=%d outside [1,1024]", "plsa_score_rows: k=2000 outside [1,1024]", "DeviceError", None),
    (SCORE, 60, "plsa_score_rows: nnz must be < 2^31", None, "DeviceError", None),
    (SCORE, 62, "plsa_score_rows: another matrix needs indptr, indices and data (all NULL and nnz = 0: the active matrix)", None,
     "ValueError", None),
    (SCORE, 64, "plsa_score_rows: indptr[0] != 0 or indptr[n] != nnz -- the matrix must have the active matrix's ",
     "plsa_score_rows: indptr[0] != 0 or indptr[n] != nnz -- the matrix must have the active matrix's 5 rows", "ValueError", None),
    (SCORE, 67, "plsa_score_rows: all three outputs are NULL", None, "DeviceError", None),
    (SCORE, 43, PTR, "plsa_score_rows: " + PTR, "ValueError", None),
    (SCORE, 44, COL, "plsa_score_rows: " + COL, "ValueError", SHORT),
    (SCORE, 44, 'bad == 3 ? "; " : ""', "plsa_score_rows: " + PTR + "; " + COL, "ValueError", None),
    (SCORE, 30, "hipMemcpyAsync(s.indptr.p, indptr,",
     "hipMemcpyAsync(s.indptr.p, indptr, sizeof(int) * (size_t)(c->n + 1), hipMemcpyHostToDevice, c->stream) failed: "
     "out of memory (plsa_score.hpp:30)", "ValueError", None),
    (CORE, 671, "resident sample weights were set for %lld documents, the active matrix has",
     "resident sample weights were set for 9 documents, the active matrix has 5", "DeviceError", None),
    (CORE, 647, "launch of %s failed: %s", "launch of k_score_rows failed: invalid configuration argument", "DeviceError", None),
]


@pytest.mark.parametrize("messages, pointer_text_wins", [(UPLOAD_MESSAGES, False), (SCORE_MESSAGES, True)])
def test_every_message_maps_to_the_exception_it_mapped_to(messages, pointer_text_wins):
    from enstop_amd.engine import DeviceError, _csr_failure
    sources = {}
    for path, _line, in_source, message, kind, text in messages:
        if path not in sources:
            sources[path] = open(os.path.join(ROOT, path)).read()
        assert in_source in sources[path], (path, in_source)
        message = in_source if message is None else message
        exc = _csr_failure(message, pointer_text_wins)
        assert type(exc) is (ValueError if kind == "ValueError" else DeviceError), message
        assert str(exc) == (message if text is None else text), message
    # the one message on which the two entry points differ: both contract violations at once
    both = "%s; %s" % (PTR, COL)
    assert str(_csr_failure("plsa_upload_csr: " + both)) == SHORT
    assert str(_csr_failure("plsa_score_rows: " + both, pointer_text_wins=True)) == "plsa_score_rows: " + both
