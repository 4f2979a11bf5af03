"""CPU: the block driver of both online fits (enstop_amd/online.py: drive_blocks), driven with recording fakes.  It uses no GPU
and loads no library: the driver imports no engine, everything that touches a device comes in as a callable.

3 blocks x 2 epochs, once with callables written here, once through plsa_fit_online's and once through lda_fit_online's own
callables with Engine, get_engine and the state classes replaced by fakes.  Held in every case:

    set-ups in block order, before the state is made;
    steps in block order with the schedule's rhos and each block's scale;
    one end_epoch per epoch with the summed values (NaN when nothing is read);
    all folds before the first row read;
    the state closed before the engines, every engine that was opened closed -- also when the second step raises.
"""
import math
import threading

import numpy as np
import pytest
import scipy.sparse as sp

from enstop_amd import lda_online, online, plsa
from enstop_amd.online import OnlineSchedule, block_tokens, drive_blocks

N, M, K, BLOCKS, EPOCHS = 30, 12, 4, 3, 2
RHO = [(10.0 + t) ** -0.7 for t in range(BLOCKS * EPOCHS)]


class Boom(RuntimeError):
    pass


class Log(list):
    def of(self, kind):
        return [e for e in self if e[0] == kind]

    def first(self, kind):
        return next(i for i, e in enumerate(self) if e[0] == kind)

    def last(self, kind):
        return max(i for i, e in enumerate(self) if e[0] == kind)


class FakeEngine:
    """the part of Engine the fits and the driver touch; every call goes to the shared log"""

    def __init__(self, log, device="fake:0"):
        self.log, self.device = log, device
        self.id = len(log.of("open"))
        self.lock = threading.RLock()
        self.rows = None
        log.append(("open", self.id))

    def upload_csr(self, X):
        self.rows = X.shape[0]
        self.log.append(("setup", self.id, X.shape[0]))

    def set_factors(self, U, V):
        assert U.shape == (self.rows, K) and V.shape == (K, M)

    def set_sample_weight(self, sw):
        pass

    def accumulator_device(self):
        return 0, M * K

    def get_factors(self, want_v=True):
        self.log.append(("rows", self.id))
        return (np.full((self.rows, K), float(self.id + 1), np.float32),)

    def close(self):
        self.log.append(("close_engine", self.id))


class FakeState:
    """OnlineState and LdaOnlineState at once: step returns 100 * (step index) + block, and raises on step `fail_at`"""
    fail_at = None

    def __init__(self, home, m, k):
        self.log = home.log
        assert (m, k) == (M, K)
        self.log.append(("state",))

    def set_topics(self, table):
        assert table.shape == (K, M)
        return self
    set_lambda = set_topics

    def _step(self, eng, rho, scale, want):
        t = len(self.log.of("step"))
        self.log.append(("step", eng.id, rho, scale, bool(want)))
        if t == self.fail_at:
            raise Boom("step %d" % t)
        return 100.0 * t + eng.id if want else None

    def step(self, eng, *args):
        if len(args) == 7:                       # OnlineState.step(eng, rho, scale, inner_iter, sw, thresh, want_ll, flags)
            rho, scale, _, _, _, want, _ = args
        else:                                    # LdaOnlineState.step(eng, alpha, eta, rho, scale, doc_iter, thresh, want, flags)
            _, _, rho, scale, _, _, want, _ = args
        return self._step(eng, rho, scale, want)

    def fold(self, eng, *args):
        self.log.append(("fold", eng.id))

    def get_topics(self):
        self.log.append(("topics",))
        return np.ones((K, M), np.float32)
    get_lambda = get_topics

    def close(self):
        self.log.append(("close_state",))


class RecordingSchedule(OnlineSchedule):
    def __init__(self, log, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.log = log

    def end_epoch(self, value):
        self.log.append(("end_epoch", value))
        return super().end_epoch(value)


def corpus():
    rs = np.random.RandomState(3)
    X = sp.random(N, M, density=0.4, format="csr", random_state=rs, dtype=np.float64)
    X.data = np.ceil(X.data * 3)
    X = X.tolil()
    X[:, 0] = 1.0                                # no empty document: every block has tokens
    return X.tocsr().astype(np.float32)


# ------------------------------------------------------------------------------------------------
# the three ways into the driver, recording into `log`: -> (result, expected scales per block, ranges)
# ------------------------------------------------------------------------------------------------
def direct(monkeypatch, log, want, fail_at):
    ranges = [(0, 10), (10, 20), (20, 30)]
    scales = [2.0, 3.0, 5.0]
    home = FakeEngine.__new__(FakeEngine)
    home.log = log
    state_cls = type("State", (FakeState,), {"fail_at": fail_at})

    def setup(eng, i, a, b):
        eng.rows = b - a
        log.append(("setup", eng.id, b - a))
        return float(b - a), scales[i]

    schedule = RecordingSchedule(log, BLOCKS, EPOCHS, tolerance=0.0)
    result = drive_blocks(N, K, ranges, None, schedule, want, "series", new_engine=lambda: FakeEngine(log), setup=setup,
                          make_state=lambda: state_cls(home, M, K), step=lambda st, eng, rho, scale, w: st._step(eng, rho, scale, w),
                          fold=lambda st, eng: st.fold(eng), rows=lambda eng: eng.get_factors(want_v=False)[0],
                          topics=lambda st: st.get_topics())
    return result, scales, ranges


def _patch(monkeypatch, module, state_name, log, fail_at):
    home = FakeEngine.__new__(FakeEngine)
    home.log, home.device, home.lock = log, "fake:0", threading.RLock()
    monkeypatch.setattr(plsa, "get_engine", lambda device=None: home)          # (_locked's lock)
    monkeypatch.setattr(module, "get_engine", lambda device=None: home)
    monkeypatch.setattr(module, "Engine", lambda device: FakeEngine(log, device))
    monkeypatch.setattr(module, state_name, type("State", (FakeState,), {"fail_at": fail_at}))
    monkeypatch.setattr(online, "OnlineSchedule", lambda *a, **kw: RecordingSchedule(log, *a, **kw))
    monkeypatch.setattr(module, "OnlineSchedule", lambda *a, **kw: RecordingSchedule(log, *a, **kw))
    for name in ("ENSTOP_AMD_MATERIALISE", "ENSTOP_AMD_ARITHMETIC"):
        monkeypatch.delenv(name, raising=False)


def through_plsa(monkeypatch, log, want, fail_at):
    _patch(monkeypatch, online, "OnlineState", log, fail_at)
    X = corpus()
    out = online.plsa_fit_online(X, K, n_batches=BLOCKS, n_epochs=EPOCHS, tolerance=0.0, shuffle_documents=False, random_state=0,
                                 return_info=want)
    from enstop_amd.sharded import row_ranges_by_nnz
    ranges = row_ranges_by_nnz(X.indptr, BLOCKS)
    return out, [1.0 / block_tokens(X[a:b]) for a, b in ranges], ranges


def through_lda(monkeypatch, log, want, fail_at):
    _patch(monkeypatch, lda_online, "LdaOnlineState", log, fail_at)
    X = corpus()
    out = lda_online.lda_fit_online(X, K, n_batches=BLOCKS, n_epochs=EPOCHS, tolerance=0.0, shuffle_documents=False,
                                    random_state=0, return_info=want)
    from enstop_amd.sharded import row_ranges_by_nnz
    ranges = row_ranges_by_nnz(X.indptr, BLOCKS)
    return out, [float(N) / (b - a) for a, b in ranges], ranges


WAYS = {"direct": (direct, "series"), "plsa_fit_online": (through_plsa, "log_likelihoods"), "lda_fit_online": (through_lda, "bounds")}


@pytest.mark.parametrize("way", sorted(WAYS))
def test_the_call_sequence(monkeypatch, way):
    run, series = WAYS[way]
    log = Log()
    out, scales, ranges = run(monkeypatch, log, True, None)
    rows, table, info = out
    # engines opened and set up in block order, all before the state is made
    assert [e[1] for e in log.of("open")] == [0, 1, 2]
    assert [(e[1], e[2]) for e in log.of("setup")] == [(i, b - a) for i, (a, b) in enumerate(ranges)]
    assert log.last("setup") < log.first("state") < log.first("step") and len(log.of("state")) == 1
    # steps in block order, with the schedule's rhos and each block's scale
    steps = log.of("step")
    assert [e[1] for e in steps] == [0, 1, 2] * EPOCHS
    assert [e[2] for e in steps] == RHO and info["rho"] == RHO
    assert [e[3] for e in steps] == scales * EPOCHS
    assert all(e[4] for e in steps)
    # one end_epoch per epoch, behind its last step, with the summed values
    sums = [sum(100.0 * (BLOCKS * e + b) + b for b in range(BLOCKS)) for e in range(EPOCHS)]
    assert [e[1] for e in log.of("end_epoch")] == sums and info[series] == sums
    ends = [i for i, e in enumerate(log) if e[0] == "end_epoch"]
    at = [i for i, e in enumerate(log) if e[0] == "step"]
    assert at[BLOCKS - 1] < ends[0] < at[BLOCKS] and at[-1] < ends[1]
    assert info["n_epochs"] == EPOCHS and info["n_steps"] == BLOCKS * EPOCHS and info["block_ranges"] == ranges
    assert info["permutation"] is None and info["bytes_per_block_context"] == 3 * 4 * M * K and len(info["tokens"]) == BLOCKS
    # every block folded before the first is read back, then the topics; rows land in their ranges
    assert [e[1] for e in log.of("fold")] == [0, 1, 2] and [e[1] for e in log.of("rows")] == [0, 1, 2]
    assert log.last("fold") < log.first("rows") < log.last("rows") < log.first("topics")
    for i, (a, b) in enumerate(ranges):
        assert (rows[a:b] == i + 1).all()
    assert table.shape == (K, M) and rows.shape == (N, K)
    # the state is closed before the engines, each engine once
    assert len(log.of("close_state")) == 1 and log.first("topics") < log.first("close_state") < log.first("close_engine")
    assert sorted(e[1] for e in log.of("close_engine")) == [0, 1, 2]


@pytest.mark.parametrize("way", sorted(WAYS))
def test_nothing_read_feeds_nan_to_the_schedule(monkeypatch, way):
    run, _ = WAYS[way]
    log = Log()
    out, _, _ = run(monkeypatch, log, False, None)
    assert len(out) == (3 if way == "direct" else 2)
    assert not any(e[4] for e in log.of("step"))
    ends = log.of("end_epoch")
    assert len(ends) == EPOCHS and all(math.isnan(e[1]) for e in ends)


@pytest.mark.parametrize("way", sorted(WAYS))
def test_a_failing_step_still_closes_the_state_and_every_engine(monkeypatch, way):
    run, _ = WAYS[way]
    log = Log()
    with pytest.raises(Boom):
        run(monkeypatch, log, True, 1)
    assert len(log.of("step")) == 2 and not log.of("fold") and not log.of("rows") and not log.of("end_epoch")
    assert len(log.of("close_state")) == 1 and log.first("close_state") < log.first("close_engine")
    assert sorted(e[1] for e in log.of("close_engine")) == [e[1] for e in log.of("open")] == [0, 1, 2]


def test_the_permutation_is_drawn_behind_the_factors_and_undone():
    """cut_blocks: one permutation from the stream the factors were drawn from, applied to every per-document array, the
    refusal names the caller, and undo puts rows back into the caller's order"""
    X = corpus()
    rng = np.random.RandomState(7)
    U0 = rng.rand(N, K)
    expected = np.random.RandomState(7)
    expected.rand(N, K)
    perm = expected.permutation(N)
    Xp, (Up, none), got, ranges, undo = online.cut_blocks("who", X, BLOCKS, rng, True, U0, None)
    assert (got == perm).all() and none is None and (Up == U0[perm]).all() and (Xp != X[perm]).nnz == 0
    assert ranges[0][0] == 0 and ranges[-1][1] == N and len(ranges) == BLOCKS
    assert (undo(Up) == U0).all()
    Xs, (Us,), none, _, same = online.cut_blocks("who", X, BLOCKS, rng, False, U0)
    assert none is None and Us is U0 and Xs is X and same(U0) is U0
    with pytest.raises(ValueError, match="^who: 2 documents cannot be split over 3 blocks$"):
        online.cut_blocks("who", X[:2], 3, rng, False)
