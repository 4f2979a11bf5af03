"""CPU: OnlineSchedule (enstop_amd/online.py), the state machine that decides what an online fit does next.  It never touches
an engine: step sizes against the formula, the fixed-rho override, the block order, the per-epoch stop on a synthetic
likelihood trace, and that a stopped schedule stays stopped."""
import math

import pytest

from enstop_amd.online import OnlineSchedule


def drive(schedule, trace):
    """run the schedule to its end, feeding trace[e] after epoch e; -> the steps handed out"""
    steps = []
    while True:
        step = schedule.next_step()
        if step is None:
            return steps
        steps.append(step)
        if step[1] == schedule.n_blocks - 1:
            schedule.end_epoch(trace[step[0]])


def test_the_step_sizes_follow_the_formula_and_the_blocks_go_in_order():
    s = OnlineSchedule(n_blocks=4, n_epochs=3, kappa=0.7, tau0=10.0, tolerance=0.0)
    steps = drive(s, [-3.0, -2.0, -1.0])
    assert [(e, b) for e, b, _ in steps] == [(e, b) for e in range(3) for b in range(4)]
    for t, (_, _, rho) in enumerate(steps):
        assert rho == (10.0 + t) ** (-0.7)               # t counts the steps from 0, across epochs
        assert 0.0 < rho <= 1.0
    assert s.rhos == [rho for _, _, rho in steps] and s.n_steps == 12 and s.n_epochs_done == 3
    assert s.log_likelihoods == [-3.0, -2.0, -1.0]
    assert s.rho_at(0) == 10.0 ** -0.7 and s.rho_at(90) == 100.0 ** -0.7


def test_a_fixed_rho_overrides_the_formula():
    s = OnlineSchedule(n_blocks=2, n_epochs=2, kappa=0.7, tau0=10.0, rho=0.25, tolerance=0.0)
    assert [rho for _, _, rho in drive(s, [-2.0, -1.0])] == [0.25] * 4
    assert OnlineSchedule(1, 1, rho=1.0).next_step() == (0, 0, 1.0)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="rho"):
            OnlineSchedule(2, 2, rho=bad)


def test_the_epoch_stop_on_a_synthetic_trace():
    # relative changes |L_e - L_(e-1)| / |L_e|: 1/9, 0.0112..., 0.00099...: the fourth epoch is the first below 1e-3
    trace = [-1000.0, -900.0, -890.0, -889.12, -889.0, -888.0]
    s = OnlineSchedule(n_blocks=3, n_epochs=6, tolerance=0.001)
    steps = drive(s, trace)
    assert abs(trace[3] - trace[2]) / abs(trace[3]) < 0.001 <= abs(trace[2] - trace[1]) / abs(trace[2])
    assert s.n_epochs_done == 4 and len(steps) == 12 and s.stopped
    assert s.log_likelihoods == trace[:4]
    # the cap
    s = OnlineSchedule(n_blocks=3, n_epochs=2, tolerance=0.001)
    assert len(drive(s, trace)) == 6 and s.n_epochs_done == 2 and s.stopped
    # a tolerance of 0 never stops on the likelihood, not even on an unchanged one; a NaN is no convergence
    s = OnlineSchedule(n_blocks=1, n_epochs=5, tolerance=0.0)
    assert len(drive(s, [-5.0] * 5)) == 5
    s = OnlineSchedule(n_blocks=1, n_epochs=3, tolerance=0.5)
    assert len(drive(s, [-5.0, float("nan"), -5.0])) == 3
    # the first epoch has nothing to compare with
    s = OnlineSchedule(n_blocks=1, n_epochs=3, tolerance=0.5)
    assert len(drive(s, [-5.0, -5.0, -5.0])) == 2


def test_end_epoch_answers_whether_another_epoch_follows_and_the_order_of_calls_is_enforced():
    s = OnlineSchedule(n_blocks=2, n_epochs=2, tolerance=0.0)
    with pytest.raises(RuntimeError):
        s.end_epoch(-1.0)                                # no epoch is complete yet
    s.next_step()
    with pytest.raises(RuntimeError):
        s.end_epoch(-1.0)
    s.next_step()
    with pytest.raises(RuntimeError):
        s.next_step()                                    # the epoch's likelihood comes first
    assert s.end_epoch(-2.0) is True
    s.next_step(), s.next_step()
    assert s.end_epoch(-1.0) is False


def test_a_stopped_schedule_stays_stopped():
    s = OnlineSchedule(n_blocks=2, n_epochs=1, tolerance=0.0)
    drive(s, [-1.0])
    assert s.stopped
    for _ in range(3):
        assert s.next_step() is None
    with pytest.raises(RuntimeError):
        s.end_epoch(-0.5)
    assert s.n_steps == 2 and s.log_likelihoods == [-1.0]
    empty = OnlineSchedule(n_blocks=2, n_epochs=0)
    assert empty.stopped and empty.next_step() is None


def test_bad_parameters_are_refused():
    for kwargs in (dict(n_blocks=0), dict(n_blocks=1, n_epochs=-1), dict(n_blocks=1, tau0=0.5), dict(n_blocks=1, kappa=-1.0),
                   dict(n_blocks=1, tolerance=-1e-3), dict(n_blocks=1, tolerance=float("nan"))):
        with pytest.raises(ValueError):
            OnlineSchedule(**kwargs)
    assert math.isclose(OnlineSchedule(1, tau0=1.0).rho_at(0), 1.0)
