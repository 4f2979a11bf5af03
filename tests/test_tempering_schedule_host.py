"""TemperingSchedule (enstop_amd/tempered.py) on scripted validation perplexities: no engine, no GPU.

The schedule is a state machine: start() and every observe(perplexity) answer with a list of actions that ends in a burst or
in a stop.  Each script below is one of the situations the rule names; the expected action sequences are written out by hand
from the rule (start at beta = 1; keep a burst that improves on the best by more than rel_tol; otherwise restore, lower beta
by eta and grant ONE burst; stop when that one fails too, when beta would fall below beta_min, or when n_iter iterations are
spent), never produced by the code under test.
"""
import math

import pytest

from enstop_amd.tempered import TemperingSchedule

SNAP, RESTORE, STOP = ("snapshot",), ("restore",), ("stop",)


def burst(beta, iterations=10):
    return ("burst", beta, iterations)


def drive(schedule, perplexities):
    """every answer of the schedule, start() first; the script must end exactly at the stop"""
    answers = [schedule.start()]
    for p in perplexities:
        assert answers[-1][-1][0] == "burst", "the schedule stopped before the script ended"
        answers.append(schedule.observe(p))
    assert answers[-1][-1] == STOP and schedule.stopped, "the script ended before the schedule stopped"
    with pytest.raises(RuntimeError):
        schedule.observe(1.0)
    return answers


def test_defaults_are_the_documented_ones():
    s = TemperingSchedule()
    assert (s.eta, s.beta_min, s.rel_tol, s.n_iter_per_test, s.n_iter) == (0.9, 0.5, 1e-4, 10, 200)
    assert s.beta == 1.0 and s.selected is None and s.spent == 0
    import enstop_amd.tempered as t
    assert "this package's" in t.__doc__ and "choices" in t.__doc__       # the values are not the paper's


def test_monotone_improvement_runs_to_n_iter_at_beta_one():
    s = TemperingSchedule(n_iter=45, n_iter_per_test=10)
    ppl = [500.0, 400.0, 390.0, 380.0, 379.0]
    answers = drive(s, ppl)
    assert answers == [[SNAP, burst(1.0)], [SNAP, burst(1.0)], [SNAP, burst(1.0)], [SNAP, burst(1.0)],
                       [SNAP, burst(1.0, 5)],                         # the budget's remainder
                       [SNAP, STOP]]
    assert s.spent == 45 and s.beta == 1.0
    assert s.selected == s.history[-1] and s.selected["perplexity"] == 379.0 and s.selected["spent"] == 45
    assert [h["improved"] for h in s.history] == [True] * 5


def test_immediate_failure_keeps_the_first_burst():
    s = TemperingSchedule()
    answers = drive(s, [500.0, 510.0, 505.0])
    assert answers == [[SNAP, burst(1.0)], [SNAP, burst(1.0)], [RESTORE, burst(0.9)], [RESTORE, STOP]]
    assert s.selected["perplexity"] == 500.0 and s.selected["beta"] == 1.0 and s.selected["spent"] == 10
    assert s.spent == 30                                              # discarded bursts count


def test_improvement_after_the_first_lowering_and_failure_after_the_second():
    s = TemperingSchedule()
    answers = drive(s, [500.0, 450.0, 460.0, 440.0, 445.0, 441.0])
    b2 = 0.9 * 0.9
    assert answers == [[SNAP, burst(1.0)], [SNAP, burst(1.0)], [SNAP, burst(1.0)],
                       [RESTORE, burst(0.9)],                        # 460 > 450: first lowering
                       [SNAP, burst(0.9)],                           # 440 improves: kept, same beta goes on
                       [RESTORE, burst(b2)],                         # 445: second lowering
                       [RESTORE, STOP]]                              # 441 does not beat 440: the one burst failed
    assert s.selected["perplexity"] == 440.0 and s.selected["beta"] == 0.9 and s.selected["spent"] == 40
    assert [h["beta"] for h in s.history] == [1.0, 1.0, 1.0, 0.9, 0.9, b2]


def test_reaching_beta_min_stops():
    # every lowered burst improves, the one after it fails: beta walks down 1, .8, .64, .512 and 0.4096 < 0.5 is refused
    s = TemperingSchedule(eta=0.8, beta_min=0.5)
    ppl, p = [], 1000.0
    for _ in range(4):
        ppl += [p, p + 1.0]              # kept, then a failure at the same beta
        p -= 100.0
    # the first failure of each pair lowers beta; the burst granted to the new beta is the next pair's improvement
    answers = drive(s, ppl)
    betas = [1.0, 0.8, 0.8 * 0.8, 0.8 * 0.8 * 0.8]
    want = [[SNAP, burst(1.0)]]
    for i, b in enumerate(betas):
        want.append([SNAP, burst(b)])                                 # improvement at b
        want.append([RESTORE, burst(0.8 * b)] if i < 3 else [RESTORE, STOP])
    assert answers == want
    assert 0.8 * betas[-1] < 0.5 <= betas[-1]
    assert s.selected["beta"] == betas[-1] and s.selected["perplexity"] == 700.0


def test_an_improvement_smaller_than_rel_tol_is_none():
    # burst 2 (496) is within rel_tol of 500 -> restore and lower; burst 3 (494) improves by 1.2 % -> kept
    s = TemperingSchedule(rel_tol=1e-2)
    assert s.start() == [SNAP, burst(1.0)]
    assert s.observe(500.0) == [SNAP, burst(1.0)]
    assert s.observe(496.0) == [RESTORE, burst(0.9)]
    assert s.history[-1]["improved"] is False
    assert s.observe(494.0) == [SNAP, burst(0.9)]
    assert s.selected["perplexity"] == 494.0
    # exactly at the tolerance is not "more than": 495 = 500 (1 - 0.01)
    s = TemperingSchedule(rel_tol=1e-2)
    s.start()
    s.observe(500.0)
    assert s.observe(495.0) == [RESTORE, burst(0.9)]


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_a_perplexity_that_is_not_finite_is_no_improvement(bad):
    s = TemperingSchedule()
    answers = drive(s, [bad, bad])                                    # from the first burst on: the starting factors are kept
    assert answers == [[SNAP, burst(1.0)], [RESTORE, burst(0.9)], [RESTORE, STOP]]
    assert s.selected is None and math.isinf(s.best)
    s = TemperingSchedule()
    answers = drive(s, [500.0, bad, 490.0, bad, bad])
    assert answers == [[SNAP, burst(1.0)], [SNAP, burst(1.0)], [RESTORE, burst(0.9)], [SNAP, burst(0.9)],
                       [RESTORE, burst(0.9 * 0.9)], [RESTORE, STOP]]
    assert s.selected["perplexity"] == 490.0 and s.best == 490.0


def test_budget_spent_on_a_failure_stops_with_a_restore_and_zero_budget_does_nothing():
    s = TemperingSchedule(n_iter=20)
    assert drive(s, [500.0, 600.0]) == [[SNAP, burst(1.0)], [SNAP, burst(1.0)], [RESTORE, STOP]]
    s = TemperingSchedule(n_iter=0)
    assert s.start() == [SNAP, STOP] and s.stopped


def test_replaying_the_history_reproduces_the_actions():
    s = TemperingSchedule(eta=0.7, beta_min=0.3, n_iter=120, n_iter_per_test=7)
    drive(s, [900.0, 800.0, 810.0, 790.0, 789.99, 700.0, 701.0, 702.0])
    again = TemperingSchedule(eta=0.7, beta_min=0.3, n_iter=120, n_iter_per_test=7)
    again.start()
    for h in s.history:
        assert again.observe(h["perplexity"]) == h["actions"]
    assert again.selected == s.selected and again.stopped


def test_arguments_are_checked():
    for kw in (dict(eta=1.0), dict(eta=0.0), dict(beta_min=0.0), dict(beta_min=1.5), dict(rel_tol=-1.0),
               dict(n_iter_per_test=0), dict(n_iter=-1), dict(rel_tol=float("nan"))):
        with pytest.raises(ValueError):
            TemperingSchedule(**kw)
    s = TemperingSchedule()
    with pytest.raises(RuntimeError):
        s.observe(1.0)                                                # nothing pending before start()
    s.start()
    with pytest.raises(RuntimeError):
        s.start()
