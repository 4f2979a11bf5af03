"""The likelihood-test loop of the fit drivers (enstop_amd/csrc/plsa_fit_schedule.hpp) on a CPU.

The header is free of HIP: tests/fit_schedule_host.cpp drives plsa::fit::run_materialised and plsa::fit::run_fused with a
backend that only keeps book (which S_i sits in which of three buffer slots, which likelihood is carried or in flight) and
aborts where a real context would lose a likelihood or overwrite factors a stop must return.  It is built as a stand-alone
program with the address and undefined-behaviour sanitizers, fed every case on stdin, and held to the reference's loop as
test_fit_driver.py restates it (reference_loop, stop32): iteration count, the state left behind (the current slot holds
S_count and is slot 0 or 1) and the trace in bits.

Cases: the plain, speculating, graph-replaying and materialised forms; n_iter 0..12 x n_iter_per_test 1..5; tolerance 0 and
every stop stop_choices offers on a trace whose changes fall from test to test; PLSA_TRACE_LL on and off; the three stop
rules, the refit's (enstop/plsa.py:913-918, restated below) on a trace that turns positive -- the branch no corpus reaches,
every corpus having a negative likelihood; a flat trace (the `change == 0` arm); a NaN in the trace (the weighted fits
produce one: no stop, no trap); a trace capacity below the number of likelihoods (counted, not written); no trace pointer;
and the speculative second enqueue failing (the factors a stop returns are current again).
"""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_fit_driver import reference_loop, stop32, stop_choices

PLAIN, SPECULATING, GRAPH, MATERIALISED = range(4)
FIT, FIT_NO_ZERO_ARM, REFIT = range(3)
N_ITERS = range(13)
PER_TESTS = range(1, 6)
N_VALUES = max(N_ITERS) + 2


def rule_fit(cur, prev, tol):
    return (True, prev) if stop32(cur, prev, tol) else (False, cur)


def rule_no_zero_arm(cur, prev, tol):
    return (True, prev) if stop32(cur, prev, tol, zero_arm=False) else (False, cur)


def rule_refit(cur, prev, tol):
    """enstop/plsa.py:913-918: `if current > 0: change = |current - previous|; if change / |current| < tolerance: break;
    else: previous = current` -- a likelihood that is not positive is neither tested nor remembered"""
    if np.float32(cur) > 0:
        return rule_no_zero_arm(cur, prev, tol)
    return False, prev


RULES = {FIT: rule_fit, FIT_NO_ZERO_ARM: rule_no_zero_arm, REFIT: rule_refit}


def expected(form, rule, n_iter, per_test, tol, ride, trail, trace):
    """reference_loop with the rule (one of RULES, or a function like them) and PLSA_TRACE_LL as parameters: without the flag
    the test of the last iteration, whose verdict changes nothing, is not evaluated; the materialised loop has k_loglik's
    value everywhere"""
    if form == MATERIALISED:
        ride = trail
    if n_iter == 0:
        return 0, [trail[0]]
    out, prev = [ride[0]], ride[0]
    for i in range(n_iter):
        if i % per_test == 0:
            last = i + 1 == n_iter
            if last and not trace:
                break
            out.append(trail[i + 1] if last else ride[i + 1])
            if not last:
                stop, prev = RULES.get(rule, rule)(out[-1], prev, tol)
                if stop:
                    return i + 1, out
    return n_iter, out


def f32(values):
    return [np.float32(v) for v in values]


FALLING = f32(-800.0 - 200.0 * 0.5 ** i for i in range(N_VALUES))          # changes fall from test to test at every cadence
TURNING = f32(6.0 - 9.0 * 0.8 ** i for i in range(N_VALUES))               # -3, -1.2, 0.24, 1.39, ...: turns positive
FLAT = f32([-5.0] * N_VALUES)
WITH_NAN = list(FALLING)
WITH_NAN[2] = np.float32("nan")
TURNING_TOLERANCES = (0.0, 1e-3, 0.05, 0.2, 0.5, 2.0, 10.0, 20.0)          # from "never" to "at the first positive value"


def trailing(ride):
    """k_loglik's value of the same factors: another float32 near it (NaN stays NaN)"""
    return f32(v - np.float32(0.25) for v in ride)


def forms(n_iter, per_test):
    """plsa_fit speculates only where no test rides on the pass enqueued ahead and there is something to enqueue ahead"""
    return [f for f in (PLAIN, SPECULATING, GRAPH, MATERIALISED) if f != SPECULATING or (per_test >= 2 and n_iter >= 3)]


def bits(values):
    return [int(np.float32(v).view(np.uint32)) for v in values]


@functools.lru_cache(maxsize=None)
def all_cases():
    """-> [(form, rule, n_iter, per_test, tol, trace, cap, ride, trail)], [what `expected` says of each]"""
    cases = []
    for n_iter in N_ITERS:
        for per_test in PER_TESTS:
            n_riding = len([i for i in range(n_iter) if i % per_test == 0 and i + 1 < n_iter])
            for form in forms(n_iter, per_test):
                for trace in (True, False):
                    def add(rule, tol, ride, cap=-1):
                        cases.append((form, rule, n_iter, per_test, float(tol), trace, cap, ride, trailing(ride)))
                    ride = FALLING
                    tols = [0.0]
                    if n_riding:
                        _, trace0 = expected(form, FIT, n_iter, per_test, 0.0, ride, trailing(ride), True)
                        tols += [tol for _, tol in stop_choices(trace0, n_riding)]
                    for tol in tols:
                        for rule in RULES:
                            add(rule, tol, ride)
                        add(FIT, tol, ride, cap=2)               # fewer places than likelihoods (from two tests on)
                        add(FIT, tol, ride, cap=-2)              # no trace pointer: counted only
                    for tol in TURNING_TOLERANCES:
                        add(REFIT, tol, TURNING)
                    for rule in RULES:
                        add(rule, 0.0, FLAT)
                        add(rule, 0.0, WITH_NAN)
                        add(rule, 0.01, WITH_NAN)
    return cases, [expected(*c[:5], c[7], c[8], c[5]) for c in cases]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fit_schedule") / "fit_schedule_host")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1",
           "-g", os.path.join(ROOT, "tests", "fit_schedule_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def run(program, cases, fail_at=-1):
    lines = []
    for form, rule, n_iter, per_test, tol, trace, cap, ride, trail in cases:
        head = [form, rule, n_iter, per_test, tol.hex(), int(trace), cap, fail_at, len(ride)]
        lines.append(" ".join(str(v) for v in head) + " " + " ".join("%08x" % b for b in bits(ride) + bits(trail)))
    out = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = [line.split() for line in out.stdout.splitlines()]
    assert len(rows) == len(cases)
    return [([int(v) for v in row[:6]], [int(v, 16) for v in row[6:]]) for row in rows]


def test_the_restated_loop_is_the_reference_loop():
    for (form, rule, n_iter, per_test, tol, trace, cap, ride, trail), got in zip(*all_cases()):
        if rule == FIT and trace:
            want = reference_loop(n_iter, per_test, tol, trail if form == MATERIALISED else ride, trail)
            assert got[0] == want[0] and bits(got[1]) == bits(want[1]), (form, n_iter, per_test, tol)


def test_cases_reach_every_branch():
    cases, want = all_cases()
    stopped = {(c[0], c[1]) for c, (iters, _) in zip(cases, want) if iters < c[2]}
    assert stopped == {(form, rule) for form in range(4) for rule in RULES}       # every rule stops every form somewhere

    def remembers_everything(cur, prev, tol):                    # a refit rule that takes a non-positive value for `previous`
        stop, _ = rule_refit(cur, prev, tol)
        return stop, prev if stop else cur
    for form in range(4):                                        # ... is told from the reference's in every form
        assert any(expected(form, remembers_everything, *c[2:5], c[7], c[8], c[5])[0] != iters
                   for c, (iters, _) in zip(cases, want) if c[0] == form and c[7] is TURNING)
    assert any(len(trace) > 2 for c, (_, trace) in zip(cases, want) if c[6] == 2)


def test_every_loop_form_against_the_reference_loop(program):
    cases, want = all_cases()
    got = run(program, cases)
    for case, (want_iters, want_trace), ((rc, iters, cur, state, count, written), trace_bits) in zip(cases, want, got):
        form, rule, n_iter, per_test, tol, trace, cap, ride, trail = case
        tag = "form %d rule %d n_iter %d per_test %d tol %r trace %d cap %d" % (form, rule, n_iter, per_test, tol, trace, cap)
        assert rc == 0, tag
        assert iters == want_iters, tag
        assert state == iters and cur in (0, 1), tag                # the current buffers hold S_count, addressed as 0 or 1
        assert count == len(want_trace), tag
        kept = 0 if cap == -2 else len(want_trace) if cap < 0 else min(cap, len(want_trace))
        assert written == kept and trace_bits == bits(want_trace[:kept]), tag


def test_a_failed_speculative_enqueue_returns_to_the_marked_factors(program):
    # n_iter_per_test 2: pass 0 carries the initial likelihood, pass 1 the test of iteration 0; the speculating loop sends it
    # off, advances to S_2's buffers and enqueues pass 2 (the enqueue with index 2) before it waits
    case = (SPECULATING, FIT, 5, 2, 0.0, True, -1, FALLING, trailing(FALLING))
    ((rc, iters, cur, state, count, written), _), = run(program, [case], fail_at=2)
    assert (rc, iters, cur, state) == (7, 1, 1, 1)
