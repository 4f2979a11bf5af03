"""The device math of variational Bayes LDA (enstop_amd/csrc/plsa_lda_math.hpp) on a CPU, against SciPy.

The header is free of HIP for a host compiler; tests/lda_math_host.cpp is a stand-alone program around it, built here with
the address and undefined-behaviour sanitizers.  The grid: 4 001 points spaced evenly in log x over 10^-6 .. 10^7, the
integers and half-integers up to 12 (the recurrence's every round count), both sides of the shift threshold 6 and of the
root 1.4616.

Error model.  digamma adds at most six reciprocals, a logarithm, 1 / (2 x) and a twelve-term series whose truncation is
below 3.2e-16: about ten roundings of 2^-53 each, relative to the largest of the magnitudes involved, which is
max(1, |psi|) up to the factor log(x + 6) <= 3 near the root.  SciPy's psi carries a few units of its own.  So
    |digamma(x) - psi(x)| <= 2^-47 max(1, |psi(x)|)                  (64 units of 2^-53: the model's ten, SciPy's, a margin of 4)
and, what a table entry needs: the absolute error is at most 2^-40 wherever psi(x) >= -88, the range in which
exp(psi(x) - psi(S)) can be a normal float32.  exp_digamma_diff inherits the absolute error of its two digammas as a relative
error, plus exp's rounding.
"""
import os
import subprocess

import numpy as np
import pytest
from scipy.special import psi

from conftest import ROOT


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lda_math") / "lda_math_host")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O2",
           "-g", os.path.join(ROOT, "tests", "lda_math_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def grid():
    x = np.concatenate([np.logspace(-6, 7, 4001), np.arange(1, 25) / 2.0, [6.0 - 2.0 ** -40, 6.0 + 2.0 ** -40],
                        [1.4616321449683623 * (1 + e) for e in (-1e-3, -1e-9, 0.0, 1e-9, 1e-3)], [0.012, 1.0 / 64, 1e-3]])
    return x


def evaluate(program, x, s):
    text = "".join("%.17g %.17g\n" % pair for pair in zip(x, s))
    out = subprocess.run([program], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    got = np.array([[float(v) for v in line.split()] for line in out.stdout.splitlines()])
    assert got.shape == (x.shape[0], 2)
    return got[:, 0], got[:, 1]


def test_digamma_against_scipy(program):
    x = grid()
    got, _ = evaluate(program, x, x + 1.0)
    want = psi(x)
    err = np.abs(got - want)
    table = want >= -88.0
    assert table.sum() > 2500
    print("\ndigamma: largest absolute error where psi >= -88: %.3g (bound %.3g); largest error / max(1, |psi|): %.3g (bound %.3g)"
          % (err[table].max(), 2.0 ** -40, (err / np.maximum(1.0, np.abs(want))).max(), 2.0 ** -47))
    assert err[table].max() <= 2.0 ** -40
    assert (err / np.maximum(1.0, np.abs(want))).max() <= 2.0 ** -47


def test_exp_digamma_diff_against_scipy(program):
    """entries of a row that sums to S = x + r, r the rest of the row: in (0, 1], within the two digammas' absolute errors and
    exp's rounding of SciPy's value"""
    x = grid()
    rs = np.random.RandomState(0)
    s = x + rs.gamma(2.0, 5.0, size=x.shape[0])
    _, got = evaluate(program, x, s)
    want = np.exp(psi(x) - psi(s))
    assert (got >= 0).all() and (got <= 1).all()
    live = want > 1e-300
    rel = np.abs(got - want)[live] / want[live]
    bound = 2.0 ** -47 * (np.maximum(1.0, np.abs(psi(x))) + np.maximum(1.0, np.abs(psi(s))))[live] + 2.0 ** -51
    print("\nexp_digamma_diff: largest relative error / bound %.3g" % (rel / bound).max())
    assert (rel <= bound).all()
    # the float32 normal range ends at a prior of about 0.012: an entry that small in a row summing to 100 is below it
    assert np.exp(psi(0.012) - psi(100.0)) < 2.0 ** -126 < np.exp(psi(0.013) - psi(100.0))


def test_bad_arguments(program):
    got, _ = evaluate(program, np.array([0.0, -1.0, np.inf]), np.array([1.0, 1.0, 1.0]))
    assert np.isnan(got[0]) and np.isnan(got[1]) and got[2] == np.inf
