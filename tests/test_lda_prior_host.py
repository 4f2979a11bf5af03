"""The host arithmetic and the launch arithmetic of LDA's learned priors (enstop_amd/csrc/plsa_lda_prior_math.hpp,
plsa_lda_prior_plan.hpp) on a CPU, against SciPy.

Both headers are free of HIP; tests/lda_prior_host.cpp is a stand-alone program around them, built here with the address and
undefined-behaviour sanitizers.

Error model of trigamma, on the grid of test_lda_math_host.py.  The series is cut behind n = 12: the first omitted term,
B_26 / x^27, is 1.4e-15 at x = 6, which is 2^-46.9 of psi'(6) = 0.181, and smaller beyond.  Below 6 the recurrence adds up to six
positive terms 1 / x^2 to a value that carries that relative error: a sum of positive terms, so the relative error does not
grow.  The arithmetic is about sixteen roundings of 2^-53 (a reciprocal, Horner's twelve, the recurrence): 2^-49.  SciPy's
polygamma(1, x) is the Hurwitz zeta function, good to a few units.  So
    |trigamma(x) - psi'(x)| <= 2^-46 psi'(x)
(2^-46.9 + 2^-49 + SciPy's is 2^-46.5).  The maximisers use psi' for the curvature alone.

The maximisers.  F(alpha) = n [lgamma(sum alpha) - sum lgamma(alpha_z)] + sum alpha_z T_z with T_z = sum_d log theta_dz of n = 2000
samples theta_d ~ Dirichlet(alpha_true) is the Dirichlet log-likelihood: real sums of the kind gamma gives.  The routine's rule
is |g_z| <= 1e-9 (n |psi(sum alpha)| + n |psi(alpha_z)| + |T_z|); recomputed here with SciPy's psi, whose values differ from the
routine's digamma by at most 2^-47 max(1, |psi|) each (test_lda_math_host.py), the gradient may exceed the rule by 2 n 2^-47 of
the same scale: the assertion allows 1e-9 + 2^-45.  The independent maximiser is SciPy's trust-region Newton method on
-F(exp x) with the exact gradient and Hessian, polished by plain Newton steps until its gradient is at rounding level.
L-BFGS-B agreed with the routine to 3e-6 relative, which was L-BFGS-B's own residue; this reference reaches 1e-10 and the
assertion is held at 1e-8.  The routine's own rule leaves about that much: |g_z| <= 1e-9 scale_z against a curvature of
n psi'(alpha_z) is a relative distance of 1e-9 scale_z / (n alpha_z psi'(alpha_z)), and scale_z / n is 1 to 10 times
alpha_z psi'(alpha_z) for alpha_z in the range of these problems (0.04 .. 1.3); Newton's last step lands far inside it.
"""
import os
import subprocess

import numpy as np
import pytest
from scipy.optimize import minimize, minimize_scalar
from scipy.special import polygamma

import lda_prior_model as pm
from conftest import ROOT
from test_lda_math_host import grid

N = 2000
FLOOR = 1e-6
KS = [1, 2, 3, 8, 64, 1024]
AGREE = 1e-8


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lda_prior") / "lda_prior_host")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O2",
           "-g", os.path.join(ROOT, "tests", "lda_prior_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def run(program, text):
    out = subprocess.run([program], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    return out.stdout.split()


def maximise_alpha(program, start, T, n):
    words = run(program, "alpha %d %.17g\n%s\n%s\n" % (len(start), n, " ".join("%.17g" % v for v in start),
                                                       " ".join("%.17g" % v for v in T)))
    assert len(words) == 3 + len(start)
    return np.array([float(v) for v in words[3:]]), dict(rounds=int(words[0]), converged=int(words[1]), moved=int(words[2]))


def maximise_eta(program, k, m, start, T):
    words = run(program, "eta %.17g %.17g %.17g %.17g\n" % (k, m, start, T))
    assert len(words) == 4
    return float(words[3]), dict(rounds=int(words[0]), converged=int(words[1]), moved=int(words[2]))


def alpha_true(k):
    if k == 8:
        return np.array(pm.PLANTED["doc_alpha"])
    rs = np.random.RandomState(k)
    return np.where(rs.rand(k) < 0.25, 0.8, 0.1) * (0.5 + rs.rand(k))


def dirichlet_sums(k, seed=0):
    """T_z = sum_d log theta_dz of N samples of Dirichlet(alpha_true(k)); k = 1: theta = 1, T = 0"""
    if k == 1:
        return np.zeros(1)
    theta = np.random.RandomState(100 + seed).dirichlet(alpha_true(k), size=N)
    logs = np.log(theta)
    assert np.isfinite(logs).all()
    return logs.sum(0)


def scipy_alpha(T, n, start):
    def f(x):
        return -pm.alpha_objective(np.exp(x), T, n)

    def grad(x):
        a = np.exp(x)
        return -pm.alpha_gradient(a, T, n)[0] * a

    def hess(x):
        a = np.exp(x)
        g = pm.alpha_gradient(a, T, n)[0]
        H = n * polygamma(1, a.sum()) * np.ones((a.size, a.size)) - np.diag(n * polygamma(1, a))
        return -(H * np.outer(a, a) + np.diag(g * a))
    res = minimize(f, np.log(start), jac=grad, hess=hess, method="trust-exact", options=dict(gtol=1e-9 * n, maxiter=2000))
    # polish: the trust-region method stops on an absolute gradient; a few plain Newton steps in x take it to rounding level
    x = res.x
    for _ in range(20):
        step = np.linalg.solve(hess(x), grad(x))
        x = x - step
        if np.abs(step).max() < 1e-14:
            break
    return np.exp(x)


def test_trigamma_against_scipy(program):
    x = grid()
    words = run(program, "trigamma %d\n%s\n" % (len(x), "\n".join("%.17g" % v for v in x)))
    got = np.array([float(v) for v in words])
    want = polygamma(1, x)
    rel = np.abs(got - want) / want
    print("\ntrigamma: largest relative error %.3g at x = %.6g (bound %.3g)" % (rel.max(), x[rel.argmax()], 2.0 ** -46))
    assert got.shape == x.shape and (rel <= 2.0 ** -46).all()
    words = run(program, "trigamma 3\n0 -1 inf\n")
    assert np.isnan(float(words[0])) and np.isnan(float(words[1])) and float(words[2]) == 0.0


@pytest.mark.parametrize("k", KS)
def test_alpha_maximiser_against_scipy(program, k):
    T = dirichlet_sums(k)
    start = np.full(k, 1.0 / k)
    got, report = maximise_alpha(program, start, T, N)
    if k == 1:
        assert got[0] == start[0] and not report["moved"]
        return
    assert (got >= FLOOR).all() and report["converged"] == 1 and report["moved"] == 1 and report["rounds"] < 100
    g, scale = pm.alpha_gradient(got, T, N)
    free = got > FLOOR
    assert free.all()
    ratio = (np.abs(g) / scale)[free].max()
    want = scipy_alpha(T, N, start)
    g_want, scale_want = pm.alpha_gradient(want, T, N)
    agree = (np.abs(got - want) / want).max()
    print("\nk=%d: %d rounds, |g| / scale %.3g (rule 1e-9), SciPy's %.3g; largest relative difference %.3g; alpha %.4g .. %.4g"
          % (k, report["rounds"], ratio, (np.abs(g_want) / scale_want).max(), agree, got.min(), got.max()))
    assert ratio <= 1e-9 + 2.0 ** -45
    assert (np.abs(g_want) / scale_want).max() <= 1e-9          # the reference is at least as converged
    assert agree <= AGREE
    assert pm.alpha_objective(got, T, N) >= pm.alpha_objective(start, T, N)
    if k == 8:                                               # the planted mix comes back: two heavy topics
        assert got[:2].min() > 3 * got[2:].max()


def test_alpha_maximiser_from_other_starts_and_at_its_own_result(program):
    k = 8
    T = dirichlet_sums(k)
    first, _ = maximise_alpha(program, np.full(k, 1.0 / k), T, N)
    for start in (np.full(k, 50.0), np.full(k, 1e-4), np.linspace(0.01, 3.0, k)):
        got, report = maximise_alpha(program, start, T, N)
        assert report["converged"] == 1 and (np.abs(got - first) / first).max() <= AGREE, (start, got, report)
        assert pm.alpha_objective(got, T, N) >= pm.alpha_objective(start, T, N)
    again, report = maximise_alpha(program, first, T, N)
    assert report["rounds"] == 0 and (again == first).all()


@pytest.mark.parametrize("depth", [1e6, 1e9])
def test_a_topic_nobody_uses_ends_at_the_floor(program, depth):
    """T_0 = -depth n.  The other seven topics have alpha_true = 0.1 .. 0.8 scaled so that their maximiser sums to less than 1:
    then psi(sum alpha) - psi(1e-6) < 1e6 and the gradient of topic 0 is negative on the floor at either depth"""
    k = 8
    T = dirichlet_sums(k)
    T[0] = -depth * N
    T[1:] *= 3.0                                             # colder sums: smaller alpha (their maximiser sums to 0.3)
    start = np.full(k, 1.0 / k)
    got, report = maximise_alpha(program, start, T, N)
    g, scale = pm.alpha_gradient(got, T, N)
    print("\ndepth %g: alpha_0 = %.9g, g_0 = %.3g, sum of the others %.4f, %d rounds, |g| / scale of the others %.3g"
          % (depth, got[0], g[0], got[1:].sum(), report["rounds"], (np.abs(g) / scale)[1:].max()))
    assert got[1:].sum() < 0.9
    assert got[0] == FLOOR and g[0] < 0 and (got[1:] > FLOOR).all()
    assert report["converged"] == 1 and ((np.abs(g) / scale)[1:] <= 1e-9 + 2.0 ** -45).all()
    assert pm.alpha_objective(got, T, N) >= pm.alpha_objective(start, T, N)


def test_an_update_that_cannot_raise_f_returns_the_start(program):
    """NaN sums: no candidate compares >= F, nothing is taken, the start comes back bit for bit"""
    start = np.array([0.3, 0.2, 0.1])
    got, report = maximise_alpha(program, start, np.array([np.nan, -1.0, -2.0]), N)
    assert (got == start).all() and report["moved"] == 0


@pytest.mark.parametrize("k,m,eta_true", [(8, 480, 0.05), (3, 50, 0.7), (64, 2000, 0.05), (1, 480, 0.3), (8, 1, 0.3)])
def test_eta_maximiser_against_scipy(program, k, m, eta_true):
    rs = np.random.RandomState(k + m)
    T = 0.0 if m == 1 else float(np.log(rs.dirichlet(np.full(m, eta_true), size=k)).sum())
    assert np.isfinite(T)
    start = 0.01
    got, report = maximise_eta(program, k, m, start, T)
    if m == 1:
        assert got == start and not report["moved"]
        return
    res = minimize_scalar(lambda x: -pm.eta_objective(np.exp(x), T, k, m), bracket=(np.log(1e-4), np.log(10.0)),
                          method="brent", options=dict(xtol=1e-12))
    want = float(np.exp(res.x))
    g, scale = pm.eta_gradient(got, T, k, m)
    print("\nk=%d m=%d: eta %.6g (SciPy %.6g, planted %.3g), %d rounds, |g| / scale %.3g" % (k, m, got, want, eta_true,
                                                                                         report["rounds"], abs(g) / scale))
    assert report["converged"] == 1 and got >= FLOOR and abs(g) <= (1e-9 + 2.0 ** -45) * scale
    assert abs(got - want) <= 1e-6 * want                    # Brent on F resolves its maximiser to sqrt(2^-53) at best
    assert pm.eta_objective(got, T, k, m) >= pm.eta_objective(start, T, k, m)


def test_the_slabs_of_the_sums_cut_the_rows_whatever_the_cap(program):
    """k_lda_logmean's loops, walked for every thread: the slab count is min(4096, max(rows, 1)) -- the plan has no grid cap to
    depend on --, the slabs are consecutive ranges that cover the rows, every entry of the table [rows, kp] is read by exactly
    one thread, a strand's rows ascend.  kp: one quarter, a width that does not divide 256 (24), 132 (one strand, idle
    threads), 256, 260 and 1024 (more than one batch of topics)."""
    cases = [(rows, kp) for rows in (0, 1, 255, 640, 4095, 4096, 4097, 9001) for kp in (4, 8, 24, 64, 132, 256, 260, 1024)
             if rows * kp <= 4097 * 260 or kp == 1024 and rows <= 640]
    words = run(program, "".join("logmean %d %d\n" % case for case in cases))
    assert len(words) == 4 * len(cases)
    for i, (rows, kp) in enumerate(cases):
        slabs, cut_ok, once, order_ok = (int(v) for v in words[4 * i: 4 * i + 4])
        assert slabs == min(4096, max(rows, 1)) and cut_ok == 1 and once == 1 and order_ok == 1, (rows, kp)
    text = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_lda_prior_kernels.hpp")).read()
    for stated in ("plan::prior_rows_first(rows, gridDim.x, blockIdx.x)", "plan::logmean_span(kp, zb)", "plan::logmean_strands(span)",
                   "plan::smooth_first(blockIdx.x, threadIdx.x)", "plan::smooth_pad_mask("):
        assert stated in text, stated
    host = open(os.path.join(ROOT, "enstop_amd", "csrc", "plsa_lda_priors.hpp")).read()
    assert "plsa::plan::lda_logmean_grid(rows)" in host and "grid_cap" not in host[host.index("int run_lda_logmean("):host.index("int run_lda_prior_stats(")]


def test_the_schedule_of_the_updates(program):
    cases = [(done, start, every) for start in (1, 3, 20) for every in (1, 2, 10) for done in range(1, 45)]
    words = run(program, "".join("due %d %d %d\n" % case for case in cases))
    for (done, start, every), word in zip(cases, words):
        assert int(word) == int(done in range(start, 100, every)), (done, start, every)
