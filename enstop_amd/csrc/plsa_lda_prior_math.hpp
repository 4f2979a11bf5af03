// plsa_lda_prior_math.hpp -- the host arithmetic of LDA's learned priors (plsa_lda_priors.hpp): the
// trigamma function and the two Newton maximisers, free of HIP like plsa_lda_math.hpp, on which it stands.
// tests/lda_prior_host.cpp runs all of it on a CPU and tests/test_lda_prior_host.py compares it with SciPy.
//
// trigamma(x), x > 0: psi'(x) = psi'(x + 1) + 1 / x^2 shifts x up to x >= 6, then
//     psi'(x) ~ 1 / x + 1 / (2 x^2) + sum_n B_2n / x^(2n+1)
// with the twelve terms n = 1 .. 12 (Horner in 1 / x^2).  At x = 6 the first omitted term is 1.4e-15, 2^-46.9 of
// psi'(6) = 0.181, and falls off like x^-27; the recurrence adds positive terms only, so the relative error does not grow on
// the way down.  The maximisers use psi' for the curvature alone: its error moves their steps, never their fixed point.
//
// The document side.  With gamma fixed the part of the bound that depends on alpha is
//     F(alpha) = n [lgamma(sum_z alpha_z) - sum_z lgamma(alpha_z)] + sum_z alpha_z T_z,        T_z = sum_d (psi(gamma_dz) - psi(S_d)),
// concave, with gradient g_z = n (psi(sum alpha) - psi(alpha_z)) + T_z and Hessian diag(h) + c 1 1^T, h_z = -n psi'(alpha_z),
// c = n psi'(sum alpha): the Newton step is linear in k (Blei, Ng, Jordan 2003, A.4.2),
//     b = sum_j (g_j / h_j) / (1 / c + sum_j 1 / h_j),        step_z = (g_z - b) / h_z,        alpha <- alpha - step.
// maximise_alpha's contract:
//   * every component of the result is >= PRIOR_FLOOR;
//   * a component that sits on the floor with g_z <= 0 is held there (it leaves the Newton system of that round); a component
//     the step would take below the floor lands on the floor; a step that lowers F is halved, 40 times at most.  Halving the
//     whole step until no component crosses would hold every other component back by the same factor, round after round;
//   * it stops when every component that is not held has |g_z| <= 1e-9 (n |psi(sum alpha)| + n |psi(alpha_z)| + |T_z|), the scale
//     of the gradient's own terms, or after 100 rounds;
//   * the result is returned only if F(result) >= F(start): otherwise the start comes back unchanged;
//   * k = 1 has F = alpha T with T = 0: the input comes back.
// "Lowers F" allows for the rounding of F itself, 2^-50 of the sum of the magnitudes it is formed from: next to the maximum a
// Newton step changes F by less than that, and a strict comparison would halve such a step to nothing.
//
// The topic side, eta symmetric: F(eta) = k [lgamma(m eta) - m lgamma(eta)] + eta T, T = sum_z sum_w (psi(lambda_zw) - psi(S_z)),
// g = k m (psi(m eta) - psi(eta)) + T, h = k m (m psi'(m eta) - psi'(eta)) < 0: the same rules in one dimension.
#pragma once

#include <cmath>
#include <vector>

#include "plsa_lda_math.hpp"

namespace plsa {
namespace lda {

constexpr double PRIOR_FLOOR = 1e-6;
constexpr int PRIOR_ROUNDS = 100;
constexpr int PRIOR_HALVINGS = 40;
constexpr double PRIOR_GRADIENT_RULE = 1e-9;

inline double trigamma(double x) {
    if (!(x > 0.0)) return NAN;
    double shift = 0.0;
    while (x < 6.0) {                // at most six rounds
        shift += 1.0 / (x * x);
        x += 1.0;
    }
    const double r = 1.0 / x, r2 = r * r;
    // B_2n, n = 12 .. 1
    double s = -236364091.0 / 2730.0;
    s = s * r2 + 854513.0 / 138.0;
    s = s * r2 - 174611.0 / 330.0;
    s = s * r2 + 43867.0 / 798.0;
    s = s * r2 - 3617.0 / 510.0;
    s = s * r2 + 7.0 / 6.0;
    s = s * r2 - 691.0 / 2730.0;
    s = s * r2 + 5.0 / 66.0;
    s = s * r2 - 1.0 / 30.0;
    s = s * r2 + 1.0 / 42.0;
    s = s * r2 - 1.0 / 30.0;
    s = s * r2 + 1.0 / 6.0;
    return r + 0.5 * r2 + s * r2 * r + shift;
}

// what a maximiser did: Newton rounds taken, whether the gradient rule was met, whether the result (not the start) came back
struct PriorReport {
    int rounds = 0;
    bool converged = false, moved = false;
};

// F(alpha) and the sum of the magnitudes it is formed from
inline double alpha_objective(const double *alpha, const double *T, int k, double n, double *scale = nullptr) {
    double sum = 0.0, lg = 0.0, lin = 0.0, mag = 0.0;
    for (int z = 0; z < k; ++z) {
        const double l = std::lgamma(alpha[z]);
        sum += alpha[z];
        lg += l;
        lin += alpha[z] * T[z];
        mag += n * std::fabs(l) + std::fabs(alpha[z] * T[z]);
    }
    const double top = std::lgamma(sum);
    if (scale) *scale = mag + n * std::fabs(top);
    return n * (top - lg) + lin;
}

// g_z of F at alpha; returns whether every component that is not held (on the floor with g_z <= 0) meets the gradient rule
inline bool alpha_gradient(const double *alpha, const double *T, int k, double n, double *g, double rule = PRIOR_GRADIENT_RULE) {
    double sum = 0.0;
    for (int z = 0; z < k; ++z) sum += alpha[z];
    const double psum = digamma(sum);
    bool met = true;
    for (int z = 0; z < k; ++z) {
        const double pz = digamma(alpha[z]);
        g[z] = n * (psum - pz) + T[z];
        const bool held = alpha[z] <= PRIOR_FLOOR && g[z] <= 0.0;
        if (!held && !(std::fabs(g[z]) <= rule * (n * std::fabs(psum) + n * std::fabs(pz) + std::fabs(T[z])))) met = false;
    }
    return met;
}

// alpha [k] in: the start (every component finite and > 0), out: the maximiser of F under the contract above
inline PriorReport maximise_alpha(double *alpha, const double *T, int k, double n) {
    PriorReport report;
    if (k <= 1 || !(n > 0.0)) { report.converged = true; return report; }
    std::vector<double> cur(alpha, alpha + k), g(k), step(k), cand(k);
    for (int z = 0; z < k; ++z) cur[z] = std::fmax(cur[z], PRIOR_FLOOR);
    double scale = 0.0;
    const double f_start = alpha_objective(alpha, T, k, n);
    double f = alpha_objective(cur.data(), T, k, n, &scale);
    for (; report.rounds < PRIOR_ROUNDS; ++report.rounds) {
        if (alpha_gradient(cur.data(), T, k, n, g.data())) { report.converged = true; break; }
        double sum = 0.0;
        for (int z = 0; z < k; ++z) sum += cur[z];
        const double c = n * trigamma(sum);
        double gh = 0.0, ih = 0.0;
        for (int z = 0; z < k; ++z) {
            const bool held = cur[z] <= PRIOR_FLOOR && g[z] <= 0.0;
            step[z] = held ? 0.0 : -n * trigamma(cur[z]);        // h_z for now
            if (!held) { gh += g[z] / step[z]; ih += 1.0 / step[z]; }
        }
        const double b = gh / (1.0 / c + ih);
        for (int z = 0; z < k; ++z)
            if (step[z] != 0.0) step[z] = (g[z] - b) / step[z];
        double t = 1.0, f_cand = f;
        bool taken = false;
        for (int halving = 0; halving <= PRIOR_HALVINGS; ++halving, t *= 0.5) {
            for (int z = 0; z < k; ++z) cand[z] = std::fmax(cur[z] - t * step[z], PRIOR_FLOOR);
            double scale_cand = 0.0;
            f_cand = alpha_objective(cand.data(), T, k, n, &scale_cand);
            if (f_cand >= f - 0x1p-50 * std::fmax(scale, scale_cand)) { taken = true; scale = scale_cand; break; }
        }
        if (!taken) break;                                       // no step of this direction raises F: cur is what there is
        cur.swap(cand);
        f = f_cand;
    }
    if (!report.converged && report.rounds == PRIOR_ROUNDS) report.converged = alpha_gradient(cur.data(), T, k, n, g.data());
    if (f >= f_start) {
        for (int z = 0; z < k; ++z) {
            if (alpha[z] != cur[z]) report.moved = true;
            alpha[z] = cur[z];
        }
    }
    return report;
}

// F(eta) and the sum of the magnitudes it is formed from; k topics of m words
inline double eta_objective(double eta, double T, double k, double m, double *scale = nullptr) {
    const double top = std::lgamma(m * eta), each = std::lgamma(eta);
    if (scale) *scale = k * (std::fabs(top) + m * std::fabs(each)) + std::fabs(eta * T);
    return k * (top - m * each) + eta * T;
}

inline double eta_gradient(double eta, double T, double k, double m, bool *met, double rule = PRIOR_GRADIENT_RULE) {
    const double ptop = digamma(m * eta), peach = digamma(eta);
    const double g = k * m * (ptop - peach) + T;
    const bool held = eta <= PRIOR_FLOOR && g <= 0.0;
    *met = held || std::fabs(g) <= rule * (k * m * std::fabs(ptop) + k * m * std::fabs(peach) + std::fabs(T));
    return g;
}

// eta in: the start, out: the maximiser of F(eta) under the rules of maximise_alpha; m = 1 has T = 0 and returns its input
inline PriorReport maximise_eta(double *eta, double T, double k, double m) {
    PriorReport report;
    if (!(m > 1.0) || !(k > 0.0)) { report.converged = true; return report; }
    double cur = std::fmax(*eta, PRIOR_FLOOR), scale = 0.0;
    const double f_start = eta_objective(*eta, T, k, m);
    double f = eta_objective(cur, T, k, m, &scale);
    for (; report.rounds < PRIOR_ROUNDS; ++report.rounds) {
        bool met = false;
        const double g = eta_gradient(cur, T, k, m, &met);
        if (met) { report.converged = true; break; }
        const double h = k * m * (m * trigamma(m * cur) - trigamma(cur));
        const double step = g / h;
        double t = 1.0, cand = cur, f_cand = f;
        bool taken = false;
        for (int halving = 0; halving <= PRIOR_HALVINGS; ++halving, t *= 0.5) {
            cand = std::fmax(cur - t * step, PRIOR_FLOOR);
            double scale_cand = 0.0;
            f_cand = eta_objective(cand, T, k, m, &scale_cand);
            if (f_cand >= f - 0x1p-50 * std::fmax(scale, scale_cand)) { taken = true; scale = scale_cand; break; }
        }
        if (!taken) break;
        cur = cand;
        f = f_cand;
    }
    if (!report.converged && report.rounds == PRIOR_ROUNDS) (void)eta_gradient(cur, T, k, m, &report.converged);
    if (f >= f_start) {
        report.moved = *eta != cur;
        *eta = cur;
    }
    return report;
}

}  // namespace lda
}  // namespace plsa
