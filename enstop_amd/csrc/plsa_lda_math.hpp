// plsa_lda_math.hpp -- the float64 special functions of variational Bayes LDA (plsa_lda_kernels.hpp):
// the digamma function, which HIP does not have, and the exp-digamma difference a table entry is.  Host and device, free of
// HIP when a host compiler reads it: tests/lda_math_host.cpp evaluates a grid that tests/test_lda_math_host.py compares with
// SciPy.
//
// digamma(x), x > 0: psi(x) = psi(x + 1) - 1 / x shifts x up to x >= 6, then
//     psi(x) ~ log x - 1 / (2 x) - sum_n B_2n / (2 n x^2n)
// with the twelve terms n = 1 .. 12 (Horner in 1 / x^2).  At x = 6 the first omitted term is 3.2e-16; the truncation is
// below one unit in the last place of psi(6) = 1.71 and falls off like x^-26.  The recurrence adds at most six reciprocals of
// the same sign, so the result is within a few 2^-53 max(1, |psi|) of the true value; next to the root at 1.4616 that is an
// absolute, not a relative, statement.  x <= 0 and NaN give NaN, +inf gives +inf.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define PLSA_LDA_HD __host__ __device__
#else
#define PLSA_LDA_HD
#endif

namespace plsa {
namespace lda {

PLSA_LDA_HD inline double digamma(double x) {
    if (!(x > 0.0)) return NAN;
    double shift = 0.0;
    while (x < 6.0) {                // at most six rounds
        shift += 1.0 / x;
        x += 1.0;
    }
    const double r = 1.0 / x, r2 = r * r;
    // B_2n / (2 n), n = 12 .. 1
    double s = -236364091.0 / 65520.0;
    s = s * r2 + 854513.0 / 3036.0;
    s = s * r2 - 174611.0 / 6600.0;
    s = s * r2 + 43867.0 / 14364.0;
    s = s * r2 - 3617.0 / 8160.0;
    s = s * r2 + 1.0 / 12.0;
    s = s * r2 - 691.0 / 32760.0;
    s = s * r2 + 1.0 / 132.0;
    s = s * r2 - 1.0 / 240.0;
    s = s * r2 + 1.0 / 252.0;
    s = s * r2 - 1.0 / 120.0;
    s = s * r2 + 1.0 / 12.0;
    return log(x) - 0.5 * r - s * r2 - shift;
}

// exp(psi(x) - psi_of_sum): the entry of an exp-digamma table whose row (or topic) sums to S, psi_of_sum = digamma(S) formed
// once per row.  x <= S, so the value lies in (0, 1]; it underflows to 0 where psi(x) - psi(S) < -745.
PLSA_LDA_HD inline double exp_digamma_diff(double x, double psi_of_sum) { return exp(digamma(x) - psi_of_sum); }

}  // namespace lda
}  // namespace plsa
#undef PLSA_LDA_HD
