// The float64 special functions of variational Bayes LDA (enstop_amd/csrc/plsa_lda_math.hpp) on a CPU: the header is free of
// HIP for a host compiler.  Reads lines "x s" from standard input and prints, with 17 significant digits,
// "digamma(x) exp_digamma_diff(x, digamma(s))" for each.  tests/test_lda_math_host.py supplies the grid and compares.
#include <cstdio>

#include "../enstop_amd/csrc/plsa_lda_math.hpp"

int main() {
    double x = 0.0, s = 0.0;
    while (std::scanf("%lf %lf", &x, &s) == 2)
        std::printf("%.17g %.17g\n", plsa::lda::digamma(x), plsa::lda::exp_digamma_diff(x, plsa::lda::digamma(s)));
    return 0;
}
