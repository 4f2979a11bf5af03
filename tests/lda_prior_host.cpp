// The host arithmetic and the launch arithmetic of LDA's learned priors (enstop_amd/csrc/plsa_lda_prior_math.hpp,
// plsa_lda_prior_plan.hpp) on a CPU: both headers are free of HIP.  Reads commands from standard input and prints, with 17
// significant digits:
//   trigamma count, then count x                   -> trigamma(x), one per line
//   alpha k n, then k starts, then k sums T        -> "rounds converged moved", then the k components of the result
//   eta k m start T                                -> "rounds converged moved result"
//   logmean rows kp                                -> "slabs cut_ok once_ok order_ok": k_lda_logmean's own loops for every thread of
//                                                     every slab (cut: the slabs are consecutive ranges that cover the rows; once:
//                                                     every entry of the table is read by exactly one thread; order: a strand's
//                                                     rows ascend)
//   due done prior_start prior_every               -> 0 / 1
// tests/test_lda_prior_host.py supplies the cases and compares.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../enstop_amd/csrc/plsa_lda_prior_math.hpp"
#include "../enstop_amd/csrc/plsa_lda_prior_plan.hpp"

namespace plan = plsa::plan;

static void logmean(int64_t rows, int kp) {
    const int slabs = plan::lda_logmean_grid(rows);
    bool cut_ok = true, once = true, order_ok = true;
    int64_t next = 0;
    std::vector<uint8_t> seen((size_t)(rows * kp), 0);
    for (int s = 0; s < slabs; ++s) {
        const int64_t r0 = plan::prior_rows_first(rows, (unsigned)slabs, (unsigned)s), r1 = plan::prior_rows_last(rows, (unsigned)slabs, (unsigned)s);
        if (r1 > r0) {
            if (r0 != next) cut_ok = false;
            next = r1;
        }
        for (int zb = 0; zb < kp; zb += plan::LDA_BLOCK) {
            const int span = plan::logmean_span(kp, zb), strands = plan::logmean_strands(span);
            if (span < 1 || span > plan::LDA_BLOCK || strands < 1 || strands * span > plan::LDA_BLOCK) order_ok = false;
            for (int t = 0; t < plan::LDA_BLOCK; ++t) {
                const int z = zb + t % span, strand = t / span;
                if (strand >= strands) continue;
                int64_t last = -1;
                for (int64_t r = r0 + strand; r < r1; r += strands) {
                    if (z >= kp || r >= rows || seen[(size_t)(r * kp + z)]++) once = false;
                    if (r <= last) order_ok = false;
                    last = r;
                }
            }
        }
    }
    if (next != rows) cut_ok = false;
    for (size_t i = 0; i < seen.size(); ++i) if (seen[i] != 1) once = false;
    std::printf("%d %d %d %d\n", slabs, cut_ok ? 1 : 0, once ? 1 : 0, order_ok ? 1 : 0);
}

int main() {
    char kind[16];
    while (std::scanf("%15s", kind) == 1) {
        if (!std::strcmp(kind, "trigamma")) {
            int count = 0;
            if (std::scanf("%d", &count) != 1) return 2;
            for (int i = 0; i < count; ++i) {
                double x = 0.0;
                if (std::scanf("%lf", &x) != 1) return 2;
                std::printf("%.17g\n", plsa::lda::trigamma(x));
            }
        } else if (!std::strcmp(kind, "alpha")) {
            int k = 0;
            double n = 0.0;
            if (std::scanf("%d %lf", &k, &n) != 2 || k < 1) return 2;
            std::vector<double> alpha((size_t)k), T((size_t)k);
            for (double &v : alpha) if (std::scanf("%lf", &v) != 1) return 2;
            for (double &v : T) if (std::scanf("%lf", &v) != 1) return 2;
            const plsa::lda::PriorReport r = plsa::lda::maximise_alpha(alpha.data(), T.data(), k, n);
            std::printf("%d %d %d\n", r.rounds, r.converged ? 1 : 0, r.moved ? 1 : 0);
            for (double v : alpha) std::printf("%.17g\n", v);
        } else if (!std::strcmp(kind, "eta")) {
            double k = 0.0, m = 0.0, eta = 0.0, T = 0.0;
            if (std::scanf("%lf %lf %lf %lf", &k, &m, &eta, &T) != 4) return 2;
            const plsa::lda::PriorReport r = plsa::lda::maximise_eta(&eta, T, k, m);
            std::printf("%d %d %d %.17g\n", r.rounds, r.converged ? 1 : 0, r.moved ? 1 : 0, eta);
        } else if (!std::strcmp(kind, "logmean")) {
            long long rows = 0;
            int kp = 0;
            if (std::scanf("%lld %d", &rows, &kp) != 2) return 2;
            logmean(rows, kp);
        } else if (!std::strcmp(kind, "due")) {
            int done = 0, start = 0, every = 0;
            if (std::scanf("%d %d %d", &done, &start, &every) != 3) return 2;
            std::printf("%d\n", plan::prior_due(done, start, every) ? 1 : 0);
        } else {
            return 2;
        }
    }
    return 0;
}
