// The likelihood-test loops of enstop_amd/csrc/plsa_fit_schedule.hpp on a CPU, against a backend that models what the real
// ones must guarantee (tests/test_fit_schedule_host.py builds this with the sanitizers, feeds the cases and compares).
//
// The factors are "which S_i": three buffer slots, an iteration writes slot[out] = slot[cur] + 1.  The likelihood a
// document pass carries is ride[S] of the factors it read, k_loglik's is trail[S].  There is ONE host word for a
// likelihood (the context's pinned double), so the backend aborts on a second likelihood in flight, on a send with nothing
// carried, on a pair while the third buffer set is in use, and on a likelihood still in flight at return.
//
// stdin, one case per line:   form rule n_iter n_iter_per_test tolerance trace cap fail_at n  ride[0..n)  trail[0..n)
//     form 0 plain | 1 speculating | 2 graph | 3 materialised;  cap < 0: no capacity, -2: no trace pointer either
//     fail_at: the enqueue() with this index fails with code 7 (-1: none);  floats as their bits in hex
// stdout, one line per case:  rc iters cur slot[cur] count  written  trace[0..written) as bits
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "../enstop_amd/csrc/plsa_fit_schedule.hpp"

namespace {

[[noreturn]] void die(const char *what) {
    std::fprintf(stderr, "fake backend: %s\n", what);
    std::abort();
}

struct Fake {
    std::vector<double> ride, trail;
    bool third_set = false, rot3 = false;
    int slot[3] = {0, -1, -1}, cur = 0, marked = 0;
    bool carried = false, in_flight = false;
    double carried_ll = 0.0, flight_ll = 0.0;
    int enqueues = 0, fail_at = -1;

    int out() const { return rot3 ? (cur + 1) % 3 : 1 - cur; }
    double at(const std::vector<double> &v, int s) const {
        if (s < 0 || s >= (int)v.size()) die("a likelihood of factors that do not exist");
        return v[(size_t)s];
    }
    void step() { slot[out()] = slot[cur] + 1; }

    int loglik(double *ll) {
        if (in_flight) die("k_loglik while a likelihood is in flight");
        *ll = at(trail, slot[cur]);
        return 0;
    }
    int iteration() { step(); cur = out(); return 0; }
    int begin() { rot3 = third_set; return 0; }
    int join() { return 0; }
    int enqueue(bool want_ll) {
        if (enqueues++ == fail_at) return 7;
        if (want_ll) { carried = true; carried_ll = at(ride, slot[cur]); }
        step();
        return 0;
    }
    int enqueue_pair() {
        if (rot3) die("a pair while the third set is in use");
        step();
        cur = out();
        step();
        cur = out();
        return 0;
    }
    int ll_send() {
        if (!carried) die("a send with nothing carried");
        if (in_flight) die("a second likelihood in flight");
        in_flight = true; flight_ll = carried_ll; carried = false;
        return 0;
    }
    int ll_wait(double *ll) {
        if (!in_flight) die("a wait with nothing in flight");
        *ll = flight_ll; in_flight = false;
        return 0;
    }
    int ll_now(double *ll) {
        if (!carried) die("a send with nothing carried");
        if (in_flight) die("a second likelihood in flight");
        *ll = carried_ll; carried = false;
        return 0;
    }
    void advance() { cur = out(); }
    void mark() { marked = cur; }
    void restore() { cur = marked; }
    void leave() {       // what the real backend's destructor does: cur back in {0, 1}
        if (in_flight) die("a likelihood still in flight at return");
        if (rot3 && cur == 2) { std::swap(slot[2], slot[0]); cur = 0; }
        rot3 = false;
    }
};

float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
uint32_t to_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

}  // namespace

int main() {
    int form, rule, n_iter, per, trace, cap, fail_at, n;
    char tol_text[64];
    while (std::scanf("%d %d %d %d %63s %d %d %d %d", &form, &rule, &n_iter, &per, tol_text, &trace, &cap, &fail_at, &n) == 9) {
        Fake b;
        b.third_set = form == 1;
        b.fail_at = fail_at;
        for (std::vector<double> *v : {&b.ride, &b.trail})
            for (int i = 0; i < n; ++i) {
                unsigned u;
                if (std::scanf("%x", &u) != 1) die("bad case");
                v->push_back((double)from_bits(u));
            }
        // exactly the capacity, from the heap: a write past it is the address sanitizer's to see
        const int room = cap >= 0 ? cap : n_iter + 2;
        std::unique_ptr<float[]> ll_trace(cap == -2 ? nullptr : new float[(size_t)room]());
        const double tolerance = std::strtod(tol_text, nullptr);
        plsa::fit::Tests tests{ll_trace.get(), tolerance, (plsa::fit::Rule)rule, per};
        if (cap >= 0) tests.cap = cap;
        int iters = 0;
        const int rc = form == 3 ? plsa::fit::run_materialised(b, tests, n_iter, trace != 0, &iters)
                                 : plsa::fit::run_fused(b, tests, n_iter, trace != 0, plsa::fit::Form{form == 1, form == 2}, &iters);
        if (!rc) b.leave();
        else if (b.rot3 && b.cur == 2) { std::swap(b.slot[2], b.slot[0]); b.cur = 0; }
        const int written = !ll_trace ? 0 : (tests.count < room ? tests.count : room);
        std::printf("%d %d %d %d %d %d", rc, iters, b.cur, b.slot[b.cur], tests.count, written);
        for (int i = 0; i < written; ++i) std::printf(" %08x", to_bits(ll_trace[(size_t)i]));
        std::printf("\n");
    }
    return 0;
}
