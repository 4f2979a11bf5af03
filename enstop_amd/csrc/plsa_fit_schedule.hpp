// plsa_fit_schedule.hpp -- the likelihood-test loop of the fit drivers (enstop/plsa.py:583-640, 884-920), free of HIP: the
// likelihood tests of one fit (Tests) and the two forms of the loop over a backend that enqueues the work.  plsa_drivers.hpp
// holds the backends of plsa_fit / plsa_refit, plsa_members.hpp keeps a loop of its own (a live mask, G likelihoods per
// synchronise) over a Tests per member; tests/fit_schedule_host.cpp runs both loops on a CPU against a fake backend.
//
// A backend B is what a loop needs from a context; every call returns 0 or the error code the loop returns at once:
//     loglik(&ll)                      likelihood of the current factors by a launch of its own, waited for
//     iteration()                      (materialised loop) one EM iteration, buffers swapped in
//     begin(), join()                  (fused loop) what precedes the first pass / what follows the last one
//     enqueue(want_ll)                 one fused iteration from the current factors into the alternate buffers, no swap;
//                                      want_ll: its document pass carries the likelihood of the factors it reads
//     enqueue_pair()                   two iterations, none carrying a likelihood; back on the starting buffers
//     ll_send(), ll_wait(&ll)          the carried likelihood sets off for the host / the host waits for it alone
//     ll_now(&ll)                      both at once: the host waits for everything enqueued
//     advance()                        the alternate buffers become the current ones
//     mark(), restore()                remember / return to the current buffers: the factors a stop returns
#pragma once

#include <climits>
#include <cmath>

namespace plsa {
namespace fit {

#define PLSA_FIT_TRY(expr) do { if (const int rc_ = (expr)) return rc_; } while (0)

// the three stop rules: plsa.py:634-638; block_parallel_plsa.py:329-331 (no `change == 0` arm); plsa.py:913-918 (the test
// only acts on a positive log-likelihood)
enum Rule { FIT, FIT_NO_ZERO_ARM, REFIT };

// The likelihood tests of one fit: the value the next test compares with, how many likelihoods were evaluated, and the
// trace.  A likelihood beyond the trace's capacity is counted, not written.
struct Tests {
    float *ll_trace;
    double tolerance;
    Rule rule;
    int n_iter_per_test;
    int cap = INT_MAX;               // places in ll_trace
    float prev = 0.f;
    int count = 0;

    bool due_after(int i) const { return i % n_iter_per_test == 0; }       // plsa.py:630

    int reserve() { return count++; }
    void write(int slot, float v) { if (ll_trace && slot < cap) ll_trace[slot] = v; }

    // plsa.py:591: the likelihood of the initial factors (initial_at: into a slot reserved when it set off)
    void initial_at(int slot, double ll) { prev = (float)ll; write(slot, prev); }
    void initial(double ll) { initial_at(reserve(), ll); }

    // records, then the stop test: float32 arithmetic, float64 comparison with the tolerance
    bool test(double ll) {
        const float cur = (float)ll;
        write(reserve(), cur);
        if (rule == REFIT && !(cur > 0.0f)) return false;
        const float change = fabsf(cur - prev);
        if ((rule == FIT && change == 0.0f) || (double)(change / fabsf(cur)) < tolerance) return true;
        prev = cur;
        return false;
    }

    // the test of the last iteration: its verdict changes nothing, it is only recorded
    void trailing(double ll) { write(reserve(), (float)ll); }
};

// The reference's kernel sequence: a likelihood, then iteration by iteration, the test right after the iteration it follows.
template <class B>
int run_materialised(B &b, Tests &t, int n_iter, bool trace, int *iters) {
    double ll = 0.0;
    PLSA_FIT_TRY(b.loglik(&ll));
    t.initial(ll);
    for (int i = 0; i < n_iter; ++i) {
        PLSA_FIT_TRY(b.iteration());
        ++*iters;
        if (t.due_after(i)) {
            if (i == n_iter - 1 && !trace) break;                // outcome cannot matter any more
            PLSA_FIT_TRY(b.loglik(&ll));
            if (t.test(ll)) break;
        }
    }
    return 0;
}

// speculate: a third set of buffers -- the iteration after a tested one is enqueued before the host waits for the test's
// likelihood.  graph: two successive iterations free of a likelihood go through enqueue_pair().  Not both.
struct Form { bool speculate, graph; };

// The fused schedule.  The likelihood the reference evaluates after iteration i is the likelihood of the factors iteration
// i + 1 reads, so it rides on iteration i + 1's document pass (the initial one on pass 0); the verdict arrives one pass
// late and a "stop" discards that pass by not advancing: factors, count and trace are the reference's.  Speculating, the
// pass after it is enqueued as well before the host waits (it writes the third set, so the factors a stop returns are still
// untouched) and a "stop" discards both; nothing is decided on the initial likelihood, which is collected when the first
// test needs it.
template <class B>
int run_fused(B &b, Tests &t, int n_iter, bool trace, Form form, int *iters) {
    double ll = 0.0;
    bool first = n_iter > 0;         // the initial likelihood rides on pass 0
    if (!first) { PLSA_FIT_TRY(b.loglik(&ll)); t.initial(ll); }
    PLSA_FIT_TRY(b.begin());
    bool pending = false;            // a test is due on the current factors
    bool stopped = false;
    int first_slot = -1;             // >= 0: the initial likelihood is in flight, this is its place in the trace
    auto collect_first = [&]() -> int {
        if (first_slot < 0) return 0;
        PLSA_FIT_TRY(b.ll_wait(&ll));
        t.initial_at(first_slot, ll);
        first_slot = -1;
        return 0;
    };
    for (int i = 0; i < n_iter; ++i) {
        const bool want_ll = pending || first;
        int done = 1;                // iterations this turn of the loop completes
        if (form.graph && !want_ll && i + 1 < n_iter && !t.due_after(i)) {     // iterations i and i + 1, neither carries a test
            PLSA_FIT_TRY(b.enqueue_pair());
            done = 2;
        } else {
            PLSA_FIT_TRY(b.enqueue(want_ll));
            if (first) {
                if (form.speculate) { PLSA_FIT_TRY(b.ll_send()); first_slot = t.reserve(); }
                else { PLSA_FIT_TRY(b.ll_now(&ll)); t.initial(ll); }
                first = false;
            } else if (pending && form.speculate && i + 1 < n_iter) {
                PLSA_FIT_TRY(collect_first());
                PLSA_FIT_TRY(b.ll_send());                       // on its way to the host; not waited for yet
                b.mark();
                b.advance();                                     // iteration i + 1 reads iteration i's output ...
                if (const int rc = b.enqueue(false)) { b.restore(); return rc; }   // ... and writes the third set (no test rides on it)
                PLSA_FIT_TRY(b.ll_wait(&ll));
                if (t.test(ll)) { b.restore(); stopped = true; break; }            // discard both passes
                done = 2;                                        // (no test follows iteration i + 1)
            } else if (pending) {
                PLSA_FIT_TRY(collect_first());
                PLSA_FIT_TRY(b.ll_now(&ll));
                if (t.test(ll)) { stopped = true; break; }       // discard this pass
            }
            b.advance();
        }
        *iters += done;
        i += done - 1;
        pending = t.due_after(i);
    }
    PLSA_FIT_TRY(collect_first());
    PLSA_FIT_TRY(b.join());
    if (!stopped && pending && trace) {                          // test of the last iteration: result-neutral
        PLSA_FIT_TRY(b.loglik(&ll));
        t.trailing(ll);
    }
    return 0;
}

#undef PLSA_FIT_TRY

}  // namespace fit
}  // namespace plsa
