// The launch arithmetic of the reference arithmetic, enstop_amd/csrc/plsa_ref_plan.hpp, on a CPU (tests/test_ref_plan_host.py
// builds this with the sanitizers, feeds the cases and compares with values that come from elsewhere).
//
// stdin, one call per line; stdout, one line of results per call:
//     lanes kp                                           -> NZ G                      (0 0: unsupported)
//     pair_chain span cap corpus kp two_levels chunk     -> L, span's n_chunks n_groups n_super n_pad, cap's four,
//                                                           bytes of csum pairs exps pairs2 exps2
//     tiles nnz nz kp                                    -> tiles lds_bytes
//     pairs_now chain_mode pairs_off nnz                 -> 0 | 1
//     walk_too_slow slow chunks                          -> 0 | 1
//     row_tiled n knob                                   -> 0 | 1
//     block_plan n nnz kp budget with_indptr [indptr[0..n]]
//                                                        -> 0 largest blocks doc[0..blocks] ent[0..blocks]
//                                                           | 1 (the budget holds no row) | 2 document length
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../enstop_amd/csrc/plsa_ref_plan.hpp"

namespace plan = plsa::ref::plan;

int main() {
    char name[32];
    long long a, b, c, d, e, f;
    while (std::scanf("%31s", name) == 1) {
        auto args = [&](int count) {
            long long *v[6] = {&a, &b, &c, &d, &e, &f};
            for (int i = 0; i < count; ++i)
                if (std::scanf("%lld", v[i]) != 1) { std::fprintf(stderr, "bad case: %s\n", name); std::abort(); }
        };
        if (!std::strcmp(name, "lanes")) {
            args(1);
            std::printf("%d %d\n", plan::topics_per_lane((int)a), plan::group_lanes((int)a));
        } else if (!std::strcmp(name, "pair_chain")) {
            args(6);
            const plan::PairChain p = plan::pair_chain(a, b, c, (int)d, e != 0, (int)f);
            std::printf("%d", p.L);
            for (const plan::ChainGeom &g : {p.span, p.cap})
                std::printf(" %lld %lld %lld %lld", (long long)g.n_chunks, (long long)g.n_groups, (long long)g.n_super, (long long)g.n_pad);
            std::printf(" %lld %lld %lld %lld %lld\n", (long long)p.csum_bytes, (long long)p.pairs_bytes, (long long)p.exps_bytes,
                        (long long)p.pairs2_bytes, (long long)p.exps2_bytes);
        } else if (!std::strcmp(name, "tiles")) {
            args(3);
            std::printf("%lld %lld\n", (long long)plan::e_step_tiles(a, (int)b), (long long)plan::tile_lds_bytes((int)c, (int)b));
        } else if (!std::strcmp(name, "pairs_now")) {
            args(3);
            std::printf("%d\n", plan::pairs_now((int)a, b != 0, c) ? 1 : 0);
        } else if (!std::strcmp(name, "walk_too_slow")) {
            args(2);
            std::printf("%d\n", plan::walk_too_slow((unsigned long long)a, (unsigned long long)b) ? 1 : 0);
        } else if (!std::strcmp(name, "row_tiled")) {
            args(2);
            std::printf("%d\n", plan::row_tiled(a, (int)b) ? 1 : 0);
        } else if (!std::strcmp(name, "block_plan")) {
            args(5);
            // exactly n + 1 places, from the heap: a step past them is the address sanitizer's to see; without them a null
            // pointer, which the plan of a single block must not touch
            std::unique_ptr<int[]> indptr;
            if (e) {
                indptr.reset(new int[a + 1]);
                for (long long i = 0; i <= a; ++i)
                    if (std::scanf("%d", &indptr[i]) != 1) { std::fprintf(stderr, "bad case: block_plan\n"); std::abort(); }
            }
            const plan::BlockPlan pl = plan::block_plan(indptr.get(), a, b, (int)c, d);
            if (pl.status == plan::BlockPlan::NO_ROW) std::printf("1\n");
            else if (pl.status == plan::BlockPlan::DOC_TOO_LONG) std::printf("2 %lld %lld\n", (long long)pl.bad_doc, (long long)pl.bad_len);
            else {
                std::printf("0 %lld %zu", (long long)pl.largest, pl.doc.size() - 1);
                for (long long v : pl.doc) std::printf(" %lld", v);
                for (long long v : pl.ent) std::printf(" %lld", v);
                std::printf("\n");
            }
        } else {
            std::fprintf(stderr, "unknown call: %s\n", name);
            return 2;
        }
    }
    return 0;
}
