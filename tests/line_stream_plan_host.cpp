// The line layout of the packed entry streams (enstop_amd/csrc/plsa_launch_plan.hpp: line_*) on a CPU.
// tests/test_line_stream_plan_host.py builds this with the sanitizers, feeds the cases and compares with a restatement.
//
// stdin, one call per line; stdout, one line of results per call:
//     sizes lpn seg                 -> words per block, words per item slot
//     blocks len lpn                -> blocks of an owner of len entries
//     pos rel lpn                   -> block lane component word, then rel and (block lane component) back from those
//     doc_bound nnz n lpn           -> upper bound of a document stream's words
//     item_words n_items seg lpn    -> words of an item stream
//     fits words                    -> 0 | 1
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../enstop_amd/csrc/plsa_launch_plan.hpp"

namespace plan = plsa::plan;

int main() {
    char name[32];
    long long a, b, c;
    while (std::scanf("%31s", name) == 1) {
        auto args = [&](int count) {
            long long *v[3] = {&a, &b, &c};
            for (int i = 0; i < count; ++i)
                if (std::scanf("%lld", v[i]) != 1) { std::fprintf(stderr, "bad case: %s\n", name); std::abort(); }
        };
        if (!std::strcmp(name, "sizes")) {
            args(2);
            std::printf("%d %d\n", plan::line_block((int)a), plan::line_slot((int)b, (int)a));
        } else if (!std::strcmp(name, "blocks")) {
            args(2);
            std::printf("%lld\n", (long long)plan::line_blocks(a, (int)b));
        } else if (!std::strcmp(name, "pos")) {
            args(2);
            const int lpn = (int)b;
            const plan::LinePos p = plan::line_pos(a, lpn);
            const long long word = plan::line_word(p, lpn);
            const plan::LinePos q = plan::line_pos_of_word(word, lpn);
            std::printf("%lld %d %d %lld %lld %lld %d %d\n", (long long)p.block, p.lane, p.comp, word,
                        (long long)plan::line_rel(p, lpn), (long long)q.block, q.lane, q.comp);
        } else if (!std::strcmp(name, "doc_bound")) {
            args(3);
            std::printf("%lld\n", (long long)plan::line_doc_words_bound(a, b, (int)c));
        } else if (!std::strcmp(name, "item_words")) {
            args(3);
            std::printf("%lld\n", (long long)plan::line_item_words(a, (int)b, (int)c));
        } else if (!std::strcmp(name, "fits")) {
            args(1);
            std::printf("%d\n", plan::line_stream_fits(a) ? 1 : 0);
        } else {
            std::fprintf(stderr, "unknown call: %s\n", name);
            return 2;
        }
    }
    return 0;
}
