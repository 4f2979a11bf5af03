// The arithmetic of factor initialisation with the MT19937 stream, enstop_amd/csrc/plsa_init_plan.hpp, on a CPU
// (tests/test_init_plan_host.py builds this with the sanitizers, feeds the cases and compares with values that come from
// elsewhere).
//
// stdin, one call per line; stdout, one line of results per call:
//     stream n m k draw_topics pos0 mt_streams mt_min_blocks
//                                     -> ok v_doubles n_doubles n_words first total_blocks per_stream log2_per n_streams
//                                        streams_p2 levels words_bytes, then per level: exponent step sources (k_mt_jump's grid x)
//                                        | 0 (bad position)
//     scratch k m streams_p2 levels chain
//                                     -> state_bytes fin_bytes poly_bytes marg_word nch tiles csum_off pairs_off tsum_off guess_off
//                                        seq_bytes, the chunk kernels' grid x y
//     grids n m kp                    -> the transposes' grid x y, k_mt_init_u's grid
//     jump_tree n m k draw_topics pos0 mt_streams mt_min_blocks key[0..623]
//                                     -> n_streams per_stream, then the 624 key words of every stream: stream 0 is the key
//                                        given, the others are made level by level with the planned jumps (csrc/mt_jump.hpp),
//                                        the way k_mt_jump fills them: source q = 2 step i, destination q + step if there is one
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../enstop_amd/csrc/mt_jump.hpp"
#include "../enstop_amd/csrc/plsa_init_plan.hpp"

namespace plan = plsa::init::plan;

int main() {
    char name[32];
    long long v[7];
    while (std::scanf("%31s", name) == 1) {
        auto args = [&](int count) {
            for (int i = 0; i < count; ++i)
                if (std::scanf("%lld", &v[i]) != 1) { std::fprintf(stderr, "bad case: %s\n", name); std::abort(); }
        };
        if (!std::strcmp(name, "stream")) {
            args(7);
            const plan::MtStream s = plan::mt_stream(v[0], v[1], (int)v[2], v[3] != 0, v[4], (int)v[5], v[6]);
            if (!s.ok) { std::printf("0\n"); continue; }
            std::printf("1 %lld %lld %lld %lld %lld %lld %d %d %d %d %lld", (long long)s.v_doubles, (long long)s.n_doubles,
                        (long long)s.n_words, (long long)s.first, (long long)s.total_blocks, (long long)s.per_stream, s.log2_per,
                        s.n_streams, s.streams_p2, s.levels, (long long)s.words_bytes());
            for (int l = 0; l < s.levels; ++l) std::printf(" %d %d %u", s.exponent(l), s.step(l), plan::jump_grid(s, l));
            std::printf("\n");
        } else if (!std::strcmp(name, "scratch")) {
            args(5);
            const plan::MtScratch s = plan::mt_scratch((int)v[0], v[1], (int)v[2], (int)v[3], v[4] != 0);
            const plan::Grid2 g = plan::chunk_grid(s, (int)v[0]);
            std::printf("%lld %lld %lld %d %d %d %lld %lld %lld %lld %lld %u %u\n", (long long)s.state_bytes, (long long)s.fin_bytes,
                        (long long)s.poly_bytes, s.marg_word, s.nch, s.tiles, (long long)s.csum_off, (long long)s.pairs_off,
                        (long long)s.tsum_off, (long long)s.guess_off, (long long)s.seq_bytes, g.x, g.y);
        } else if (!std::strcmp(name, "grids")) {
            args(3);
            const plan::Grid2 g = plan::transpose_grid(v[1], (int)v[2]);
            std::printf("%u %u %u\n", g.x, g.y, plan::init_u_grid(v[0]));
        } else if (!std::strcmp(name, "jump_tree")) {
            args(7);
            const plan::MtStream s = plan::mt_stream(v[0], v[1], (int)v[2], v[3] != 0, v[4], (int)v[5], v[6]);
            if (!s.ok) { std::fprintf(stderr, "bad case: jump_tree\n"); std::abort(); }
            // exactly streams_p2 blocks, from the heap, zeroed as mt_init zeroes them: a step past them is the address sanitizer's
            std::vector<uint32_t> st((size_t)s.streams_p2 * 624, 0u);
            for (int i = 0; i < 624; ++i)
                if (std::scanf("%u", &st[i]) != 1) { std::fprintf(stderr, "bad case: jump_tree\n"); std::abort(); }
            for (int l = 0; l < s.levels; ++l) {
                uint32_t g[624];
                if (!mtjump::block_jump_polynomial(s.exponent(l), g)) { std::fprintf(stderr, "no polynomial\n"); std::abort(); }
                const int step = s.step(l);
                for (unsigned i = 0; i < plan::jump_grid(s, l); ++i) {
                    const int q = (int)i * 2 * step, dst = q + step;
                    if (dst >= s.n_streams) continue;
                    std::memcpy(&st[(size_t)dst * 624], &st[(size_t)q * 624], sizeof(uint32_t) * 624);
                    mtjump::apply_jump(&st[(size_t)dst * 624], g);
                }
            }
            std::printf("%d %lld", s.n_streams, (long long)s.per_stream);
            for (size_t i = 0; i < (size_t)s.n_streams * 624; ++i) std::printf(" %u", st[i]);
            std::printf("\n");
        } else {
            std::fprintf(stderr, "unknown call: %s\n", name);
            return 2;
        }
    }
    return 0;
}
