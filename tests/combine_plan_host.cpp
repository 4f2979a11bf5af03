// The launch arithmetic of the topic combination (enstop_amd/csrc/plsa_combine_plan.hpp) on a CPU: the header is free of HIP.
// Reads one case per line from standard input and prints one line of integers per case.
//   tri nt                       i j of tri_tile(b, nt) for every b in [0, tri_tiles(nt)), after the tile count
//   square nt                    the same for square_tile and square_tiles
//   slicing kind t m cus         kind 0: Hellinger (triangular walk), 1: KL (square walk).  Walks slice_begin / slice_end over the
//                                slices.  Prints nt tiles wanted words slices last_words cut_ok(0/1) finish_grid
//   sets free held n sets cap    metric_sets_per_pass, then metric_mark_x(n) and metric_count_x(n)
//   egrid count                  elementwise_grid(count), then GRID_YZ_MAX
//   mcarve chunk nw              co positive words total (bytes)
//   knn t k                      idx done int_total dist member rho sigma row_sum float_total (elements)
//   members n_clusters t l...    member_lists over the t labels.  Prints bad, len(first), first..., len(members), members...
//   layout t dim                 fits path(0) path(1) path(2) epoch_grid
//   sched wmax w rate            float32 bit patterns in, the bit patterns of eps and of the first negative sample out
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../enstop_amd/csrc/plsa_combine_plan.hpp"

namespace plan = plsa::plan;

static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, sizeof f); return f; }
static uint32_t to_bits(float f) { uint32_t u; std::memcpy(&u, &f, sizeof u); return u; }

int main() {
    std::string line, out;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        out.clear();
        if (kind == "tri" || kind == "square") {
            int nt = 0;
            in >> nt;
            const int64_t tiles = kind == "tri" ? plan::tri_tiles(nt) : plan::square_tiles(nt);
            out += std::to_string(tiles);
            for (int64_t b = 0; b < tiles; ++b) {
                const plan::PairTile p = kind == "tri" ? plan::tri_tile((unsigned)b, nt) : plan::square_tile((unsigned)b, nt);
                out += ' '; out += std::to_string(p.i); out += ' '; out += std::to_string(p.j);
            }
        } else if (kind == "slicing") {
            int which = 0, cus = 0;
            int64_t t = 0, m = 0;
            in >> which >> t >> m >> cus;
            const int nt = plan::pair_nt(t);
            const int64_t tiles = which == 0 ? plan::tri_tiles(nt) : plan::square_tiles(nt);
            const plan::Slicing s = plan::vocab_slicing(tiles, m, cus);
            bool cut_ok = true;
            int64_t at = 0, last = 0;
            for (int y = 0; y < s.slices; ++y) {          // gridDim.y
                const int64_t w0 = plan::slice_begin((unsigned)y, s.words), w1 = plan::slice_end((unsigned)y, s.words, m);
                if (w0 != at || w1 <= w0) cut_ok = false;
                if (y + 1 < s.slices && (w1 - w0) % plan::HELL_KSTEP != 0) cut_ok = false;
                at = w1;
                last = w1 - w0;
            }
            if (at != m) cut_ok = false;
            std::printf("%d %lld %d %lld %d %lld %d %u\n", nt, (long long)tiles, s.wanted, (long long)s.words, s.slices, (long long)last,
                        cut_ok ? 1 : 0, plan::elementwise_grid(t * t));
            continue;
        } else if (kind == "sets") {
            uint64_t free_b = 0, held = 0;
            int64_t n = 0, sets = 0;
            int cap = 0;
            in >> free_b >> held >> n >> sets >> cap;
            std::printf("%lld %u %u\n", (long long)plan::metric_sets_per_pass(free_b, held, n, sets, cap), plan::metric_mark_x(n),
                        plan::metric_count_x(n));
            continue;
        } else if (kind == "egrid") {
            int64_t count = 0;
            in >> count;
            std::printf("%u %d\n", plan::elementwise_grid(count), plan::GRID_YZ_MAX);
            continue;
        } else if (kind == "mcarve") {
            int64_t chunk = 0;
            int nw = 0;
            in >> chunk >> nw;
            const plan::MetricCarve v = plan::metric_carve(chunk, nw);
            std::printf("%zu %zu %zu %zu\n", v.co, v.positive, v.words, v.total);
            continue;
        } else if (kind == "knn") {
            int64_t t = 0;
            int k = 0;
            in >> t >> k;
            const plan::KnnCarve v = plan::knn_carve(t, k);
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", v.idx, v.done, v.int_total, v.dist, v.member, v.rho, v.sigma, v.row_sum,
                        v.float_total);
            continue;
        } else if (kind == "members") {
            int n_clusters = 0;
            int64_t t = 0;
            in >> n_clusters >> t;
            std::vector<int32_t> labels((size_t)t);
            for (int64_t i = 0; i < t; ++i) in >> labels[(size_t)i];
            std::vector<int> first, members;
            const int64_t bad = plan::member_lists(labels.data(), t, n_clusters, first, members);
            out += std::to_string(bad) + ' ' + std::to_string(first.size());
            for (int v : first) { out += ' '; out += std::to_string(v); }
            out += ' ' + std::to_string(members.size());
            for (int v : members) { out += ' '; out += std::to_string(v); }
        } else if (kind == "layout") {
            int64_t t = 0;
            int dim = 0;
            in >> t >> dim;
            const bool fits = plan::layout_fits_lds(t, dim);
            std::printf("%d %d %d %d %u\n", fits ? 1 : 0, (int)plan::layout_path(0, fits), (int)plan::layout_path(1, fits),
                        (int)plan::layout_path(2, fits), plan::layout_epoch_grid(t));
            continue;
        } else if (kind == "sched") {
            uint32_t wmax = 0, w = 0, rate = 0;
            in >> wmax >> w >> rate;
            const plan::EdgeSchedule s = plan::layout_edge_schedule(from_bits(wmax), from_bits(w), from_bits(rate));
            std::printf("%u %u\n", to_bits(s.eps), to_bits(s.negative));
            continue;
        } else {
            std::fprintf(stderr, "unknown case: %s\n", line.c_str());
            return 2;
        }
        std::puts(out.c_str());
    }
    return 0;
}
