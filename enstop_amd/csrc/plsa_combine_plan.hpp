// plsa_combine_plan.hpp -- the launch arithmetic of the topic combination (plsa_combine_kernels.hpp, plsa_metric_kernels.hpp,
// plsa_embed_kernels.hpp; host side plsa_combine.hpp), free of HIP like plsa_lda_plan.hpp: plain values in, plain values out.
// The kernels take their tile origin and slice bounds from here, the host takes its grids, carves and member lists from here,
// and tests/combine_plan_host.cpp walks the same functions on a CPU.
//
// Pair tiles.  The t x t matrices are cut into nt x nt tiles of HELL_TILE rows and columns.  Hellinger is symmetric: workgroup
// b owns the b-th tile of `for i, for j >= i` (tri_tile), nt (nt + 1) / 2 of them.  KL is not: workgroup b owns tile
// (b / nt, b % nt) (square_tile).
//
// Vocabulary slices.  gridDim.y cuts the m words into `slices` ranges of `words` words, a multiple of the staging step
// HELL_KSTEP, so that tiles * slices fills the chip: slice s is [slice_begin, slice_end).  (slices * tiles <= 4 CUs + tiles:
// with slices > 1 the [slices][t][t] partial buffer stays below 2e8 bytes.)
//
// Grid limits: x below 2^31, y and z at most GRID_YZ_MAX.  t <= 65536 keeps every grid here inside them; the clusters of the
// representatives are gridDim.y and are refused above GRID_YZ_MAX.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace plsa {
namespace plan {

constexpr int COMBINE_BLOCK = 256;     // threads of the dense kernels (16 x 16 threads, 4 x 4 outputs each in the gram kernels)
constexpr int HELL_TILE = 64;          // rows / columns of the output tile
constexpr int HELL_KSTEP = 32;         // words staged per step
constexpr int COMBINE_MAX_SLICES = 64;
constexpr int GRID_YZ_MAX = 65535;
constexpr int METRIC_MAX_WORDS = 32;   // bits of a mask
constexpr int METRIC_BLOCK = 256;
constexpr int METRIC_MAX_SETS = 4096;  // sets per pass (grid z)
constexpr int LAYOUT_EPOCH_BLOCK = 256;
constexpr size_t LAYOUT_LDS_BYTES = 64 * 1024;     // dynamic LDS a kernel gets without an opt-in attribute

#if defined(__HIPCC__)
#define PLSA_COMBINE_PLAN_HD __host__ __device__
#else
#define PLSA_COMBINE_PLAN_HD
#endif

// ---------------------------------------------------------------------------------------------------------------------
// pair tiles
struct PairTile { int i, j; };

PLSA_COMBINE_PLAN_HD inline int pair_nt(int64_t t) { return (int)((t + HELL_TILE - 1) / HELL_TILE); }
PLSA_COMBINE_PLAN_HD inline int64_t tri_tiles(int nt) { return (int64_t)nt * (nt + 1) / 2; }
PLSA_COMBINE_PLAN_HD inline int64_t square_tiles(int nt) { return (int64_t)nt * nt; }

// the b-th pair of `for i, for j >= i`.  Counted from the end the rows hold 1, 2, 3, ... tiles: r tiles lie behind b, `back`
// whole rows of them, back (back + 1) / 2 <= r -- a float32 root (8 r + 1 < 2^24 for nt <= 1024: exact) and an integer
// correction.  A function of blockIdx.x alone: uniform per workgroup, evaluated once before the kernel's loop.
PLSA_COMBINE_PLAN_HD inline PairTile tri_tile(unsigned b, int nt) {
    const int r = (int)(tri_tiles(nt) - 1 - (int64_t)b);
    int back = (int)((sqrtf((float)(8 * r + 1)) - 1.f) * 0.5f);
    while (back * (back + 1) / 2 > r) --back;
    while ((back + 1) * (back + 2) / 2 <= r) ++back;
    const int i = nt - 1 - back;
    const int row_start = (int)(tri_tiles(nt) - tri_tiles(back + 1));
    return PairTile{i, i + ((int)b - row_start)};
}
PLSA_COMBINE_PLAN_HD inline PairTile square_tile(unsigned b, int nt) { return PairTile{(int)(b / (unsigned)nt), (int)(b % (unsigned)nt)}; }

// ---------------------------------------------------------------------------------------------------------------------
// vocabulary slices
PLSA_COMBINE_PLAN_HD inline int64_t slice_begin(unsigned s, int64_t words) { return (int64_t)s * words; }
PLSA_COMBINE_PLAN_HD inline int64_t slice_end(unsigned s, int64_t words, int64_t m) {
    const int64_t w1 = slice_begin(s, words) + words;
    return w1 < m ? w1 : m;
}
#undef PLSA_COMBINE_PLAN_HD

struct Slicing {
    int wanted;       // slices that would fill the chip
    int64_t words;    // words per slice, a multiple of HELL_KSTEP
    int slices;       // slices launched (gridDim.y)
};
inline Slicing vocab_slicing(int64_t tiles, int64_t m, int cus) {
    Slicing s;
    s.wanted = (int)std::max<int64_t>(1, std::min<int64_t>(COMBINE_MAX_SLICES, (4 * (int64_t)cus + tiles - 1) / tiles));
    s.words = ((m + s.wanted - 1) / s.wanted + HELL_KSTEP - 1) / HELL_KSTEP * HELL_KSTEP;
    s.slices = (int)((m + s.words - 1) / s.words);
    return s;
}

// one thread per element (k_hell_finish, k_sum_slices: t * t elements) or per word (the representatives: gridDim.x)
inline unsigned elementwise_grid(int64_t count) { return (unsigned)((count + COMBINE_BLOCK - 1) / COMBINE_BLOCK); }

// ---------------------------------------------------------------------------------------------------------------------
// representatives: the members of each cluster in row order, first[c] .. first[c + 1] (labels < 0 are noise).  Returns the
// index of the first label >= n_clusters, or -1; nothing is written for such a label.
inline int64_t member_lists(const int32_t *labels, int64_t t, int n_clusters, std::vector<int> &first, std::vector<int> &members) {
    first.assign((size_t)n_clusters + 1, 0);
    members.clear();
    for (int64_t i = 0; i < t; ++i) {
        if (labels[i] >= n_clusters) return i;
        if (labels[i] >= 0) first[(size_t)labels[i] + 1]++;
    }
    for (int cl = 0; cl < n_clusters; ++cl) first[(size_t)cl + 1] += first[(size_t)cl];
    members.resize((size_t)first[(size_t)n_clusters]);
    std::vector<int> fill(first.begin(), first.end() - 1);
    for (int64_t i = 0; i < t; ++i)
        if (labels[i] >= 0) members[(size_t)fill[(size_t)labels[i]]++] = (int)i;
    return -1;
}

// ---------------------------------------------------------------------------------------------------------------------
// co-document counts.  Sets per pass: what the caller asks for, else a quarter of what is free (the masks already held count
// as free) over one 32-bit mask per document; at least 1, at most the sets there are and METRIC_MAX_SETS.
inline int64_t metric_sets_per_pass(uint64_t free_bytes, uint64_t held_bytes, int64_t n, int64_t sets, int max_sets_per_pass) {
    int64_t chunk = max_sets_per_pass;
    if (chunk == 0) chunk = (int64_t)((free_bytes + held_bytes) / 4 / (sizeof(unsigned) * (uint64_t)n));
    return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(chunk, sets), METRIC_MAX_SETS));
}
// several workgroups per posting list (a head word has about n postings), several per mask row
inline unsigned metric_mark_x(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, (n + 4095) / 4096)); }
inline unsigned metric_count_x(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(128, (n + 2047) / 2048)); }
// metric_small in bytes: [chunk][nw][nw] co-document counters, [chunk][nw] positive counters (both 64-bit), [chunk][nw] word ids
struct MetricCarve { size_t co, positive, words, total; };
inline MetricCarve metric_carve(int64_t chunk, int nw) {
    MetricCarve v;
    v.co = 0;
    v.positive = sizeof(uint64_t) * (size_t)(chunk * nw * nw);
    v.words = v.positive + sizeof(uint64_t) * (size_t)(chunk * nw);
    v.total = v.words + sizeof(int32_t) * (size_t)(chunk * nw);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// k-NN membership, tk = t * n_neighbors.  Offsets in elements of the integer buffer (idx [tk], the arrival counter) and of the
// float buffer (dist [tk], member [tk], rho [t], sigma [t], row sums [t]); every array starts on 8 bytes.
struct KnnCarve {
    size_t idx, done, int_total;
    size_t dist, member, rho, sigma, row_sum, float_total;
};
inline KnnCarve knn_carve(int64_t t, int n_neighbors) {
    const auto even = [](size_t x) { return (x + 1) & ~(size_t)1; };
    const size_t tk = even((size_t)t * (size_t)n_neighbors), tt = even((size_t)t);
    KnnCarve v;
    v.idx = 0; v.done = tk; v.int_total = tk + 1;
    v.dist = 0; v.member = tk; v.rho = 2 * tk; v.sigma = v.rho + tt; v.row_sum = v.sigma + tt; v.float_total = v.row_sum + (size_t)t;
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// layout: k_layout_lds keeps two position buffers [t][dim] float32 in LDS
inline bool layout_fits_lds(int64_t t, int dim) { return 2 * sizeof(float) * (size_t)t * (size_t)dim <= LAYOUT_LDS_BYTES; }
enum LayoutPath { LAYOUT_REFUSED = -1, LAYOUT_LDS = 1, LAYOUT_PER_EPOCH = 2 };
// path 0 (auto) follows `fits`, path 1 (LDS) is refused when the buffers do not fit, path 2 runs an epoch per launch
inline LayoutPath layout_path(int path, bool fits) {
    if (path == 1) return fits ? LAYOUT_LDS : LAYOUT_REFUSED;
    return path == 0 && fits ? LAYOUT_LDS : LAYOUT_PER_EPOCH;
}
inline unsigned layout_epoch_grid(int64_t t) { return (unsigned)((t + LAYOUT_EPOCH_BLOCK - 1) / LAYOUT_EPOCH_BLOCK); }
// the schedule in float32, as the kernels advance it: an edge is due every max(W) / w epochs, first in that epoch, and its
// first negative samples eps / rate epochs in
struct EdgeSchedule { float eps, negative; };
inline EdgeSchedule layout_edge_schedule(float wmax, float w, float rate) {
    const float eps = wmax / w;
    return EdgeSchedule{eps, eps / rate};
}

}  // namespace plan
}  // namespace plsa
