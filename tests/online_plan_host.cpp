// The launch arithmetic of k_online_blend (enstop_amd/csrc/plsa_online_plan.hpp) on a CPU; tests/test_online_plan_host.py builds
// this with the sanitizers and feeds the cases.
//
// stdin, one call per line; stdout, one line of results per call:
//     blend m kp -> grid n4 lanes counted walked strands_ok
// A table is [m, kp] float32: n4 = m * kp / 4 float4s.  grid: workgroups (= slabs).  lanes: active lanes of a workgroup.
// counted: sum over all lanes of all workgroups of the float4s each one's loop visits (closed form per lane).  walked: the
// kernel's loop, `for (i = first; i < end; i += stride)`, run literally for every thread of every workgroup over a bitmap of n4
// places taken from the heap -- 1 when every place was visited exactly once and none outside, 0 otherwise.  strands_ok: every
// active lane's float4 column and strand are the ones colsum_slab_body gives the four columns it covers (column z of a sweep
// of `span` columns and rpp = 256 / span strands belongs to thread (z - zb) + strand * span there), lanes of different
// sweeps never share a column, and every (column, strand) pair of every sweep has exactly one owner.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../enstop_amd/csrc/plsa_online_plan.hpp"

namespace plan = plsa::plan;

int main() {
    char name[32];
    long long m, kp;
    while (std::scanf("%31s %lld %lld", name, &m, &kp) == 3) {
        if (std::strcmp(name, "blend")) { std::fprintf(stderr, "unknown call: %s\n", name); return 2; }
        if (kp <= 0 || kp % 4 || kp > plan::BLEND_MAX_KP) { std::fprintf(stderr, "bad kp\n"); return 2; }
        const int grid = plan::blend_grid(m);
        const int kq = (int)kp / 4;
        const int64_t n4 = (int64_t)m * kq;
        const size_t words = (size_t)((n4 + 63) / 64);
        std::unique_ptr<uint64_t[]> seen(new uint64_t[words]());      // exactly the places of the table
        bool once = true, strands_ok = true;
        int64_t counted = 0;
        int lanes = 0;
        // who owns (column, strand): colsum_slab_body's thread for that pair, per sweep
        std::vector<int> owners((size_t)kp * 256, 0);
        for (unsigned t = 0; t < (unsigned)plan::BLEND_BLOCK; ++t) {
            const plan::BlendLane l = plan::blend_lane((int)kp, t);
            if (!l.active) continue;
            ++lanes;
            const int zb = l.sweep * 256;
            const int span = (int)kp - zb < 256 ? (int)kp - zb : 256;
            strands_ok = strands_ok && zb < kp && l.span == span && l.rpp == 256 / span && l.strand >= 0 && l.strand < l.rpp &&
                         4 * l.q >= zb && 4 * l.q + 3 < zb + span;
            if (!strands_ok) break;
            for (int c = 0; c < 4; ++c) ++owners[(size_t)(4 * l.q + c) * 256 + l.strand];
        }
        for (int z = 0; z < kp && strands_ok; ++z) {
            const int zb = z / 256 * 256, span = (int)kp - zb < 256 ? (int)kp - zb : 256, rpp = 256 / span;
            for (int r = 0; r < 256; ++r) strands_ok = strands_ok && owners[(size_t)z * 256 + r] == (r < rpp ? 1 : 0);
        }
        for (int b = 0; b < grid; ++b) {
            const int64_t first_row = plan::blend_rows_first(m, (unsigned)grid, (unsigned)b);
            const int64_t last_row = plan::blend_rows_last(m, (unsigned)grid, (unsigned)b);
            for (unsigned t = 0; t < (unsigned)plan::BLEND_BLOCK; ++t) {
                const plan::BlendLane l = plan::blend_lane((int)kp, t);
                if (!l.active) continue;
                const int64_t end = plan::blend_end(last_row, kq), stride = plan::blend_stride(kq, l);
                const int64_t first = plan::blend_first(first_row, kq, l);
                if (first < end) counted += (end - 1 - first) / stride + 1;
                for (int64_t i = first; i < end; i += stride) {
                    if (i < 0 || i >= n4) { once = false; break; }
                    uint64_t &w = seen[(size_t)(i >> 6)];
                    const uint64_t bit = 1ull << (i & 63);
                    once = once && !(w & bit);
                    w |= bit;
                }
            }
        }
        for (size_t w = 0; w < words && once; ++w) {
            const int64_t left = n4 - (int64_t)w * 64;
            once = seen[w] == (left >= 64 ? ~0ull : (1ull << left) - 1);
        }
        std::printf("%d %lld %d %lld %d %d\n", grid, (long long)n4, lanes, (long long)counted, once ? 1 : 0, strands_ok ? 1 : 0);
    }
    return 0;
}
