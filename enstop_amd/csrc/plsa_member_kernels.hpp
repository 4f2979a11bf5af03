// plsa_member_kernels.hpp -- the fused EM iteration of a BATCH of ensemble members: every kernel of the iteration
// launched once for all members (include/plsa_hip_members.h, plsa_hip.hip: plsa_members_fit).
//
// A member is a bootstrap resample with its own structures (CSC items, packed streams, row items, factors), built by the
// builders a standalone fit uses.  Each kernel here is the BODY of its standalone counterpart (plsa_kernels.hpp:
// row_pass_body, col_pass_body, ...) behind a per-member argument table: blockIdx.y selects the member, blockIdx.x is the
// member's workgroup, and every body gets the member's OWN standalone grid as the partition of its work -- the launch's
// x-extent is the maximum over the members, and workgroups beyond a member's grid exit at once.  That is what keeps a
// member bit-identical to its standalone fit: the fused log-likelihood leaves one double per workgroup of that grid and
// ll_final_body adds exactly those; norm_reduce_body cuts the chunk rows by that grid.
//
// `live`: bit r set while member r (position in the table, at most 64) is still iterating; a stopped member's workgroups
// exit before they read the table.  `cu` / `cv`: which of the member's two P(z|d) / P(w|z) buffers holds its current
// factors (a stopped member's parity freezes, so the table holds both buffers and the parity travels by value).
#pragma once

#include "plsa_kernels.hpp"

namespace plsa {

constexpr int MEMBERS_MAX = 64;    // members per launch: the live set is one 64-bit kernel argument

struct MemberArgs {
    // column pass
    const int4 *item_rec;
    const int *csc_row;            // the packed CSC stream in a packed group
    const float *csc_val;
    int slot;                      // words per item slot of the packed CSC stream
    float *partial;
    double *chunk_sums;
    i64 n_items;
    // column tail
    double *chunk_sums2;           // stage-2 rows of the norm (members with more than 2048 chunk rows)
    float *norm_pwz;
    const int *item_first, *heavy_cols;
    int n_chunks, norm_blocks;     // norm_blocks: grid of the member's k_norm_reduce (0: one stage)
    int m, n_heavy, heavy_items, reduce_grid;
    // document pass
    const int *indptr, *colidx;    // colidx: the packed CSR stream in a packed group
    const float *vals;
    const int *sblk;               // block offsets of the documents in the packed CSR stream
    const int *row_order, *ritem_row, *ritem_start, *ritem_first;   // ritem_*: nullptr for a member on whole rows
    float *rpartial;
    double *ll_partials, *ll_out;
    i64 n_ritems;
    int n, rseg, row_grid, row_reduce_grid;
    // factors, both parities
    float *U[2], *Vt[2];
};

__device__ __forceinline__ bool member_live(u64 live, unsigned r) { return (live >> r) & 1ull; }

template <class S, bool WANT_LL, bool TINY>
__global__ __launch_bounds__(256, PLSA_WAVES) void k_row_pass_members(const MemberArgs *__restrict__ args, u64 live, u64 cu,
                                                                      u64 cv, int kp_rt, float thresh) {
    const unsigned r = blockIdx.y;
    if (!member_live(live, r)) return;
    const MemberArgs &a = args[r];
    if (blockIdx.x >= (unsigned)a.row_grid) return;
    const int pu = (int)((cu >> r) & 1ull), pv = (int)((cv >> r) & 1ull);
    row_pass_body<S, false, WANT_LL, TINY>(a.indptr, a.colidx, a.vals, a.sblk, a.n, a.row_order, a.U[pu], a.Vt[pv], nullptr, a.U[1 - pu],
                                           nullptr, nullptr, kp_rt, thresh, a.ll_partials, a.ritem_row, a.ritem_start, a.rseg,
                                           a.n_ritems, a.rpartial, 0, blockIdx.x, (unsigned)a.row_grid);
}

template <class S>
__global__ __launch_bounds__(256) void k_row_reduce_members(const MemberArgs *__restrict__ args, u64 live, u64 cu, int kp_rt) {
    const unsigned r = blockIdx.y;
    if (!member_live(live, r)) return;
    const MemberArgs &a = args[r];
    if (!a.ritem_row || blockIdx.x >= (unsigned)a.row_reduce_grid) return;
    const int pu = (int)((cu >> r) & 1ull);
    row_reduce_body<S>(a.ritem_first, a.n, a.rpartial, a.U[1 - pu], nullptr, kp_rt, blockIdx.x, (unsigned)a.row_reduce_grid);
}

// one workgroup per member: the fixed-order sum of the member's own row_grid partials
__global__ __launch_bounds__(256) void k_ll_final_members(const MemberArgs *__restrict__ args, u64 live) {
    __shared__ double red[256];
    const unsigned r = blockIdx.x;
    if (!member_live(live, r)) return;
    const MemberArgs &a = args[r];
    ll_final_body(a.ll_partials, a.row_grid, a.ll_out, red);
}

// One chunk of items per trip, grid-stride over the member's chunks: partials are per item and the norm rows per chunk,
// so the results do not depend on which workgroup visits a chunk (plsa_kernels.hpp: k_col_pass); equal stretches, no
// XCD split.
template <class S, bool TINY>
__global__ __launch_bounds__(256, PLSA_WAVES_COL) void k_col_pass_members(const MemberArgs *__restrict__ args, u64 live, u64 cu,
                                                                          u64 cv, int kp_rt, float thresh) {
    extern __shared__ double scol[];   // [GPB][kp]
    const unsigned r = blockIdx.y;
    if (!member_live(live, r)) return;
    const MemberArgs &a = args[r];
    if (blockIdx.x >= (unsigned)a.n_chunks) return;
    const int pu = (int)((cu >> r) & 1ull), pv = (int)((cv >> r) & 1ull);
    const unsigned nblocks = min((unsigned)a.n_chunks, gridDim.x);
    col_pass_body<S, false, false, TINY>(a.item_rec, a.n_items, nullptr, a.csc_row, a.csc_val, a.slot, nullptr, a.U[pu], a.Vt[pv], nullptr,
                                         nullptr, a.partial, kp_rt, thresh, 0, a.chunk_sums, nullptr, scol, blockIdx.x, nblocks);
}

__global__ __launch_bounds__(256) void k_norm_reduce_members(const MemberArgs *__restrict__ args, u64 live, int kp) {
    __shared__ double sred[256];
    const unsigned r = blockIdx.y;
    if (!member_live(live, r)) return;
    const MemberArgs &a = args[r];
    if (blockIdx.x >= (unsigned)a.norm_blocks) return;
    norm_reduce_body(a.chunk_sums, a.n_chunks, kp, a.chunk_sums2, sred, blockIdx.x, (unsigned)a.norm_blocks);
}

__global__ __launch_bounds__(256) void k_colsum_final_members(const MemberArgs *__restrict__ args, u64 live, int kp) {
    __shared__ double sred[256];
    const unsigned r = blockIdx.x;
    if (!member_live(live, r)) return;
    const MemberArgs &a = args[r];
    if (a.norm_blocks > 0) colsum_final_body(a.chunk_sums2, a.norm_blocks, kp, a.norm_pwz, sred);
    else colsum_final_body(a.chunk_sums, a.n_chunks, kp, a.norm_pwz, sred);
}

template <class S>
__global__ __launch_bounds__(256) void k_col_reduce_norm_members(const MemberArgs *__restrict__ args, u64 live, u64 cv,
                                                                 int kp_rt) {
    extern __shared__ float sdyn[];  // [GPB][kp] heavy-column sums, then [kp] norm_pwz
    const unsigned r = blockIdx.y;
    if (!member_live(live, r)) return;
    const MemberArgs &a = args[r];
    if (blockIdx.x >= (unsigned)a.reduce_grid) return;
    const int kp = S::kp(kp_rt);
    constexpr int GPB = 256 / S::LPN;
    float *snorm = sdyn + GPB * kp;
    for (int z = threadIdx.x; z < kp; z += 256) snorm[z] = a.norm_pwz[z];
    __syncthreads();
    const int pv = (int)((cv >> r) & 1ull);
    col_reduce_body<S, true>(a.item_first, a.m, a.heavy_items, a.heavy_cols, a.n_heavy, a.partial, a.Vt[1 - pv], kp,
                             (int)blockIdx.x, a.reduce_grid, sdyn, snorm);
}

}  // namespace plsa
