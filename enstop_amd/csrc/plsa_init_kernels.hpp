// plsa_init_kernels.hpp -- gfx950 device kernels of factor initialisation (plsa_init.hpp): the layout transposes between the
// reference's V [k, m] and the device's Vt [m, kp], the counter-based initialisation of throughput runs, and the reference's
// MT19937 stream on the device -- the generator, its jump-ahead, the sequential float64 topic marginals (the plain chain and
// the parity pairs) and the kernels that turn the words into factors.
#pragma once

#include "plsa_kernels.hpp"

namespace plsa {

// V [k,m] (reference layout) -> Vt [m,kp] (device layout), 32x32 tiles through LDS
__global__ void k_v_to_vt(const float *__restrict__ V, float *__restrict__ Vt, int k, int m, int kp) {
    __shared__ float tile[32][33];
    const int w0 = blockIdx.x * 32, z0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: ty = 0..7
    for (int r = ty; r < 32; r += 8) {
        const int z = z0 + r, w = w0 + tx;
        tile[r][tx] = (z < k && w < m) ? V[(i64)z * m + w] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int w = w0 + r, z = z0 + tx;
        if (w < m && z < kp) Vt[(i64)w * kp + z] = tile[tx][r];
    }
}

__global__ void k_vt_to_v(const float *__restrict__ Vt, float *__restrict__ V, int k, int m, int kp) {
    __shared__ float tile[32][33];
    const int w0 = blockIdx.x * 32, z0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int w = w0 + r, z = z0 + tx;
        tile[r][tx] = (w < m && z < kp) ? Vt[(i64)w * kp + z] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int z = z0 + r, w = w0 + tx;
        if (z < k && w < m) V[(i64)z * m + w] = tile[tx][r];
    }
}

// device-side factor initialisation for throughput runs (NOT the reference's MT19937 stream):
// counter-based uniform numbers, rows L1-normalised in place.  One group of 64 lanes per row.
__global__ void k_init_rows(float *__restrict__ A, i64 rows, int k, int kp, unsigned long long seed) {
    const int lane = threadIdx.x & 63;
    const i64 wid = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const i64 nw = ((i64)gridDim.x * blockDim.x) >> 6;
    for (i64 r = wid; r < rows; r += nw) {
        float part = 0.f;
        for (int z = lane; z < kp; z += 64) {
            float v = 0.f;
            if (z < k) {
                unsigned long long x = seed ^ ((unsigned long long)r * 0x9E3779B97F4A7C15ull + (unsigned long long)z);
                x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
                x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; x ^= x >> 31;
                v = ((float)(x >> 40) + 0.5f) * (1.0f / 16777216.0f);
            }
            A[r * kp + z] = v;
            part += v;
        }
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
        for (int z = lane; z < k; z += 64) A[r * kp + z] /= part;
    }
}

// ------------------------------------------------------------------------------------------------
// plsa_init(random) on the device with the REFERENCE'S random stream.  NumPy's legacy
// RandomState.rand() is MT19937: every double consumes two tempered 32-bit outputs,
// (a >> 5) * 2^26 + (b >> 6)) / 2^53.  k_mt19937_fill continues a given generator state (624 words
// + position) with one workgroup -- the recurrence is sequential across 624-word blocks but each
// block update is three data-parallel sweeps -- and leaves the advanced state behind so that the host
// generator can be set to exactly where the reference would be.  k_mt_init_v / k_mt_init_u turn the
// stream into the factors the way plsa.py:455-456, 510-511, 709-710 do: rand(k, m) first, then
// rand(n, k); float64 row sums accumulated left to right (enstop/utils.py:22-29), division, cast to
// float32 -- bit-identical to the host path.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned mt_temper(unsigned y) {
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
}
__device__ __forceinline__ unsigned mt_mix(unsigned hi, unsigned lo, unsigned far) {
    const unsigned y = (hi & 0x80000000u) | (lo & 0x7fffffffu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

#ifndef PLSA_MT_THREADS
#define PLSA_MT_THREADS 256  // measured: 256 threads 142 ms, 128 threads 187 ms for 140 M words (config 3), one stream
#endif
// one 624-word block of the recurrence: o = current block, nw = next block (distinct LDS arrays).
// Three data-parallel sweeps -- the recurrence reaches back 227 words -- with one synchronisation
// each; on return every thread may read nw.
template <int T>
__device__ __forceinline__ void mt_next_block(const unsigned *o, unsigned *nw, int t) {
#pragma unroll
    for (int i = t; i < 227; i += T) nw[i] = mt_mix(o[i], o[i + 1], o[i + 397]);            // old words only
    __syncthreads();
#pragma unroll
    for (int i = t; i < 227; i += T) nw[i + 227] = mt_mix(o[i + 227], o[i + 228], nw[i]);   // new [0, 227)
    __syncthreads();
#pragma unroll
    for (int i = t; i < 169; i += T) nw[i + 454] = mt_mix(o[i + 454], o[i + 455], nw[i + 227]);   // new [227, 396)
    if (t == T - 1) nw[623] = mt_mix(o[623], nw[0], nw[396]);
    __syncthreads();
}

// Continues the generator whose 624-word block is states[0] (position pos0 inside it) for n_words
// outputs.  Workgroup r starts from states[r] -- the block r * blocks_per_stream blocks further on,
// placed there by k_mt_jump -- and produces the blocks r * blocks_per_stream + 1 ... of the stream;
// with n_streams = 1 this is the plain sequential generator.  The last workgroup leaves the
// advanced state (624 words + position) in final_state.
__global__ __launch_bounds__(PLSA_MT_THREADS) void k_mt19937_fill(const unsigned *__restrict__ states, unsigned *__restrict__ out,
                                                                 int pos0, i64 blocks_per_stream, i64 n_words, int n_streams,
                                                                 unsigned *__restrict__ final_state /*[625]*/) {
    constexpr int T = PLSA_MT_THREADS;
    __shared__ unsigned buf[2][624];
    const int t = threadIdx.x, r = blockIdx.x;
    for (int i = t; i < 624; i += T) buf[0][i] = states[(i64)r * 624 + i];
    int cur = 0;
    __syncthreads();
    const i64 first = min((i64)(624 - pos0), n_words);          // the rest of the current block
    if (r == 0)
        for (i64 i = t; i < first; i += T) out[i] = mt_temper(buf[0][pos0 + i]);
    int pos = pos0 + (int)first;
    const i64 total_blocks = (n_words - first + 623) / 624;
    const i64 jb = (i64)r * blocks_per_stream + 1, je = min(jb + blocks_per_stream - 1, total_blocks);
    for (i64 j = jb; j <= je; ++j) {
        mt_next_block<T>(buf[cur], buf[cur ^ 1], t);
        cur ^= 1;
        const i64 at = first + (j - 1) * 624;
        const i64 take = min((i64)624, n_words - at);
        for (i64 i = t; i < take; i += T) out[at + i] = mt_temper(buf[cur][i]);
        pos = (int)take;
        // the next block is written into the copy read two sweeps ago: every thread passed the third
        // synchronisation after its last read of that copy
    }
    if (r == n_streams - 1) {
        __syncthreads();
        for (int i = t; i < 624; i += T) final_state[i] = buf[cur][i];
        if (t == 0) final_state[624] = (unsigned)pos;
    }
}

// Jump-ahead (csrc/mt_jump.hpp): word j of the block J words further on is XOR_{i : g_i = 1} x[i + j]
// over the raw word sequence x of the source block.  blockIdx.x picks the source stream
// q = 2 * step * blockIdx.x and fills stream q + step (zeroed beforehand); blockIdx.y takes one
// slice of the polynomial's 624 coefficient words, regenerates the stretch of x it needs in LDS and
// XORs its share into the destination.
constexpr int MT_JUMP_SLICES = 16;
constexpr int MT_JUMP_GW = 624 / MT_JUMP_SLICES;                 // coefficient words per slice
constexpr int MT_JUMP_WIN = MT_JUMP_GW * 32 + 624;               // words of x a slice touches
__global__ __launch_bounds__(256) void k_mt_jump(const unsigned *__restrict__ g /*[624]*/, unsigned *__restrict__ states,
                                                 int step, int n_streams) {
    const int q = (int)blockIdx.x * 2 * step, dst = q + step;
    if (dst >= n_streams) return;
    __shared__ unsigned buf[2][624];
    __shared__ unsigned win[MT_JUMP_WIN + 8];
    __shared__ unsigned gw[MT_JUMP_GW];
    const int t = threadIdx.x;
    const int i0 = (int)blockIdx.y * MT_JUMP_GW * 32, i1 = i0 + MT_JUMP_WIN;
    for (int i = t; i < 624; i += 256) buf[0][i] = states[(i64)q * 624 + i];
    if (t < MT_JUMP_GW) gw[t] = g[blockIdx.y * MT_JUMP_GW + t];
    __syncthreads();
    int cur = 0;
    for (int base = 0;; base += 624) {
        for (int i = t; i < 624; i += 256) {
            const int gi = base + i;
            if (gi >= i0 && gi < i1) win[gi - i0] = buf[cur][i];
        }
        if (base + 624 >= i1) break;
        mt_next_block<256>(buf[cur], buf[cur ^ 1], t);
        cur ^= 1;
    }
    __syncthreads();
    unsigned a0 = 0, a1 = 0, a2 = 0;
    const bool third = t + 512 < 624;
    for (int w = 0; w < MT_JUMP_GW; ++w) {
        unsigned bits = gw[w];
        while (bits) {
            const unsigned *x = win + w * 32 + __builtin_ctz(bits);
            bits &= bits - 1;
            a0 ^= x[t];
            a1 ^= x[t + 256];
            if (third) a2 ^= x[t + 512];
        }
    }
    unsigned *d = states + (i64)dst * 624;
    atomicXor(d + t, a0);
    atomicXor(d + t + 256, a1);
    if (third) atomicXor(d + t + 512, a2);
}

__device__ __forceinline__ double mt_double(const unsigned *w, i64 idx) {
    const unsigned a = w[2 * idx] >> 5, b = w[2 * idx + 1] >> 6;
    return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
}

// Sequential float64 marginal of each topic row, same rounding sequence as the reference's
// left-to-right sum (enstop/utils.py:24-29).  One wave per row: the 64 values of a chunk go through
// LDS so that every lane adds them in stream order (broadcast reads, one dependent add per value --
// the chain of m adds is the whole cost); chunks are prefetched four deep.  Padding adds +0.0,
// which leaves a non-negative sum unchanged.
__global__ __launch_bounds__(64) void k_mt_marginal_v(const unsigned *__restrict__ words, int k, int m,
                                                      double *__restrict__ marg) {
    constexpr int PF = 4;
    __shared__ double tile[2][64];
    const int z = blockIdx.x, lane = threadIdx.x;
    if (z >= k) return;
    const i64 base = (i64)z * m;
    double nxt[PF];
#pragma unroll
    for (int p = 0; p < PF; ++p) {
        const int w = p * 64 + lane;
        nxt[p] = w < m ? mt_double(words, base + w) : 0.0;
    }
    double s = 0.0;
    for (int w0 = 0; w0 < m; w0 += 64 * PF) {
        double cur[PF];
#pragma unroll
        for (int p = 0; p < PF; ++p) cur[p] = nxt[p];
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const i64 w = (i64)w0 + 64 * PF + p * 64 + lane;
            nxt[p] = w < m ? mt_double(words, base + w) : 0.0;
        }
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            if (w0 + p * 64 >= m) break;
            tile[p & 1][lane] = cur[p];
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 64; ++i) s += tile[p & 1][i];
        }
    }
    if (lane == 0) marg[z] = s;
}

// ------------------------------------------------------------------------------------------------
// The same marginal WITHOUT the chain of m dependent adds (k_mt_marginal_v above: 1.9 ms for the 173 762 words of the
// 20NG shape, three quarters of a member's initialisation) -- bit for bit the same sequence of roundings.
//
// The draws are X * 2^-53 with integers X < 2^53 (numpy's random_sample), so while the running sum s stays inside one
// binade [2^e, 2^(e+1)), e >= 0, it is an integer multiple T of u = 2^(e-52) and one rounded addition is
//     T' = T + q + c,   q = X >> (e+1),  r = X mod 2^(e+1),   c = [r > half] or ([r == half] and (T + q) odd)
// (round to nearest even): the increment depends on T only through its PARITY.  A chunk of 64 draws therefore maps the
// parity at its start to a total increment -- a pair (A0, A1) that every chunk computes on its own (k_mt_chunk_pairs),
// for the binade its approximate prefix sum points at.  One wave per topic then walks the chunks: s += A[parity] is an
// integer addition on the bit pattern, checked on the spot (exponent of s equals the chunk's binade before AND after: no
// crossing inside, all 64 roundings were at that granularity); a chunk that fails the check -- the ~18 binade crossings,
// the first chunk (s < 1: exact additions), a wrong guess -- is added one draw at a time exactly as above.  The checks
// make the result independent of how good the guess is; the guess only decides how many chunks take the slow way.
// Validated against the sequential sum draw for draw by the NumPy-identity tests and a tie-heavy host prototype.
// ------------------------------------------------------------------------------------------------
constexpr int MT_SEQ_L = 64;      // draws per chunk = chunks per workgroup tile
__device__ __forceinline__ u64 mt_int53(const unsigned *w, i64 idx) {
    return ((u64)(w[2 * idx] >> 5) << 26) | (u64)(w[2 * idx + 1] >> 6);
}

// tile[c][j] = draw j of chunk c0 + c of topic z (0 beyond the row): coalesced loads, conflict-free row reads
__device__ __forceinline__ void mt_load_tile(const unsigned *__restrict__ words, i64 base, int m, i64 c0,
                                             u64 (*tile)[MT_SEQ_L + 1]) {
    const int lane = threadIdx.x;
    for (int c = 0; c < MT_SEQ_L; ++c) {
        const i64 w = (c0 + c) * MT_SEQ_L + lane;
        tile[c][lane] = w < m ? mt_int53(words, base + w) : 0ull;
    }
    __syncthreads();
}

// exact integer sum of every chunk (< 2^59) and the approximate (float64) sum of every tile of 64 chunks:
// grid (ceil(nch / 64), k), 64 threads
__global__ __launch_bounds__(64) void k_mt_chunk_sums(const unsigned *__restrict__ words, int m, int nch,
                                                      u64 *__restrict__ csum, double *__restrict__ tsum) {
    __shared__ u64 tile[MT_SEQ_L][MT_SEQ_L + 1];
    const int z = blockIdx.y, lane = threadIdx.x;
    const i64 c0 = (i64)blockIdx.x * MT_SEQ_L;
    mt_load_tile(words, (i64)z * m, m, c0, tile);
    u64 t = 0;
#pragma unroll 8
    for (int j = 0; j < MT_SEQ_L; ++j) t += tile[lane][j];
    if (c0 + lane < nch) csum[(i64)z * nch + c0 + lane] = t;
    double tt = (c0 + lane < nch) ? (double)t : 0.0;
    for (int o = 32; o > 0; o >>= 1) tt += __shfl_xor(tt, o, 64);
    if (lane == 0) tsum[(i64)z * gridDim.x + blockIdx.x] = tt;
}

// per chunk: guessed binade e (from the approximate prefix sum of the chunk sums; -1: s < 1 or no guess) and the
// parity -> increment pair at that binade's granularity.  Same grid.
__global__ __launch_bounds__(64) void k_mt_chunk_pairs(const unsigned *__restrict__ words, int m, int nch,
                                                       const u64 *__restrict__ csum, const double *__restrict__ tsum,
                                                       u64 *__restrict__ pairs /*[2]*/, int *__restrict__ guess) {
    __shared__ u64 tile[MT_SEQ_L][MT_SEQ_L + 1];
    __shared__ double pre[MT_SEQ_L];
    const int z = blockIdx.y, lane = threadIdx.x;
    const i64 c0 = (i64)blockIdx.x * MT_SEQ_L;
    const u64 *cs = csum + (i64)z * nch;
    // approximate real prefix at this tile's first chunk -- the sums of the TILES in front of it (k_mt_chunk_sums; one
    // value per 4096 draws: linear in m per topic where summing the chunk sums was quadratic) -- then at each of its
    // chunks (any summation order will do: the walk checks every guess)
    double before = 0.0;
    const double *ts = tsum + (i64)z * gridDim.x;
    for (int t = lane; t < (int)blockIdx.x; t += 64) before += ts[t];
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
    pre[lane] = (c0 + lane < nch) ? (double)cs[c0 + lane] : 0.0;
    mt_load_tile(words, (i64)z * m, m, c0, tile);     // (synchronises)
    double start = before;
    for (int j = 0; j < lane; ++j) start += pre[j];
    start *= 0x1p-53;
    const int e = start >= 1.0 ? (int)((__double_as_longlong(start) >> 52) & 0x7ff) - 1023 : -1;
    u64 a0 = 0, a1 = 0;
    if (e >= 0 && e <= 51) {
        const int sh = e + 1;
        const u64 mask = (1ull << sh) - 1, half = 1ull << (sh - 1);
        u64 t0 = 0, t1 = 1;
#pragma unroll 4
        for (int j = 0; j < MT_SEQ_L; ++j) {
            const u64 x = tile[lane][j], q = x >> sh, r = x & mask;
            const u64 up = r > half, tie = r == half;
            t0 += q + (up | (tie & ((t0 + q) & 1)));
            t1 += q + (up | (tie & ((t1 + q) & 1)));
        }
        a0 = t0; a1 = t1 - 1;
    }
    if (c0 + lane < nch) {
        const i64 o = (i64)z * nch + c0 + lane;
        pairs[2 * o] = a0; pairs[2 * o + 1] = a1;
        guess[o] = (e >= 0 && e <= 51) ? e : -1;
    }
}

// one wave per topic walks its chunks; marg[z] = the reference's left-to-right float64 sum.  The walk is wave-uniform:
// lane l fetches the pair and the guess of chunk c0 + l (the next 64 are requested before the current 64 are walked --
// they do not depend on the sum), v_readlane moves chunk j's values to scalar registers and the dependent chain per chunk
// is a handful of SCALAR instructions (parity, select, 64-bit add, two range checks); only the draw-by-draw fallback
// touches the vector units.
__device__ __forceinline__ u64 readlane64(u64 v, int l) {
    return (u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffull), l) |
           ((u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l) << 32);
}
__global__ __launch_bounds__(64) void k_mt_marginal_walk(const unsigned *__restrict__ words, int m, int nch,
                                                         const u64 *__restrict__ pairs, const int *__restrict__ guess,
                                                         double *__restrict__ marg) {
    __shared__ double sx[MT_SEQ_L];
    const int z = blockIdx.x, lane = threadIdx.x;
    const i64 base = (i64)z * m;
    const u64 *pz = pairs + 2 * (i64)z * nch;
    const int *gz = guess + (i64)z * nch;
    u64 b = 0;      // bit pattern of the running sum (+0.0)
    u64 n0 = 0, n1 = 0;
    int ne = -1;
    if (lane < nch) { n0 = pz[2 * lane]; n1 = pz[2 * lane + 1]; ne = gz[lane]; }
    for (int c0 = 0; c0 < nch; c0 += 64) {
        const u64 v0 = n0, v1 = n1;
        const int ve = ne;
        const int cn = c0 + 64 + lane;
        if (cn < nch) { n0 = pz[2 * (i64)cn]; n1 = pz[2 * (i64)cn + 1]; ne = gz[cn]; }
        const int cnt = min(64, nch - c0);
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const int e = __builtin_amdgcn_readlane(ve, j);
            const u64 a0 = readlane64(v0, j), a1 = readlane64(v1, j);      // (independent of the sum: issued ahead)
            // binade e = bit patterns [lo, lo + 2^52) with lo = (e + 1023) << 52: compared on the high words.  The sum may
            // take the pair iff it starts and ends inside
            const unsigned lo_hi = (unsigned)(e + 1023) << 20;
            const u64 nb = b + ((b & 1) ? a1 : a0);
            if (e >= 0 && (unsigned)(b >> 32) >= lo_hi && (unsigned)(nb >> 32) < lo_hi + (1u << 20)) { b = nb; continue; }
            // one draw at a time (uniform branch: every lane walks the same sum)
            const i64 w = (i64)(c0 + j) * MT_SEQ_L + lane;
            __syncthreads();
            sx[lane] = w < m ? mt_double(words, base + w) : 0.0;
            __syncthreads();
            double sd = __longlong_as_double((long long)b);
#pragma unroll 8
            for (int i = 0; i < MT_SEQ_L; ++i) sd += sx[i];
            b = readlane64((u64)__double_as_longlong(sd), 0);      // (uniform; back to scalar registers)
        }
    }
    if (lane == 0) marg[z] = __longlong_as_double((long long)b);
}

// V[z, w] = float32(draw / marginal_z) in the reference layout, for the transpose kernel
__global__ __launch_bounds__(256) void k_mt_scale_v(const unsigned *__restrict__ words, const double *__restrict__ marg,
                                                    int k, int m, float *__restrict__ V) {
    const i64 total = (i64)k * m;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < total; i += (i64)gridDim.x * 256) {
        const double mg = marg[i / m];
        double v = mt_double(words, i);
        if (mg > 0.0) v /= mg;
        V[i] = (float)v;
    }
}

// 64 documents per wave: doubles [off + d*k, off + (d+1)*k) of the stream per document.  The draws
// are read coalesced (the 64 documents' values are one contiguous range) into an LDS tile of
// MT_U_COLS columns at a time, lane d adds document d's values in stream order, then the range is
// read again, divided and written as U[d, :] (pad columns zeroed) -- again coalesced.
constexpr int MT_U_COLS = 32;
__global__ __launch_bounds__(64) void k_mt_init_u(const unsigned *__restrict__ words, i64 off, i64 n, int k, int kp,
                                                  float *__restrict__ U) {
    __shared__ double tile[64][MT_U_COLS + 1];
    __shared__ double marg[64];
    const int lane = threadIdx.x;
    const i64 d0 = (i64)blockIdx.x * 64;
    const int docs = (int)min((i64)64, n - d0);
    double s = 0.0;
    for (int kc = 0; kc < k; kc += MT_U_COLS) {
        const int cols = min(MT_U_COLS, k - kc);
        const int cnt = docs * cols;
#pragma unroll 4
        for (int e = lane; e < cnt; e += 64) {
            const int r = e / cols, col = e - r * cols;
            tile[r][col] = mt_double(words, off + (d0 + r) * k + kc + col);
        }
        __syncthreads();
        if (lane < docs) {
#pragma unroll 8
            for (int i = 0; i < cols; ++i) s += tile[lane][i];
        }
        __syncthreads();
    }
    marg[lane] = s;
    __syncthreads();
    const int cnt = docs * kp;
#pragma unroll 4
    for (int e = lane; e < cnt; e += 64) {
        const int r = e / kp, z = e - r * kp;
        double v = 0.0;
        if (z < k) {
            v = mt_double(words, off + (d0 + r) * k + z);
            const double mg = marg[r];
            if (mg > 0.0) v /= mg;
        }
        U[d0 * kp + e] = (float)v;
    }
}

}  // namespace plsa
