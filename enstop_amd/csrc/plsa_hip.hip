// plsa_hip.hip -- host side of libplsa_hip.so: context, HBM layout, kernel dispatch, EM drivers and
// the C ABI declared in include/plsa_hip.h (the drop-in) and include/plsa_hip_diag.h (diagnostics, measurement, test plumbing).
// The features built on them are host headers included at the end of this file, each after its kernel header: from the fit
// drivers (csrc/plsa_drivers.hpp) to the topic combination (csrc/plsa_combine.hpp).  gfx950 only; no other back-end exists.
//
// HBM layout per context (n docs, m words, k topics, kp = 4*ceil(k/4)):
//   base CSR     indptr i32[n+1], col i32[nnz], val f32[nnz]      the uploaded corpus
//   active CSR   same arrays for the matrix the EM runs on (== base, or a bootstrap resample)
//   rowidx       i32[nnz]   COO row ids of the active matrix (nnz-parallel E-step)
//   CSC copy     colptr i32[m+1], csc_row/csc_pos i32[nnz], csc_val f32[nnz], column items
//                (built lazily; not needed with PLSA_ATOMIC_V)
//   U[2(+1)]     f32[n,kp]  P(z|d), double-buffered (a rejected iteration is simply not swapped in); a third buffer while a
//                fit of a small corpus runs one iteration ahead of its likelihood tests (plsa_fit)
//   Vt[2(+1)], Vacc  f32[m,kp]  P(w|z) word-major, buffered like U, + the un-normalised accumulator
//   P            f32[nnz,kp] materialised responsibilities (only when not PLSA_FUSED)
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/plsa_hip.h"
#include "../../include/plsa_hip_diag.h"
#include "../../include/plsa_hip_members.h"
#include "../../include/plsa_hip_blocked.h"
#include "../../include/plsa_hip_nmf.h"
#include "../../include/plsa_hip_score.h"
#include "../../include/plsa_hip_tempered.h"
#include "../../include/plsa_hip_online.h"
#include "../include/plsa_hip_lda_priors.h"
#include "../include/plsa_hip_lda_online.h"
#include "mt_jump.hpp"
#include "plsa_init_kernels.hpp"
#include "plsa_init_plan.hpp"
#include "plsa_kernels.hpp"
#include "plsa_launch_plan.hpp"
#include "plsa_member_kernels.hpp"
#include "plsa_nmf_kernels.hpp"
#include "plsa_ref_kernels.hpp"
#include "plsa_synth.hpp"

using plsa::i64;

namespace {

thread_local std::string g_err;  // errors before a context exists

// Ensemble members of a small corpus are fitted concurrently on several contexts of ONE device (two streams each).  The
// HIP runtime multiplexes all streams of a process onto GPU_MAX_HW_QUEUES = 4 hardware queues by default, and streams that
// share a queue run in submission order: a member's initialisation chain then stalls another member's EM kernels (20NG
// shape, four contexts: 7 060 -> 7 770 ... 8 500 fits/min through ensemble_of_topics; single fits unchanged).  Rounds 3-4
// set GPU_MAX_HW_QUEUES=8 from a constructor of this library; a drop-in must not edit its host's environment behind its
// back, so since round 5 the LIBRARY never does: enstop_amd/_lib.py (the Python host layer) sets it before loading the
// library unless ENSTOP_AMD_HW_QUEUES=0, and a C host that wants concurrent members calls
// setenv("GPU_MAX_HW_QUEUES", "8", 0) itself before its first HIP call.  plsa_hw_queues() reports what
// this process runs with.

// Device memory, freed with its holder.  A BORROWED buffer (plsa_p_borrow) only views memory lent by someone else: it is
// never freed here, and release() leaves it in place (borrow(nullptr) ends the loan).
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    bool borrowed = false;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept { swap(o); }
    DevBuf &operator=(DevBuf &&o) noexcept { DevBuf(std::move(o)).swap(*this); return *this; }   // (the old memory goes with the temporary)
    void swap(DevBuf &o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); std::swap(borrowed, o.borrowed); }
    ~DevBuf() { if (p && !borrowed) (void)hipFree(p); }
    void release() { if (!borrowed) *this = DevBuf(); }
    void borrow(void *q, size_t bytes) { *this = DevBuf(); p = q; cap = q ? bytes : 0; borrowed = q != nullptr; }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// owning HIP stream / event handle; converts to the raw handle wherever one is passed
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle &&o) noexcept { std::swap(h, o.h); }
    Handle &operator=(Handle &&o) noexcept { Handle(std::move(o)).swap(*this); return *this; }
    void swap(Handle &o) noexcept { std::swap(h, o.h); }
    ~Handle() { if (h) (void)Destroy(h); }
    operator H() const { return h; }
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;

// page-locked host memory
struct HostFree { void operator()(void *p) const { (void)hipHostFree(p); } };
template <class T> using Pinned = std::unique_ptr<T[], HostFree>;
template <class T> hipError_t host_alloc(Pinned<T> &h, size_t count) {
    h.reset();
    void *q = nullptr;
    const hipError_t e = hipHostMalloc(&q, sizeof(T) * count, hipHostMallocDefault);
    h.reset(static_cast<T *>(q));
    return e;
}

// A structure derived from the active matrix, the lane shape or P(z|w,d).  Only its builder (ensure_*) marks it valid;
// invalidate() keeps its allocations for the next build (bootstrap members reuse them), drop() frees them as well.
template <class T> struct Derived {
    bool valid = false;
    void invalidate() { valid = false; }
    void drop() { static_cast<T &>(*this) = T{}; }
};

struct Timed {
    int name_id;
    Event a, b;
};

}  // namespace

// Every resource is owned by its member and freed with the context; the streams come first, so that they outlive the
// buffers and events declared after them.
struct plsa_ctx {
    int device = 0;
    Stream stream;
    Stream stream2;                  // column-side chain of the fused iteration (overlaps the document pass)
    hipStream_t ls = nullptr;        // stream the kernel wrappers currently launch on (LaunchOn)
    Event ev_fork, ev_join;
    Event ev_row, ev_tail;           // pipelined small-corpus iteration: document pass done / column chain done
    bool overlap = true;
    double overlap_full_limit = 2e9;   // nnz * kp below which both passes run side by side (PLSA_OVERLAP_FULL_LIMIT)
    std::string err;
    hipDeviceProp_t prop;
    int grid_cap = 2048;

    // corpus
    i64 bn = 0, bm = 0, bnnz = 0;
    DevBuf b_indptr, b_col, b_val;
    bool active_is_base = true;
    i64 n = 0, m = 0, nnz = 0;
    DevBuf a_indptr, a_col, a_val;
    const int *indptr = nullptr, *col = nullptr;
    const float *val = nullptr;
    struct RowIndex : Derived<RowIndex> { DevBuf ids; } rowidx;   // COO row ids of the active matrix

    // CSC copy + column items + the columns with heavy_items items or more (Zipf head words) + the column pass' XCD stretches
    struct Csc : Derived<Csc> {
        DevBuf colptr, row, val, pos, item_first, item_col, item_start, item_end, item_order, heavy_cols;
        DevBuf item_rec;             // visiting-order item records
        DevBuf xcd_lo;               // chunk boundaries per XCD (measured, see ensure_balance)
        bool balanced = false;       // xcd_lo matches the current structure
        int seg = 256, n_heavy = 0;  // column item length
        i64 n_items = 0;
    } csc;
    int seg_override = 0, struct_lpn = 0;   // column item length: adaptive unless PLSA_COL_SEG is set
    int struct_row_lpn = 0;          // document-pass lane count the row items were sized for (struct_lpn: the column pass')
    DevBuf partial;
    bool use_item_order = true, xcd_split = true;
    // packed entry streams of the fused passes (plsa_kernels.hpp: Packed) in the line layout (plsa_launch_plan.hpp): pk_csr
    // holds the documents (or, in row-item mode, the row items) of col / val in blocks of 4 * row_lpn words, pk_csc the column
    // items of csc.row / csc.val in blocks of 4 * lpn words.  A stream is used (ok) when its ids fit 24 bits, at most 1/16
    // of the entries escape and its words fit 32-bit offsets.
    bool packed = true;              // PLSA_PACKED=0: the two-array streams everywhere (A/B)
    struct PackedStream : Derived<PackedStream> {
        DevBuf buf;
        DevBuf blk;                  // pk_csr over whole documents: n + 1 block offsets
        int lpn = 0, seg = 0;        // what the layout was written for: lane count; item length (0: whole documents)
        i64 words = 0;
        bool ok = false;
        bool reshape = false;        // pk_csc: invalidated by a lane-shape change that kept the CSC copy (ensure_csc writes it again)
        int state() const { return !valid ? -1 : (ok ? 1 : 0); }   // -1 not built, 0 the pass runs on the arrays, 1 packed
    } pk_csr, pk_csc;
    DevBuf pk_count;
    int chunks_per_lane = 2;
    int row_lpn = 1, row_ch = 1;     // lane shape of the DOCUMENT pass (may differ from lpn / ch: see set_shape)
    bool row_shape_8x2 = true;       // PLSA_ROW_SHAPE=0: document pass in the common shape
    bool p_lent = false;           // plsa_p_reserve handed this context's P(z|w,d) address out: it must not move (no regrowth) until plsa_release_scratch
    int e_rows = -1;               // E-step traversal: 1 document-owned, 0 one group per non-zero, -1 by size (PLSA_E_ROWS)
    int mt_streams = 256;          // pieces the MT19937 init stream is cut into (PLSA_MT_STREAMS; 1 = sequential)
    i64 mt_min_blocks = 4096;      // ... once it is at least this many 624-word blocks long (PLSA_MT_MIN_BLOCKS)
    int heavy_items = 32;

    // row items (documents cut into pieces) for corpora with few / very uneven rows
    bool force_wide = false;           // PLSA_FORCE_WIDE: 64-bit gather addresses whatever the table size
    struct RowItems : Derived<RowItems> {
        DevBuf first, row, start;
        bool use = false;
        int seg = 64;                // entries per row item
        i64 n = 0;
    } ritems;
    int rseg_override = 0, ritems_mode = -1;   // ritems_mode: -1 auto, 0 never, 1 always (PLSA_ROW_ITEMS); PLSA_ROW_SEG (0 = by size)
    DevBuf rpartial;

    // items of the document-owned E-step: documents cut into pieces of seg entries (balanced: the four
    // groups of a wave all run the same number of gather/store bursts; measured 5.27 -> 4.62 ms at config 3)
    struct EItems : Derived<EItems> { DevBuf row, start; int seg = 0; i64 n = 0; } eitems;
    int eseg_override = -1;          // PLSA_E_SEG: -1 auto, 0 whole documents, N pieces of N entries

    // rows in descending-length order (row-owned kernels: groups of a wave finish together)
    bool sort_rows = true;
    struct RowOrder : Derived<RowOrder> {
        DevBuf ids;
        int range = 0;               // documents per range the order was built for (0: plain length order)
    } roworder;
    // parameters of the last topical corpus generated on this context (plsa_synthetic_dominant_topics)
    i64 syn_n = 0; int syn_k0 = 0; double syn_alpha = 0.0; uint64_t syn_seed = 0;
    bool row_xcd = false;            // PLSA_ROW_XCD=1 (experiment): XCD x walks the x-th eighth of the documents (k_row_pass)

    // factors
    int k = 0, kp = 0, lpn = 1, ch = 1;
    DevBuf U[3], Vt[3], Vacc;      // [2]: third buffers of the speculating fit loop (plsa_fit); cu, cv stay in {0, 1} outside it
    bool rot3 = false;             // inside that loop: the output buffers are (cu + 1) % 3, (cv + 1) % 3
    int speculate = -1;            // PLSA_SPECULATE: -1 small corpora only, 0 never, 1 whenever the loop allows
    Event ev_ll;                   // likelihood of a test has reached the host buffer
    int cu = 0, cv = 0;
    i64 fac_n = 0, fac_m = 0;
    DevBuf P;                      // borrowed while it lives in memory lent by plsa_p_borrow
    struct PState : Derived<PState> {} p_state;   // P holds the responsibilities of the current factors (or plsa_set_p's)
    // arithmetic of the kernel-level operators and drivers (plsa_set_arithmetic; PLSA_REFERENCE_SUMS / PLSA_REFERENCE_LL of plsa_fit):
    // ref_sums: every factor sum one float32 accumulator in the reference's loop order (plsa_ref_kernels.hpp)
    // ref_ll:   the log-likelihood one float32 running sum over the non-zeros (plsa.py:322 read literally)
    bool ref_sums = false, ref_ll = false;
    DevBuf ref_terms;              // float32 [nnz]: per-entry log-likelihood terms of the sequential sum
    // norm_pwz of the reference arithmetic from per-chunk parity pairs (k_ref_pair_*): PLSA_REF_CHAIN = pairs | serial | auto
    // (auto, default: pairs from 4096 non-zeros on, back to the serial chain for the rest of a corpus' fits once more than a
    // quarter of the chunks of an iteration took the walk's slow way -- chains that drift too far from the real sums)
    int ref_chain_mode = 0;        // 0 auto, 1 always pairs, 2 always the serial chain
    bool ref_pairs_off = false;    // auto mode: the current corpus went back to the serial chain
    DevBuf ref_csum, ref_pairs, ref_exps, ref_pairs2, ref_exps2, ref_stats, ref_ll_neg;
    // tile sums of x * P(z|w,d) [* sw] left by the last reference-arithmetic E-step (valid for THAT P and THOSE weights only)
    struct RefTileSums : Derived<RefTileSums> {
        DevBuf sums;
        const float *sw = nullptr;   // weights the sums were formed with
        int tj = 0;                  // entries per tile
    } ref_tsum;
    const float *ref_e_sw = nullptr; // weights the next E-step should form its tile sums with
    bool ref_e_no_sums = false;      // the E-steps of a refit: no norm_pwz chain follows
    struct RefHeavy : Derived<RefHeavy> { DevBuf cols; int n = 0, min = 0; } ref_heavy;   // the reference arithmetic's long columns: [count, columns...]
    // plsa_set_p_budget: the drivers' reference arithmetic with P(z|w,d) of one block of documents at a time.  The plan cuts the
    // ACTIVE matrix' documents greedily into blocks [doc[b], doc[b + 1]) = entries [ent[b], ent[b + 1]) that fit the budget.
    int64_t p_budget = 0;          // bytes; 0: none (P holds all non-zeros)
    struct RefBlocks : Derived<RefBlocks> {
        std::vector<i64> doc, ent;
        int64_t budget = 0;        // the budget and the padded topic count the plan was made for
        int kp = 0;
        i64 largest = 0;           // non-zeros of the largest block
        int blocks() const { return (int)doc.size() - 1; }
    } ref_blocks;
    struct PBlockInfo { int64_t budget = 0; int blocks = 0; int64_t largest = 0, p_bytes = 0; } p_block_info;   // last driver iteration
    Pinned<unsigned long long> h_ref_stats;   // [2]: chunks that took the slow way / chunks, of the last finished walk
    Event ev_ref_stats;
    bool ref_stats_pending = false;
    unsigned long long ref_slow_total = 0, ref_chunks_total = 0;   // accumulated over the walks read back so far (plsa_reference_chain_info)
    int placement_candidates = 4, placement_tried = 0;
    double placement_gbps[2] = {0.0, 0.0};
    size_t p_shift = 0;   // experiment knob: byte offset of P inside its allocation (PLSA_P_OFFSET_KB)

    // small buffers
    DevBuf sw, ll_partials, ll_out, colsum_partials, norm_pwz, norm_pdz, tmp0, tmp1, tmp2, cubtmp;
    DevBuf mt_seq;                                // chunk sums / parity pairs / binade guesses of the topic marginals
    bool mt_chain = false;                        // PLSA_MT_CHAIN
    DevBuf mt_words, mt_state, mt_fin, mt_poly;   // MT19937 initialisation scratch: kept between calls (an ensemble member per call:
                                                  // four hipMalloc + four hipFree per member cost more than the generator kernels)
    Pinned<double> h_ll;

    DevBuf colsum_rows, colsum_rows2;
    // plsa_codocument_counts: one 32-bit mask per document and set of a chunk; the chunk's word lists and counters.  Kept
    // between calls (a sweep scores one model after the other), freed by plsa_release_scratch
    DevBuf metric_mask, metric_small;
    // KL-divergence NMF (plsa_nmf.hpp): W_sum / H_sum as float64 [2][kp] and guarded float32 [2][kp], the slab sums they are
    // added up from, the objective's per-workgroup partials and its result.  W and H themselves live in U[cu] / Vt[cv]
    struct Nmf { DevBuf raw, guarded, slabs, obj, out; } nmf;
    // plsa_score_rows (plsa_score.hpp): the CSR arrays of ANOTHER matrix with the active matrix's shape, the validation flag
    // and the three per-document sums [3][n].  Kept between calls, freed by plsa_release_scratch; never part of the corpus
    struct Score { DevBuf indptr, col, val, flag, out; } score;
    // tempered EM (plsa_tempered.hpp): the two side tables U^beta [n, kp] and Vt^beta [m, kp] of the iteration in flight, and
    // the one snapshot slot of plsa_factors_snapshot with the shape it was taken for.  4 kp (n + m) bytes each, kept between
    // calls, freed by plsa_release_scratch
    struct Tempered {
        DevBuf U, Vt, snapU, snapVt;
        bool have_snap = false;
        i64 snap_n = 0, snap_m = 0;
        int snap_k = 0;
    } tempered;
    // smoothed EM (plsa_smoothed.hpp): norm_pdz [n] of the document pass in flight, which k_smooth_rows reads right behind it
    // (nothing else ever does: no validity to keep), the slab partials [2][256] of k_log_prior, its two sums and the page-locked
    // slot they are copied to.  Kept between calls, freed by plsa_release_scratch
    struct Smoothed { DevBuf norm_pdz, partials, out; Pinned<double> h_out; } smoothed;
    // variational Bayes LDA (plsa_lda.hpp): the exp-digamma side tables A [n, kp] and B [m, kp] of the state in force (valid
    // only inside the call that formed them), the float64 sums S_d, psi(S_d) [n] and S_z, psi(S_z) [kp] they were formed with,
    // norm_pdz [n] of the document pass in flight, the slab partials [2][256] of k_lda_bound, its two sums and the page-locked
    // slot they are copied to.  Kept between calls, freed by plsa_release_scratch
    struct Lda { DevBuf A, B, sums, norm_pdz, partials, out; Pinned<double> h_out; bool a_valid = false, b_valid = false; } lda;
    // LDA's vector and learned priors (plsa_lda_priors.hpp): the prior vector as float64 [kp] and float32 [kp], the slab partials
    // [min(4096, rows)][kp] of k_lda_logmean, its sums [2][kp] and the page-locked slot [4 kp] the sums arrive in and the vector
    // leaves from.  Kept between calls, freed by plsa_release_scratch
    struct LdaPrior { DevBuf alpha, partials, t; Pinned<double> h; int h_kp = 0; } lda_prior;
    DevBuf t_end;                    // end stamps of the column pass' timed tuning launches (ensure_balance)
    bool pipeline = true;            // PLSA_PIPELINE=0: fork/join form of the small-corpus iteration (A/B)
    bool graph = false;              // PLSA_GRAPH=1: hipGraph replay of the iterations between two likelihood tests
    int order_band = -1;             // PLSA_ORDER_BAND: documents per band of the visiting order (-1 auto, 0 first-document order)
    int balance = -1;                // PLSA_BALANCE: -1 auto (large problems), 0 equal stretches, 1 always measure
    bool bal_have_frac = false;      // bal_frac holds measured boundaries (kept across bootstrap resamples as the start)
    double bal_frac[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int bal_lo[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    i64 bal_chunks = -1;
    int bal_launches = 0;            // timed tuning launches spent on the current structure
    double bal_end_us[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // per-XCD finish times of the last timed launch
    int small_grid = 0;              // PLSA_SMALL_GRID: workgroups per CU of the column pass on small corpora (0 = no cap)
    int colsum_rows_used = 0;        // rows of colsum_rows written by the last column pass
    // plsa_fit_info: how the last plsa_fit / plsa_refit ran (written where the decisions are made, read by tests only)
    struct FitInfo {
        int fused = 0, pipelined = 0, speculated = 0, graph_launches = 0;
        int tail = 0;                // column tail: 0 none ran, 1 the single sweep (k_col_reduce_norm), 2 the four-kernel form
        int two_stage = 0;           // norm_pwz went through k_norm_reduce
        int xcd_split = 0;           // the last column pass walked its chunks in per-XCD stretches
    } fit_info;

    // multi-GPU exchange: one RCCL communicator per context (one process per GPU), collectives are
    // enqueued on the context's own streams
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    bool sharded = false;            // PLSA_SHARDED fit in progress: accumulators / likelihoods are all-reduced
    bool sw_resident = false;   // plsa_set_sample_weight: sw_res holds weights that apply whenever a call passes sw = NULL
    i64 sw_n = 0;               // (their own buffer: a call that passes explicit weights stages them in c->sw and leaves these alone)
    DevBuf sw_res;
    DevBuf comm_send, comm_recv, comm_small, comm_stack;   // comm_stack: the member stack (plsa_stack_reserve)
    Pinned<float> comm_host;         // landing buffer of plsa_comm_allgather_stack
    size_t comm_host_cap = 0;

    // timing
    bool timing = false;
    std::vector<std::string> names;
    std::vector<Timed> timed;
    std::vector<Event> pool;
    std::vector<double> acc_ms;
    std::vector<i64> acc_n;
};

namespace {

inline float *p_base(plsa_ctx *c) { return reinterpret_cast<float *>(reinterpret_cast<char *>(c->P.p) + c->p_shift); }

int fail(plsa_ctx *c, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_err = buf;
    return 1;
}

#define HIPCHK(c, expr)                                                                            \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail((c), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,      \
                        __LINE__);                                                                 \
    } while (0)

#define CHK(expr)                                                                                  \
    do {                                                                                           \
        int r_ = (expr);                                                                           \
        if (r_) return r_;                                                                         \
    } while (0)

#define NCCLCHK(c, expr)                                                                           \
    do {                                                                                           \
        ncclResult_t n_ = (expr);                                                                  \
        if (n_ != ncclSuccess)                                                                     \
            return fail((c), "%s failed: %s (%s:%d)", #expr, ncclGetErrorString(n_), __FILE__,     \
                        __LINE__);                                                                 \
    } while (0)

int grid_for(plsa_ctx *c, i64 work_items, int items_per_block);
bool g_contig = false;   // PLSA_CONTIG=1: ask for physically contiguous HBM for large buffers

int ensure(plsa_ctx *c, DevBuf &b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return 0;
    // a buffer that GROWS is one whose size follows the data of the moment (the non-zeros of a bootstrap resample vary by
    // a fraction of a percent from member to member): 6 % head-room ends the hipFree + hipMalloc pairs (device-wide
    // synchronisations) after the first few members.  First allocations and buffers of 1 GB or more stay exact.
    if (b.p && bytes < ((size_t)1 << 30)) bytes += bytes / 16;
    if (b.p) { HIPCHK(c, hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    if (g_contig && bytes >= ((size_t)64 << 20)) {
        if (hipExtMallocWithFlags(&b.p, bytes, hipDeviceMallocContiguous) == hipSuccess) { b.cap = bytes; return 0; }
        (void)hipGetLastError();
        b.p = nullptr;
    }
    HIPCHK(c, hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return 0;
}

// HBM placement matters for the streamed P array: the same kernel on the same data ran 6.3 ... 7.4 ms
// depending only on which physical pages hipMalloc happened to hand out (tools/p_offset_probe*.py;
// the start offset inside one allocation is irrelevant).  For that one buffer the engine therefore
// allocates a few candidates, streams a non-temporal fill through each (~5 ms per 25 GB) and keeps
// the fastest.  Candidates are held simultaneously so the allocator cannot return the same pages.
int ensure_best_placement(plsa_ctx *c, DevBuf &b, size_t bytes, int max_candidates, double *gbps, int *n_tried) {
    if (b.cap >= bytes) return 0;
    if (gbps) { gbps[0] = gbps[1] = 0.0; }
    if (n_tried) *n_tried = 0;
    if (b.p) { HIPCHK(c, hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    size_t free_b = 0, total_b = 0;
    int ncand = 1;
    if (max_candidates > 1 && hipMemGetInfo(&free_b, &total_b) == hipSuccess)
        ncand = (int)std::min<size_t>((size_t)max_candidates, (size_t)((double)free_b * 0.6) / std::max<size_t>(bytes, 1));
    if (ncand < 2 || bytes < ((size_t)256 << 20)) return ensure(c, b, bytes);
    std::vector<void *> cand;
    std::vector<float> ms;
    Event e0, e1;
    (void)hipEventCreate(&e0.h); (void)hipEventCreate(&e1.h);
    const i64 n4 = (i64)(bytes / 16);
    const int grid = grid_for(c, n4, 256);
    for (int i = 0; i < ncand; ++i) {
        void *p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); break; }
        cand.push_back(p);
        hipLaunchKernelGGL((plsa::k_probe_fill<true>), dim3(grid), dim3(256), 0, c->stream, (float *)p, n4);   // first touch
        (void)hipEventRecord(e0, c->stream);
        hipLaunchKernelGGL((plsa::k_probe_fill<true>), dim3(grid), dim3(256), 0, c->stream, (float *)p, n4);
        hipLaunchKernelGGL((plsa::k_probe_fill<true>), dim3(grid), dim3(256), 0, c->stream, (float *)p, n4);
        (void)hipEventRecord(e1, c->stream);
        (void)hipStreamSynchronize(c->stream);
        float t = 0.f;
        (void)hipEventElapsedTime(&t, e0, e1);
        ms.push_back(t / 2.f);
    }
    if (cand.empty()) return ensure(c, b, bytes);
    size_t best = 0, worst = 0;
    for (size_t i = 1; i < cand.size(); ++i) { if (ms[i] < ms[best]) best = i; if (ms[i] > ms[worst]) worst = i; }
    for (size_t i = 0; i < cand.size(); ++i) if (i != best) (void)hipFree(cand[i]);
    b.p = cand[best]; b.cap = bytes;
    if (gbps) { gbps[0] = bytes / 1e9 / (ms[best] / 1e3); gbps[1] = bytes / 1e9 / (ms[worst] / 1e3); }
    if (n_tried) *n_tried = (int)cand.size();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Large host <-> device copies.  The boundary takes ordinary (pageable) host arrays -- NumPy's -- and a plain hipMemcpy
// of such memory ran at 25 GB/s up / 10 GB/s down on the GPU box (profiles/r05_pcie_inclusive_plsa_fit_from_host.jsonl: 60 of
// the 72 ms a config-3 fit spends outside its iterations).  From STAGE_MIN bytes on, a copy is cut into 8-MB chunks that
// STAGE_THREADS helper threads move through page-locked slots of their own (two each, one HIP stream each): the host-side
// memcpy of one chunk (and the first-touch page faults of a fresh destination array) overlaps the PCIe transfer of the
// others.  The slots are process-wide (64 MB page-locked once), copies of different contexts take turns.
// ---------------------------------------------------------------------------------------------
constexpr size_t STAGE_CHUNK = (size_t)8 << 20;
constexpr int STAGE_THREADS_MAX = 8;
int g_stage_threads = 4;          // helper threads in use (PLSA_STAGE_THREADS, 1 .. 8)
constexpr size_t STAGE_MIN = (size_t)48 << 20;
struct HostStage {
    std::mutex mu;
    int device = -1;
    void *slot[STAGE_THREADS_MAX][2] = {};
    hipStream_t stream[STAGE_THREADS_MAX] = {};
    hipEvent_t ev[STAGE_THREADS_MAX][2] = {};
    bool ok = false, tried = false;
} g_stage;

bool stage_ready(int device) {        // (g_stage.mu held)
    if (g_stage.tried && g_stage.device == device) return g_stage.ok;
    if (g_stage.tried) {              // another device: rebuild the streams / events there, keep the host slots
        for (int t = 0; t < STAGE_THREADS_MAX; ++t) {
            if (g_stage.stream[t]) (void)hipStreamDestroy(g_stage.stream[t]);
            for (int b = 0; b < 2; ++b) if (g_stage.ev[t][b]) (void)hipEventDestroy(g_stage.ev[t][b]);
            g_stage.stream[t] = nullptr; g_stage.ev[t][0] = g_stage.ev[t][1] = nullptr;
        }
    }
    g_stage.tried = true; g_stage.device = device; g_stage.ok = true;
    const char *off = getenv("PLSA_STAGED_COPIES");
    if (off && atoi(off) == 0) { g_stage.ok = false; return false; }
    const char *nt = getenv("PLSA_STAGE_THREADS");
    if (nt) g_stage_threads = std::max(1, std::min(STAGE_THREADS_MAX, atoi(nt)));
    for (int t = 0; t < g_stage_threads && g_stage.ok; ++t) {
        for (int b = 0; b < 2; ++b) {
            if (!g_stage.slot[t][b] && hipHostMalloc(&g_stage.slot[t][b], STAGE_CHUNK, hipHostMallocDefault) != hipSuccess) g_stage.ok = false;
            if (hipEventCreateWithFlags(&g_stage.ev[t][b], hipEventDisableTiming) != hipSuccess) g_stage.ok = false;
        }
        if (hipStreamCreateWithFlags(&g_stage.stream[t], hipStreamNonBlocking) != hipSuccess) g_stage.ok = false;
    }
    if (!g_stage.ok) (void)hipGetLastError();
    return g_stage.ok;
}

// dev <- host (to_device) or host <- dev, `bytes` contiguous on both sides.  The caller has synchronised whatever produced
// the source; on return the data is in place (every helper stream drained).  Returns false if the staged path is unavailable.
bool staged_copy(plsa_ctx *c, void *dev, void *host, size_t bytes, bool to_device) {
    if (bytes < STAGE_MIN) return false;
    std::lock_guard<std::mutex> lock(g_stage.mu);
    if (!stage_ready(c->device)) return false;
    const size_t n_chunks = (bytes + STAGE_CHUNK - 1) / STAGE_CHUNK;
    const int STAGE_THREADS = g_stage_threads;
    bool failed[STAGE_THREADS_MAX] = {};
    auto worker = [&](int t) {
        if (hipSetDevice(c->device) != hipSuccess) { failed[t] = true; return; }
        hipStream_t st = g_stage.stream[t];
        if (to_device) {
            int b = 0;
            for (size_t i = t; i < n_chunks; i += STAGE_THREADS, b ^= 1) {
                const size_t off = i * STAGE_CHUNK, len = std::min(STAGE_CHUNK, bytes - off);
                if (hipEventSynchronize(g_stage.ev[t][b]) != hipSuccess) { failed[t] = true; return; }   // the slot's previous transfer
                memcpy(g_stage.slot[t][b], (const char *)host + off, len);
                if (hipMemcpyAsync((char *)dev + off, g_stage.slot[t][b], len, hipMemcpyHostToDevice, st) != hipSuccess ||
                    hipEventRecord(g_stage.ev[t][b], st) != hipSuccess) { failed[t] = true; return; }
            }
        } else {
            // chunk j+1 is on its way into the other slot while chunk j is copied out to the caller's pages
            size_t i = t;
            int b = 0;
            auto issue = [&](size_t ci, int slot) {
                const size_t off = ci * STAGE_CHUNK, len = std::min(STAGE_CHUNK, bytes - off);
                return hipMemcpyAsync(g_stage.slot[t][slot], (const char *)dev + off, len, hipMemcpyDeviceToHost, st) == hipSuccess &&
                       hipEventRecord(g_stage.ev[t][slot], st) == hipSuccess;
            };
            if (i < n_chunks && !issue(i, b)) { failed[t] = true; return; }
            for (; i < n_chunks; i += STAGE_THREADS, b ^= 1) {
                const size_t nxt = i + STAGE_THREADS;
                if (nxt < n_chunks && !issue(nxt, b ^ 1)) { failed[t] = true; return; }
                if (hipEventSynchronize(g_stage.ev[t][b]) != hipSuccess) { failed[t] = true; return; }
                const size_t off = i * STAGE_CHUNK, len = std::min(STAGE_CHUNK, bytes - off);
                memcpy((char *)host + off, g_stage.slot[t][b], len);
            }
        }
        if (hipStreamSynchronize(st) != hipSuccess) failed[t] = true;
    };
    std::thread th[STAGE_THREADS_MAX];
    for (int t = 1; t < STAGE_THREADS; ++t) th[t] = std::thread(worker, t);
    worker(0);
    for (int t = 1; t < STAGE_THREADS; ++t) th[t].join();
    (void)hipSetDevice(c->device);
    for (int t = 0; t < STAGE_THREADS; ++t)
        if (failed[t]) { (void)hipGetLastError(); return false; }      // the caller repeats the copy the plain way
    return true;
}

// host -> device on the context's stream order: everything enqueued on c->stream so far is complete when the staged path
// writes (it waits), and the data is in place when this returns, so later work on c->stream sees it
int copy_to_device(plsa_ctx *c, void *dev, const void *host, size_t bytes) {
    if (bytes >= STAGE_MIN) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (staged_copy(c, dev, const_cast<void *>(host), bytes, true)) return 0;
    }
    HIPCHK(c, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream));
    return 0;
}

// device -> host; the data is in `host` on return
int copy_to_host(plsa_ctx *c, void *host, const void *dev, size_t bytes) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bytes >= STAGE_MIN && staged_copy(c, const_cast<void *>(dev), host, bytes, false)) return 0;
    HIPCHK(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int name_id(plsa_ctx *c, const char *name) {
    for (size_t i = 0; i < c->names.size(); ++i)
        if (c->names[i] == name) return (int)i;
    c->names.emplace_back(name);
    c->acc_ms.push_back(0.0);
    c->acc_n.push_back(0);
    return (int)c->names.size() - 1;
}

Event get_event(plsa_ctx *c) {
    Event e;
    if (!c->pool.empty()) { e = std::move(c->pool.back()); c->pool.pop_back(); }
    else (void)hipEventCreate(&e.h);
    return e;
}

// folds finished event pairs into the per-kernel totals (requires the stream to be idle)
int timing_flush(plsa_ctx *c) {
    if (c->timed.empty()) return 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream2));
    for (auto &t : c->timed) {
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, t.a, t.b));
        c->acc_ms[t.name_id] += ms;
        c->acc_n[t.name_id] += 1;
        c->pool.push_back(std::move(t.a));
        c->pool.push_back(std::move(t.b));
    }
    c->timed.clear();
    return 0;
}

struct Scope {  // brackets one kernel launch with events when timing is on
    plsa_ctx *c;
    Timed t;
    bool on;
    Scope(plsa_ctx *c_, const char *name) : c(c_), on(c_->timing) {
        if (on) {
            t.name_id = name_id(c, name);
            t.a = get_event(c);
            t.b = get_event(c);
            (void)hipEventRecord(t.a, c->ls);
        }
    }
    ~Scope() {
        if (on) {
            (void)hipEventRecord(t.b, c->ls);
            c->timed.push_back(std::move(t));
        }
    }
};

struct LaunchOn {  // the kernel wrappers launch on `s` inside this scope (c->ls), on the previous stream again after it
    plsa_ctx *c;
    hipStream_t prev;
    LaunchOn(plsa_ctx *c_, hipStream_t s) : c(c_), prev(c_->ls) { c->ls = s; }
    ~LaunchOn() { c->ls = prev; }
};

template <class Fn>
int dispatch_shape(plsa_ctx *c, Fn &&fn) {
    const bool full = c->kp == 4 * c->lpn * c->ch;
#define PLSA_SHAPE(L, H)                                                                           \
    if (c->lpn == L && c->ch == H) {                                                               \
        if (full) fn(plsa::Shape<L, H, true>{}); else fn(plsa::Shape<L, H, false>{});              \
        return 0;                                                                                  \
    }
    PLSA_SHAPE(1, 1) PLSA_SHAPE(2, 1) PLSA_SHAPE(4, 1) PLSA_SHAPE(8, 1) PLSA_SHAPE(16, 1)
    PLSA_SHAPE(32, 1) PLSA_SHAPE(64, 1) PLSA_SHAPE(64, 2) PLSA_SHAPE(64, 4)
    PLSA_SHAPE(16, 2) PLSA_SHAPE(32, 2)
#undef PLSA_SHAPE
    return fail(c, "unsupported topic count k=%d (max 1024)", c->k);
}

// a gathered table of 4 GB or more takes the WIDE instantiations (plsa_launch_plan.hpp); PLSA_FORCE_WIDE=1: any size
bool table_is_wide(plsa_ctx *c, i64 rows) { return plsa::plan::table_is_wide(rows, c->kp, c->force_wide); }

template <class Fn>
int dispatch_shape_gather(plsa_ctx *c, bool wide, Fn &&fn) {
    if (!wide) return dispatch_shape(c, fn);
#define PLSA_SHAPE(L, H)                                                                           \
    if (c->lpn == L && c->ch == H) { fn(plsa::Shape<L, H, false, true>{}); return 0; }
    PLSA_SHAPE(1, 1) PLSA_SHAPE(2, 1) PLSA_SHAPE(4, 1) PLSA_SHAPE(8, 1) PLSA_SHAPE(16, 1)
    PLSA_SHAPE(32, 1) PLSA_SHAPE(64, 1) PLSA_SHAPE(64, 2) PLSA_SHAPE(64, 4)
    PLSA_SHAPE(16, 2) PLSA_SHAPE(32, 2)
#undef PLSA_SHAPE
    return fail(c, "unsupported topic count k=%d (max 1024)", c->k);
}

// lane shape of the document pass (k_row_pass, k_row_reduce); it gathers P(w|z) rows: m of them
template <class Fn>
int dispatch_shape_row(plsa_ctx *c, Fn &&fn) {
    const bool wide = table_is_wide(c, c->m);
    if (c->row_lpn == 8 && c->row_ch == 2 && c->kp == 64) {
        if (wide) fn(plsa::Shape<8, 2, false, true>{}); else fn(plsa::Shape<8, 2, true>{});
        return 0;
    }
    return dispatch_shape_gather(c, wide, fn);
}

int launch_check(plsa_ctx *c, const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, "launch of %s failed: %s", what, hipGetErrorString(e));
    return 0;
}

// buffers the passes write (the alternates of the current factors)
inline int out_u(const plsa_ctx *c) { return c->rot3 ? (c->cu + 1) % 3 : 1 - c->cu; }
inline int out_v(const plsa_ctx *c) { return c->rot3 ? (c->cv + 1) % 3 : 1 - c->cv; }

int grid_for(plsa_ctx *c, i64 work_items, int items_per_block) {
    return plsa::plan::grid_for(work_items, items_per_block, c->grid_cap);
}

}  // namespace

#include "plsa_structures.hpp"   // what is derived from the active matrix and the lane shape: builders and invalidation rules

namespace {

int upload_sw(plsa_ctx *c, const float *sw, const float **d_sw) {
    *d_sw = nullptr;
    if (!sw) {
        // weights made resident by plsa_set_sample_weight: no copy, no host wait (the per-iteration calls of the
        // split doc-sharded loop stay enqueue-only)
        if (c->sw_resident) {
            if (c->sw_n != c->n) return fail(c, "resident sample weights were set for %lld documents, the active matrix has %lld",
                                              (long long)c->sw_n, (long long)c->n);
            *d_sw = c->sw_res.as<float>();
        }
        return 0;
    }
    CHK(ensure(c, c->sw, sizeof(float) * (size_t)c->n));
    HIPCHK(c, hipMemcpyAsync(c->sw.p, sw, sizeof(float) * (size_t)c->n, hipMemcpyHostToDevice, c->stream));
    // `sw` is borrowed for the call only (it may be a temporary of the caller): the copy must have left the host
    // buffer before any stream-ordered entry point (plsa_em_accumulate) returns
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *d_sw = c->sw.as<float>();
    return 0;
}

int need_factors(plsa_ctx *c) {
    if (c->k <= 0 || !c->U[0].p || !c->Vt[0].p) return fail(c, "factors not set (call plsa_set_factors)");
    if (c->n <= 0) return fail(c, "no corpus uploaded");
    if (c->fac_n != c->n || c->fac_m != c->m)
        return fail(c, "factors were set for a %lld x %lld matrix but the active matrix is %lld x %lld "
                       "(call plsa_set_factors after plsa_upload_csr / plsa_bootstrap)",
                    (long long)c->fac_n, (long long)c->fac_m, (long long)c->n, (long long)c->m);
    return 0;
}

// how an entry point that takes weights opens when it refuses nothing in between: the device, the factors, the weights
int open_weighted(plsa_ctx *c, const float *sw, const float **d_sw) {
    HIPCHK(c, hipSetDevice(c->device));
    CHK(need_factors(c));
    return upload_sw(c, sw, d_sw);
}

// ---------------------------------------------------------------------------------------------
// kernel wrappers
// ---------------------------------------------------------------------------------------------
// Compile-time choices of a pass' instantiation.  A bool picks its tag at run time; a caller that fixes a choice passes the
// tag itself (std::false_type{}) and only that branch is instantiated.
template <class Fn> void with_flag(bool v, Fn &&fn) { if (v) fn(std::true_type{}); else fn(std::false_type{}); }
template <bool V, class Fn> void with_flag(std::integral_constant<bool, V> v, Fn &&fn) { fn(v); }

// P(z|w,d) for `rows` non-zeros (all of them, or the largest block of a budgeted reference-arithmetic iteration)
int ensure_p(plsa_ctx *c, i64 rows) {
    {   // the materialised schedule needs the whole nnz x kp array: say so instead of a bare OOM
        const size_t need = sizeof(float) * (size_t)(rows + 64) * (size_t)c->kp;
        size_t free_b = 0, total_b = 0;
        if (!c->P.borrowed && c->P.cap < need && hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b + c->P.cap < need)
            return fail(c, c->ref_sums ? "the reference arithmetic (PLSA_REFERENCE_SUMS) stores P(z|w,d) like the reference does: %.1f GB needed, "
                                         "%.1f GB of HBM free -- at this size only the default arithmetic is available, or this one block "
                                         "of documents at a time (plsa_set_p_budget / p_budget=, plsa_fit and plsa_refit)"
                                       : "materialising P(z|w,d) needs %.1f GB but only %.1f GB of HBM are free; use the fused "
                           "schedule (PLSA_FUSED), which never stores it, or tile the documents (plsa_em_accumulate_materialised)", need / 1e9, (free_b + c->P.cap) / 1e9);
    }
    if (c->P.borrowed || c->p_lent) {
        const size_t need = sizeof(float) * (size_t)(rows + 64) * (size_t)c->kp;
        if (c->P.cap < need)
            return fail(c, c->P.borrowed ? "the borrowed P(z|w,d) buffer holds %.2f GB, this matrix needs %.2f GB (plsa_p_borrow)"
                                         : "the P(z|w,d) buffer lent out by plsa_p_reserve holds %.2f GB, this matrix needs %.2f GB: it cannot "
                                           "grow while other contexts hold its address (end the loans, then plsa_release_scratch)",
                        c->P.cap / 1e9, need / 1e9);
        c->p_shift = 0;
    } else
    // one tile (64 rows) of slack: the last tile is stored without a predicate
    {   // placement experiment knobs: PLSA_P_SLACK_MB over-allocates, PLSA_P_OFFSET_KB shifts the start
        const char *s1 = getenv("PLSA_P_SLACK_MB"), *s2 = getenv("PLSA_P_OFFSET_KB");
        // (under a budget: neither knob, and no placement candidates -- they are held side by side while they are compared)
        const bool budgeted = c->ref_sums && c->p_budget > 0;
        const size_t slack = s1 && !budgeted ? (size_t)atoll(s1) << 20 : 0;
        c->p_shift = s2 && !budgeted ? (size_t)atoll(s2) * 1024 : 0;
        CHK(ensure_best_placement(c, c->P, sizeof(float) * (size_t)(rows + 64) * (size_t)c->kp + std::max(slack, c->p_shift),
                                  budgeted ? 1 : c->placement_candidates, c->placement_gbps, &c->placement_tried));
    }
    return 0;
}

}  // namespace

#include "plsa_ref.hpp"       // the reference arithmetic (PLSA_REFERENCE_SUMS / PLSA_REFERENCE_LL): E-step, M-step, blocks, likelihood

namespace {

int run_e_step(plsa_ctx *c, float thresh) {
    c->ref_tsum.invalidate();          // (a new P(z|w,d): the tile sums of the last reference-arithmetic E-step are history)
    CHK(ensure_p(c, c->nnz));
    // Two traversals.  Document-owned: a group keeps its document's P(z|d) row in registers and gathers only
    // P(w|z) rows (config 3 5.3 ms against 6.3 ms for one group per non-zero), and with the documents cut
    // into pieces of 4 index batches every group of a wave runs the same number of gather/store bursts
    // (config 3 5.27 -> 4.62 ms = 71 % of the HBM peak; config 2 0.357 -> 0.235 ms = 71 %).  Tiny corpora
    // (config 1: 84 us in all) keep the flat kernel: one group per non-zero, perfectly balanced, no setup.
    if (c->ref_sums) return run_ref_e_step(c, thresh);
    bool e_rows = c->e_rows < 0 ? (double)c->nnz * c->kp >= 1e8 : c->e_rows != 0;
    if (e_rows) {
        const int eseg = plsa::plan::e_item_len(c->lpn, c->eseg_override);
        CHK(ensure_eitems(c, eseg));
        const bool items = eseg > 0 && c->eitems.n > 0;
        const int grid = grid_for(c, items ? c->eitems.n : c->n, 256 / c->lpn);
        const int *order = nullptr;
        if (!items) CHK(ensure_roworder(c, &order));
        CHK(dispatch_shape(c, [&](auto S) {
            Scope s(c, "k_e_step");
            auto go = [&](auto TN) {      // TN: the denormal-norm rescue is compiled in only for thresholds below TINY_THRESH
                hipLaunchKernelGGL((plsa::k_e_step_rows<decltype(S), decltype(TN)::value>), dim3(grid), dim3(256), 0, c->stream,
                                   c->indptr, c->col, (int)c->n, order, c->U[c->cu].as<float>(), c->Vt[c->cv].as<float>(),
                                   p_base(c), c->kp, thresh, items ? c->eitems.row.as<int>() : nullptr,
                                   items ? c->eitems.start.as<int>() : nullptr, eseg, c->eitems.n);
            };
            if (thresh < plsa::TINY_THRESH) go(std::true_type{}); else go(std::false_type{});
        }));
    } else {
        CHK(ensure_rowidx(c));
        const i64 tiles = (c->nnz + 63) / 64;
        const int grid = grid_for(c, tiles, 4);
        CHK(dispatch_shape(c, [&](auto S) {
            Scope s(c, "k_e_step");
            auto go = [&](auto TN) {
                hipLaunchKernelGGL((plsa::k_e_step<decltype(S), decltype(TN)::value>), dim3(grid), dim3(256), 0, c->stream,
                                   c->rowidx.ids.as<int>(), c->col, c->nnz, c->U[c->cu].as<float>(),
                                   c->Vt[c->cv].as<float>(), p_base(c), c->kp, thresh);
            };
            if (thresh < plsa::TINY_THRESH) go(std::true_type{}); else go(std::false_type{});
        }));
    }
    CHK(launch_check(c, "k_e_step"));
    c->p_state.valid = true;
    return 0;
}

// Instantiation of the document pass in lane shape Sh: fn(stream shape, FROM_P, LL, TINY).  Fused: the packed entry stream
// when it is eligible; TINY: the denormal-norm rescue, compiled in for thresholds below TINY_THRESH only.  From P(z|w,d):
// the two arrays, no likelihood, no rescue.
template <class Sh, class FromP, class Fn>
void select_row_pass(bool packed, FromP from_p, bool want_ll, bool tiny, Fn &&fn) {
    with_flag(from_p, [&](auto FP) {
        if constexpr (decltype(FP)::value) fn(Sh{}, FP, std::false_type{}, std::false_type{});
        else with_flag(want_ll, [&](auto LL) {
            with_flag(tiny, [&](auto TN) { if (packed) fn(plsa::Packed<Sh>{}, FP, LL, TN); else fn(Sh{}, FP, LL, TN); });
        });
    });
}

// Instantiation of the column pass in lane shape Sh: fn(stream shape, FROM_P, TIMED, TINY), as above
template <class Sh, class FromP, class Timed, class Fn>
void select_col_pass(bool packed, FromP from_p, Timed timed, bool tiny, Fn &&fn) {
    with_flag(from_p, [&](auto FP) {
        with_flag(timed, [&](auto TM) {
            if constexpr (decltype(FP)::value) fn(Sh{}, FP, TM, std::false_type{});
            else with_flag(tiny, [&](auto TN) { if (packed) fn(plsa::Packed<Sh>{}, FP, TM, TN); else fn(Sh{}, FP, TM, TN); });
        });
    });
}

// What one document pass is launched with: THE place its structures, scratch and grids are decided (plsa_launch_plan.hpp holds
// the arithmetic).  Nothing here is cached: prepare_row_pass computes it from the context on every call; in the steady state
// every builder and every `ensure` is a no-op.  The builders run on c->stream: called before a fork, it leaves nothing for
// the second stream to build.
struct RowLaunch {
    plsa::plan::RowPass plan;
    bool items, packed, xcd_rows;    // over row items / the packed entry stream / PLSA_ROW_XCD's schedule
    const int *indptr, *colidx;      // colidx: the packed CSR stream when `packed`
    const float *vals;
    const int *sblk;                 // `packed` over whole documents: their block offsets in the stream
    const int *order;                // visiting order of whole documents (nullptr over items, or unsorted)
    const int *ritem_row, *ritem_start, *ritem_first;   // nullptr on whole documents
    float *rpartial;                 // one k-vector per row item (nullptr on whole documents)
    double *ll_partials;             // plan.grid partial sums (sized only when the pass carries the likelihood)
    i64 n_ritems;
    int rseg;
};

int prepare_row_pass(plsa_ctx *c, bool from_p, bool want_ll, RowLaunch &r) {
    CHK(ensure_ritems(c));
    r.items = c->ritems.use && c->ritems.n > 0;
    // PLSA_ROW_XCD (experiment): the visiting list is ordered range by range (range = the documents of one eighth), longest
    // document first inside a range
    r.xcd_rows = !r.items && !from_p && c->sort_rows && row_xcd_range(c) > 0;
    r.plan = plsa::plan::row_pass(c->n, c->ritems.n, r.items, c->row_lpn, c->grid_cap, r.xcd_rows);
    r.order = nullptr;
    if (!r.items) CHK(ensure_roworder(c, &r.order));
    if (r.items) CHK(ensure(c, c->rpartial, sizeof(float) * (size_t)c->ritems.n * c->kp));
    if (want_ll) CHK(ensure(c, c->ll_partials, sizeof(double) * (size_t)r.plan.grid));
    if (!from_p) CHK(ensure_packed_csr(c));
    r.packed = !from_p && c->packed && c->pk_csr.ok;
    r.indptr = c->indptr; r.colidx = r.packed ? c->pk_csr.buf.as<int>() : c->col; r.vals = c->val;
    r.sblk = r.packed && !r.items ? c->pk_csr.blk.as<int>() : nullptr;
    r.ritem_row = r.items ? c->ritems.row.as<int>() : nullptr;
    r.ritem_start = r.items ? c->ritems.start.as<int>() : nullptr;
    r.ritem_first = r.items ? c->ritems.first.as<int>() : nullptr;
    r.rpartial = r.items ? c->rpartial.as<float>() : nullptr;
    r.ll_partials = c->ll_partials.as<double>();
    r.n_ritems = c->ritems.n; r.rseg = c->ritems.seg;
    return 0;
}

// document-owned pass: writes U[1-cu]; optional LL partials of the current factors
int run_row_pass(plsa_ctx *c, bool from_p, bool want_ll, const float *d_sw, float thresh,
                 float *d_norm_pdz, int *ll_blocks) {
    RowLaunch r;
    CHK(prepare_row_pass(c, from_p, want_ll, r));
    CHK(dispatch_shape_row(c, [&](auto S) {
        using Sh = decltype(S);
        const float *U = c->U[c->cu].as<float>(), *Vt = c->Vt[c->cv].as<float>();
        float *Un = c->U[out_u(c)].as<float>();
        const int n = (int)c->n, kp = c->kp;
        select_row_pass<Sh>(r.packed, from_p, want_ll, thresh < plsa::TINY_THRESH, [&](auto SS, auto FP, auto LL, auto TN) {
            Scope s(c, from_p ? "k_row_pass<P>" : want_ll ? "k_row_pass<fused,LL>" : "k_row_pass<fused>");
            hipLaunchKernelGGL((plsa::k_row_pass<decltype(SS), decltype(FP)::value, decltype(LL)::value, decltype(TN)::value>),
                               dim3(r.plan.grid), dim3(256), 0, c->ls, r.indptr, r.colidx, r.vals, r.sblk, n, r.order, U, Vt, p_base(c),
                               Un,
                               d_sw, d_norm_pdz, kp, thresh, r.ll_partials, r.ritem_row, r.ritem_start, r.rseg, r.n_ritems,
                               r.rpartial, r.xcd_rows ? 1 : 0);
        });
        if (r.items) {
            Scope s(c, "k_row_reduce");
            hipLaunchKernelGGL((plsa::k_row_reduce<Sh>), dim3(r.plan.reduce_grid), dim3(256), 0, c->ls,
                               r.ritem_first, n, r.rpartial, Un, d_norm_pdz, kp);
        }
    }));
    CHK(launch_check(c, "k_row_pass"));
    if (ll_blocks) *ll_blocks = r.plan.grid;
    return 0;
}

// What one column pass and its tail are launched with: the counterpart of RowLaunch, by the same rules (prepare_col_pass)
struct ColLaunch {
    plsa::plan::ColPass plan;
    bool packed;                     // the packed entry stream
    int xcd_split;                   // the pass walks its chunks in per-XCD stretches
    const int4 *item_rec;            // item records in visiting order
    i64 n_items;
    const int *csc_row, *csc_pos;    // csc_row: the packed CSC stream when `packed`
    const float *csc_val;
    int slot;                        // `packed`: words per item slot of the stream
    float *partial;                  // one k-vector per item
    double *colsum_rows, *colsum_rows2;   // one float64 sum row per chunk; stage-2 rows of the norm (plan.norm_blocks of them)
    float *norm_pwz;
    const int *item_first, *heavy_cols;
    int n_heavy, heavy_items;
};

int prepare_col_pass(plsa_ctx *c, bool from_p, ColLaunch &l) {
    CHK(from_p ? ensure_csc(c) : ensure_packed_csc(c));
    l.packed = !from_p && c->packed && c->pk_csc.ok;
    l.plan = plsa::plan::col_pass(c->csc.n_items, c->m, c->lpn, c->csc.n_heavy, c->grid_cap);
    l.xcd_split = plsa::plan::xcd_split(c->xcd_split, l.plan.n_chunks, c->n, c->kp) ? 1 : 0;
    CHK(ensure(c, c->partial, sizeof(float) * (size_t)std::max<i64>(c->csc.n_items, 1) * c->kp));
    CHK(ensure(c, c->colsum_rows, sizeof(double) * (size_t)std::max(l.plan.n_chunks, 1) * c->kp));
    CHK(ensure(c, c->norm_pwz, sizeof(float) * (size_t)c->kp));
    if (l.plan.norm_blocks) CHK(ensure(c, c->colsum_rows2, sizeof(double) * (size_t)l.plan.norm_blocks * c->kp));
    l.item_rec = c->csc.item_rec.as<int4>(); l.n_items = c->csc.n_items;
    l.csc_row = l.packed ? c->pk_csc.buf.as<int>() : c->csc.row.as<int>();
    l.csc_pos = c->csc.pos.as<int>(); l.csc_val = c->csc.val.as<float>();
    l.slot = l.packed ? plsa::plan::line_slot(c->pk_csc.seg, c->pk_csc.lpn) : 0;
    l.partial = c->partial.as<float>(); l.norm_pwz = c->norm_pwz.as<float>();
    l.colsum_rows = c->colsum_rows.as<double>(); l.colsum_rows2 = c->colsum_rows2.as<double>();
    l.item_first = c->csc.item_first.as<int>(); l.heavy_cols = c->csc.heavy_cols.as<int>();
    l.n_heavy = c->csc.n_heavy; l.heavy_items = c->heavy_items;
    return 0;
}

// vocabulary-owned pass (no atomics): partial k-vectors per column item (+ per-chunk sums of them, from
// which the column tail gets norm_pwz), then per-column sums -> Vacc
// parts: 1 = the column pass itself, 2 = the un-normalised per-column sums of its partials (k_col_reduce),
//        3 = both
int run_col_pass(plsa_ctx *c, bool from_p, const float *d_sw, float thresh, int parts = 3) {
    ColLaunch l;
    CHK(prepare_col_pass(c, from_p, l));
    int rc = 0;
    CHK(dispatch_shape_gather(c, table_is_wide(c, c->n), [&](auto S) {     // the pass gathers P(z|d) rows: n of them
        using Sh = decltype(S);
        constexpr int GPB = 256 / Sh::LPN;
        const int n_chunks = l.plan.n_chunks, kp = c->kp;
        if (parts & 1) {
            c->fit_info.xcd_split = l.xcd_split;
            const size_t smem = sizeof(double) * (size_t)GPB * kp;
            auto launch = [&](bool timed) -> int {
                int grid = plsa::plan::col_grid(c->bal_lo, n_chunks, l.xcd_split != 0);
                // PLSA_SMALL_GRID (experiment knob): cap the pass of a small corpus at that many workgroups per CU
                if (c->small_grid > 0 && (double)c->nnz * kp < c->overlap_full_limit)
                    grid = std::min(grid, c->small_grid * c->prop.multiProcessorCount);
                Scope s(c, from_p ? "k_col_pass<P>" : "k_col_pass<fused>");
                const int *lo = c->csc.xcd_lo.as<int>();
                const float *U = c->U[c->cu].as<float>(), *Vt = c->Vt[c->cv].as<float>();
                unsigned long long *te = c->t_end.as<unsigned long long>();
                select_col_pass<Sh>(l.packed, from_p, timed, thresh < plsa::TINY_THRESH, [&](auto SS, auto FP, auto TM, auto TN) {
                    hipLaunchKernelGGL((plsa::k_col_pass<decltype(SS), decltype(FP)::value, decltype(TM)::value, decltype(TN)::value>),
                                       dim3(grid), dim3(256), smem, c->ls, l.item_rec, l.n_items, lo, l.csc_row, l.csc_val, l.slot,
                                       l.csc_pos,
                                       U, Vt, p_base(c), d_sw, l.partial, kp, thresh, l.xcd_split, l.colsum_rows, te);
                });
                return launch_check(c, "k_col_pass");
            };
            rc = ensure_balance(c, n_chunks, l.xcd_split != 0, launch);
            if (rc) return;
            rc = launch(false);
            if (rc) return;
            c->colsum_rows_used = n_chunks;
        }
        if (parts & 2) {
            // heavy columns (one block each) and the rest share one launch
            Scope s(c, "k_col_reduce");
            hipLaunchKernelGGL((plsa::k_col_reduce<Sh>), dim3(l.plan.reduce_grid), dim3(256), GPB * kp * sizeof(float), c->ls,
                               l.item_first, (int)c->m, l.heavy_items, l.heavy_cols, l.n_heavy, l.partial, c->Vacc.as<float>(), kp);
        }
    }));
    if (rc) return rc;
    CHK(launch_check(c, "k_col_pass"));
    return 0;
}

// norm_pwz[z] = sum_w Vacc[w, z]: float64 slab sums, added in a fixed order
int run_vacc_norm(plsa_ctx *c) {
    const int nb = (int)std::min<i64>(plsa::NORM_BLOCKS, std::max<i64>(1, c->m));
    CHK(ensure(c, c->colsum_partials, sizeof(double) * (size_t)nb * c->kp));
    {
        Scope s(c, "k_colsum_partial");
        hipLaunchKernelGGL(plsa::k_colsum_partial, dim3(nb), dim3(256), 256 * sizeof(double), c->ls,
                           c->Vacc.as<float>(), (int)c->m, c->kp, c->colsum_partials.as<double>());
    }
    CHK(ensure(c, c->norm_pwz, sizeof(float) * (size_t)c->kp));
    {
        Scope s(c, "k_colsum_final");
        hipLaunchKernelGGL(plsa::k_colsum_final, dim3(1), dim3(256), 0, c->ls,
                           c->colsum_partials.as<double>(), nb, c->kp, c->norm_pwz.as<float>());
    }
    return 0;                        // (the caller's launch_check covers both)
}

// Vacc -> normalised topics in Vt[1-cv]  (plsa.py:196-199)
int run_v_normalise(plsa_ctx *c) {
    if (c->sharded && c->comm) {
        // doc-sharded fit: the un-normalised P(w|z) sums of the local rows become the global sums (the
        // `.sum(axis=0)` over tiles of distributed_plsa.py:116-128 / block_parallel_plsa.py:182-185) --
        // in place, on the stream this chain runs on (underneath the document pass when overlapped)
        Scope s(c, "rccl_allreduce_accumulator");
        NCCLCHK(c, ncclAllReduce(c->Vacc.p, c->Vacc.p, (size_t)c->m * c->kp, ncclFloat, ncclSum, c->comm, c->ls));
    }
    CHK(run_vacc_norm(c));
    {
        Scope s(c, "k_v_normalise");
        const i64 total4 = c->m * c->kp / 4;
        hipLaunchKernelGGL(plsa::k_v_normalise, dim3(grid_for(c, total4, 256)), dim3(256),
                           c->kp * sizeof(float), c->ls, c->Vacc.as<float>(),
                           c->Vt[out_v(c)].as<float>(), (int)c->m, c->kp, c->norm_pwz.as<float>());
    }
    CHK(launch_check(c, "k_v_normalise"));
    return 0;
}

// Everything behind the column pass: norm_pwz from the pass' own per-block sums (two small launches),
// then per-column sums of the item partials and the division in ONE sweep (k_col_reduce_norm) ->
// Vt[1-cv].  The doc-sharded fit needs the un-normalised accumulator for its all-reduce and keeps the
// four-kernel form (k_col_reduce, k_colsum_partial, k_colsum_final, k_v_normalise).
int run_col_tail(plsa_ctx *c) {
    if (c->sharded) {
        c->fit_info.tail = 2;
        c->fit_info.two_stage = 0;
        CHK(run_col_pass(c, false, nullptr, 0.f, 2));
        return run_v_normalise(c);
    }
    ColLaunch l;
    CHK(prepare_col_pass(c, true, l));           // (the tail reads no entry stream: nothing packed to ensure)
    c->fit_info.tail = 1;
    c->fit_info.two_stage = l.plan.norm_blocks > 0;
    if (c->colsum_rows_used <= 0) return fail(c, "internal: column tail without a column pass");
    const double *rows_in = l.colsum_rows;
    int n_rows = l.plan.n_chunks;
    if (l.plan.norm_blocks) {        // many chunks (large corpora): two stages
        Scope s(c, "k_norm_reduce");
        hipLaunchKernelGGL(plsa::k_norm_reduce, dim3(l.plan.norm_blocks), dim3(256), 0, c->ls, rows_in, n_rows, c->kp,
                           l.colsum_rows2);
        rows_in = l.colsum_rows2;
        n_rows = l.plan.norm_blocks;
    }
    {
        Scope s(c, "k_colsum_final");
        hipLaunchKernelGGL(plsa::k_colsum_final, dim3(1), dim3(256), 0, c->ls, rows_in, n_rows, c->kp, l.norm_pwz);
    }
    CHK(dispatch_shape(c, [&](auto S) {
        using Sh = decltype(S);
        constexpr int GPB = 256 / Sh::LPN;
        Scope s(c, "k_col_reduce_norm");
        hipLaunchKernelGGL((plsa::k_col_reduce_norm<Sh>), dim3(l.plan.reduce_grid), dim3(256),
                           sizeof(float) * (size_t)(GPB + 1) * c->kp, c->ls, l.item_first, (int)c->m, l.heavy_items, l.heavy_cols,
                           l.n_heavy, l.partial, l.norm_pwz, c->Vt[out_v(c)].as<float>(), c->kp);
    }));
    return launch_check(c, "k_col_reduce_norm");
}

int finish_ll(plsa_ctx *c, int blocks, double *out) {
    CHK(ensure(c, c->ll_out, sizeof(double)));
    {
        Scope s(c, "k_ll_final");
        hipLaunchKernelGGL(plsa::k_ll_final, dim3(1), dim3(256), 0, c->stream,
                           c->ll_partials.as<double>(), blocks, c->ll_out.as<double>());
    }
    CHK(launch_check(c, "k_ll_final"));
    if (c->sharded && c->comm)      // log-likelihood of all shards: one scalar all-reduce per test
        NCCLCHK(c, ncclAllReduce(c->ll_out.p, c->ll_out.p, 1, ncclDouble, ncclSum, c->comm, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_ll.get(), c->ll_out.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (!out) return hipEventRecord(c->ev_ll, c->stream) == hipSuccess ? 0 : fail(c, "event record failed");   // collected by wait_ll
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out = c->h_ll[0];
    return 0;
}

// second half of finish_ll(c, blocks, nullptr): the host waits for the likelihood only, not for the work enqueued behind it
int wait_ll(plsa_ctx *c, double *out) {
    HIPCHK(c, hipEventSynchronize(c->ev_ll));
    *out = c->h_ll[0];
    return 0;
}

int run_loglik(plsa_ctx *c, const float *d_sw, double *out) {
    if (c->ref_ll) return run_ref_loglik(c, d_sw, out);
    const int grid = grid_for(c, c->n, 256 / c->lpn);
    const int *order = nullptr;
    CHK(ensure_roworder(c, &order));
    CHK(ensure(c, c->ll_partials, sizeof(double) * (size_t)grid));
    CHK(dispatch_shape(c, [&](auto S) {
        Scope s(c, "k_loglik");
        hipLaunchKernelGGL((plsa::k_loglik<decltype(S)>), dim3(grid), dim3(256), 0, c->stream, c->indptr,
                           c->col, c->val, (int)c->n, order, c->U[c->cu].as<float>(),
                           c->Vt[c->cv].as<float>(), d_sw, c->kp, c->ll_partials.as<double>());
    }));
    CHK(launch_check(c, "k_loglik"));
    return finish_ll(c, grid, out);
}

// one M-step from the materialised P: U[1-cu], and (update_v) Vt[1-cv]; swaps the buffers in
int run_m_step_from_p(plsa_ctx *c, const float *d_sw, bool update_v, float *d_norm_pdz) {
    if (!c->p_state.valid) return fail(c, "plsa_m_step: no P(z|w,d) on the device (run plsa_e_step or plsa_set_p)");
    if (c->ref_sums) return run_ref_m_step(c, d_sw, update_v, d_norm_pdz);
    CHK(run_row_pass(c, true, false, nullptr, 0.f, d_norm_pdz, nullptr));
    if (update_v) {
        CHK(run_col_pass(c, true, d_sw, 0.f, 1));
        CHK(run_col_tail(c));
    }
    c->cu ^= 1;
    if (update_v) c->cv ^= 1;
    return 0;
}

// the PLSA_* knobs a context reads when it is created (a member context of a batch reads them like its leader)
void read_knobs(plsa_ctx *c) {
    if (const char *s = getenv("PLSA_OVERLAP")) c->overlap = atoi(s) != 0;
    if (const char *s = getenv("PLSA_OVERLAP_FULL_LIMIT")) c->overlap_full_limit = atof(s);
    if (const char *s = getenv("PLSA_ROW_ITEMS")) c->ritems_mode = atoi(s);
    if (const char *s = getenv("PLSA_PACKED")) c->packed = atoi(s) != 0;
    if (const char *s = getenv("PLSA_ROW_SEG")) c->rseg_override = std::max(1, atoi(s));
    int mult = 128;  // blocks per CU a grid may hold: large (but bounded) grids measured best
    if (const char *s = getenv("PLSA_GRID_MULT")) mult = std::max(1, atoi(s));
    c->grid_cap = c->prop.multiProcessorCount * mult;
    if (const char *s = getenv("PLSA_CONTIG")) g_contig = atoi(s) != 0;
    if (const char *s = getenv("PLSA_PLACEMENT_CANDIDATES")) c->placement_candidates = std::max(1, atoi(s));
    if (const char *s = getenv("PLSA_COL_SEG")) c->seg_override = std::max(1, atoi(s));
    if (const char *s = getenv("PLSA_HEAVY_ITEMS")) c->heavy_items = std::max(1, atoi(s));
    if (const char *s = getenv("PLSA_SORT_ROWS")) c->sort_rows = atoi(s) != 0;
    if (const char *s = getenv("PLSA_ROW_XCD")) c->row_xcd = atoi(s) != 0;
    if (const char *s = getenv("PLSA_ITEM_ORDER")) c->use_item_order = atoi(s) != 0;
    if (const char *s = getenv("PLSA_XCD_SPLIT")) c->xcd_split = atoi(s) != 0;
    if (const char *s = getenv("PLSA_BALANCE")) c->balance = atoi(s);
    if (const char *s = getenv("PLSA_ORDER_BAND")) c->order_band = atoi(s);
    if (const char *s = getenv("PLSA_GRAPH")) c->graph = atoi(s) != 0;
    if (const char *s = getenv("PLSA_PIPELINE")) c->pipeline = atoi(s) != 0;
    if (const char *s = getenv("PLSA_CHUNKS_PER_LANE")) c->chunks_per_lane = atoi(s);
    if (const char *s = getenv("PLSA_E_ROWS")) c->e_rows = atoi(s);
    if (const char *s = getenv("PLSA_E_SEG")) c->eseg_override = atoi(s);
    if (const char *s = getenv("PLSA_MT_STREAMS")) c->mt_streams = std::max(1, std::min(4096, atoi(s)));
    if (const char *s = getenv("PLSA_MT_MIN_BLOCKS")) c->mt_min_blocks = std::max(1, atoi(s));
    if (const char *s = getenv("PLSA_SMALL_GRID")) c->small_grid = std::max(0, atoi(s));
    if (const char *s = getenv("PLSA_ROW_SHAPE")) c->row_shape_8x2 = atoi(s) != 0;
    if (const char *s = getenv("PLSA_FORCE_WIDE")) c->force_wide = atoi(s) != 0;
    if (const char *s = getenv("PLSA_MT_CHAIN")) c->mt_chain = atoi(s) != 0;
    if (const char *s = getenv("PLSA_SPECULATE")) c->speculate = atoi(s);
    c->ref_chain_mode = ref_knobs(c, REF_AT_CREATE).chain_mode;      // (plsa_ref.hpp; the other knobs of the reference arithmetic are read per call)
}

}  // namespace

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

int plsa_device_count(int *count) {
    hipError_t e = hipGetDeviceCount(count);
    if (e != hipSuccess) { *count = 0; return fail(nullptr, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    return 0;
}

const char *plsa_last_error(const plsa_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int plsa_create(int device, plsa_ctx **out) {
    *out = nullptr;
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess || cnt <= 0)
        return fail(nullptr, "no HIP device available (%s)", hipGetErrorString(e));
    if (device < 0 || device >= cnt) return fail(nullptr, "device %d out of range [0,%d)", device, cnt);
    std::unique_ptr<plsa_ctx> owner(new plsa_ctx());      // (a failed creation frees whatever exists so far)
    plsa_ctx *c = owner.get();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&c->prop, device) != hipSuccess)
        return fail(nullptr, "hipSetDevice(%d) failed", device);
    if (strncmp(c->prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, "libplsa_hip is built for gfx950 (MI355X) only; device %d is %s", device,
                    c->prop.gcnArchName);
    // the second stream carries the short column tail underneath the document pass: highest priority, so that its
    // few workgroups are placed as soon as slots free up instead of queueing behind the pass' 32 k workgroups
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    const char *prio_env = getenv("PLSA_TAIL_PRIORITY");
    const bool tail_prio = !prio_env || atoi(prio_env) != 0;
    if (hipStreamCreateWithFlags(&c->stream.h, hipStreamNonBlocking) != hipSuccess ||
        (tail_prio ? hipStreamCreateWithPriority(&c->stream2.h, hipStreamNonBlocking, prio_hi)
                   : hipStreamCreateWithFlags(&c->stream2.h, hipStreamNonBlocking)) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork.h, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join.h, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_row.h, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_tail.h, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_ll.h, hipEventDisableTiming) != hipSuccess ||
        host_alloc(c->h_ll, 2) != hipSuccess)
        return fail(nullptr, "stream / pinned buffer creation failed");
    c->ls = c->stream;
    read_knobs(c);
    *out = owner.release();
    return 0;
}

void plsa_destroy(plsa_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->comm) (void)ncclCommDestroy(c->comm);
    delete c;
}

int plsa_synchronize(plsa_ctx *c) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int plsa_hw_queues(void) {
    const char *s = getenv("GPU_MAX_HW_QUEUES");
    return s && atoi(s) > 0 ? atoi(s) : 4;           // 4: the HIP runtime's default
}

int plsa_device_info(plsa_ctx *c, char *name64, char *arch64, int *cus, int64_t *hbm_bytes) {
    if (name64) { strncpy(name64, c->prop.name, 63); name64[63] = 0; }
    if (arch64) { strncpy(arch64, c->prop.gcnArchName, 63); arch64[63] = 0; }
    if (cus) *cus = c->prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)c->prop.totalGlobalMem;
    return 0;
}

int plsa_upload_csr(plsa_ctx *c, const int32_t *indptr, const int32_t *indices, const float *data,
                    int64_t n, int64_t m, int64_t nnz) {
    HIPCHK(c, hipSetDevice(c->device));
    if (n <= 0 || m <= 0 || nnz < 0) return fail(c, "plsa_upload_csr: bad shape n=%lld m=%lld nnz=%lld",
                                                 (long long)n, (long long)m, (long long)nnz);
    if (n >= INT32_MAX || m >= INT32_MAX || nnz >= INT32_MAX)
        return fail(c, "plsa_upload_csr: n, m and nnz must each be < 2^31");
    if (indptr[0] != 0 || indptr[n] != nnz) return fail(c, "plsa_upload_csr: indptr[0] != 0 or indptr[n] != nnz");
    CHK(ensure(c, c->b_indptr, sizeof(int) * (size_t)(n + 1)));
    CHK(ensure(c, c->b_col, sizeof(int) * (size_t)nnz));
    CHK(ensure(c, c->b_val, sizeof(float) * (size_t)nnz));
    HIPCHK(c, hipMemcpyAsync(c->b_indptr.p, indptr, sizeof(int) * (size_t)(n + 1), hipMemcpyHostToDevice, c->stream));
    if (nnz) {      // (large arrays: chunked through page-locked slots by helper threads, see staged_copy)
        CHK(copy_to_device(c, c->b_col.p, indices, sizeof(int) * (size_t)nnz));
        CHK(copy_to_device(c, c->b_val.p, data, sizeof(float) * (size_t)nnz));
    }
    // the header's contract, checked on the device (the arrays are there now; one streaming pass): a violation is a
    // status code for the caller, not a GPU fault three calls later
    CHK(ensure(c, c->tmp2, 16));
    int bad = 0;
    HIPCHK(c, hipMemsetAsync(c->tmp2.p, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(plsa::k_validate_csr, dim3(grid_for(c, std::max<i64>(n, nnz), 256)), dim3(256), 0, c->stream,
                       c->b_indptr.as<int>(), c->b_col.as<int>(), (i64)n, (i64)m, (i64)nnz, c->tmp2.as<int>());
    CHK(launch_check(c, "k_validate_csr"));
    HIPCHK(c, hipMemcpyAsync(&bad, c->tmp2.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bad) {
        c->bn = c->bm = c->bnnz = 0;                   // nothing usable is resident
        c->n = c->m = c->nnz = 0;
        c->active_is_base = true;
        return fail(c, "plsa_upload_csr: %s%s%s", (bad & 1) ? "indptr is not non-decreasing within [0, nnz]" : "",
                    bad == 3 ? "; " : "", (bad & 2) ? "column index outside [0, m)" : "");
    }
    c->bn = n; c->bm = m; c->bnnz = nnz;
    c->syn_n = 0;
    c->active_is_base = true;
    set_active_pointers(c);
    return 0;
}

int plsa_bootstrap(plsa_ctx *c, const int64_t *idx, int64_t n_out) {
    HIPCHK(c, hipSetDevice(c->device));
    if (c->bn <= 0) return fail(c, "plsa_bootstrap: no corpus uploaded");
    if (!idx) {
        c->active_is_base = true;
        set_active_pointers(c);
        return 0;
    }
    if (n_out <= 0 || n_out >= INT32_MAX) return fail(c, "plsa_bootstrap: bad n_out");
    // idx -> device, row lengths (int64), exclusive scan -> output row pointers
    CHK(ensure(c, c->tmp0, sizeof(i64) * (size_t)n_out));
    CHK(ensure(c, c->tmp1, sizeof(i64) * (size_t)(n_out + 1)));
    CHK(ensure(c, c->tmp2, sizeof(i64) * (size_t)(n_out + 1) + 16));
    i64 *d_idx = c->tmp0.as<i64>();
    int *d_len = c->tmp1.as<int>();
    i64 *d_ptr = c->tmp2.as<i64>();
    int *d_bad = reinterpret_cast<int *>(d_ptr + n_out + 1);
    HIPCHK(c, hipMemcpyAsync(d_idx, idx, sizeof(i64) * (size_t)n_out, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_bad, 0, sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(d_len, 0, sizeof(int) * (size_t)(n_out + 1), c->stream));
    hipLaunchKernelGGL(plsa::k_boot_lengths, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, c->stream,
                       c->b_indptr.as<int>(), d_idx, (i64)n_out, c->bn, d_len, d_bad);
    CHK(launch_check(c, "k_boot_lengths"));
    {
        // int lengths summed into int64 pointers (a resample may exceed the base nnz)
        auto in64 = hipcub::TransformInputIterator<i64, hipcub::CastOp<i64>, int *>(d_len, hipcub::CastOp<i64>());
        auto scan = [&](void *tmp, size_t &bytes) {
            return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, in64, d_ptr, (int)(n_out + 1), c->stream);
        };
        CHK(cub_two_phase(c, "hipcub::DeviceScan::ExclusiveSum", scan));
    }
    i64 total = 0;
    int bad = 0;
    HIPCHK(c, hipMemcpyAsync(&total, d_ptr + n_out, sizeof(i64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bad) return fail(c, "plsa_bootstrap: row index out of range [0,%lld)", (long long)c->bn);
    if (total >= INT32_MAX) return fail(c, "plsa_bootstrap: resampled nnz %lld >= 2^31", (long long)total);
    CHK(ensure(c, c->a_indptr, sizeof(int) * (size_t)(n_out + 1)));
    CHK(ensure(c, c->a_col, sizeof(int) * (size_t)total));
    CHK(ensure(c, c->a_val, sizeof(float) * (size_t)total));
    {
        Scope s(c, "k_boot_gather");
        hipLaunchKernelGGL(plsa::k_boot_gather, dim3(grid_for(c, n_out + 1, 4)), dim3(256), 0, c->stream,
                           c->b_indptr.as<int>(), c->b_col.as<int>(), c->b_val.as<float>(), d_idx,
                           (i64)n_out, d_ptr, c->a_indptr.as<int>(), c->a_col.as<int>(),
                           c->a_val.as<float>());
    }
    CHK(launch_check(c, "k_boot_gather"));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->active_is_base = false;
    c->n = n_out; c->m = c->bm; c->nnz = total;
    set_active_pointers(c);
    return 0;
}

int plsa_active_shape(plsa_ctx *c, int64_t *n, int64_t *m, int64_t *nnz) {
    if (n) *n = c->n;
    if (m) *m = c->m;
    if (nnz) *nnz = c->nnz;
    return 0;
}

int plsa_download_active_csr(plsa_ctx *c, int32_t *indptr, int32_t *indices, float *data) {
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n <= 0) return fail(c, "no corpus uploaded");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (indptr) HIPCHK(c, hipMemcpy(indptr, c->indptr, sizeof(int) * (size_t)(c->n + 1), hipMemcpyDeviceToHost));
    if (indices && c->nnz) HIPCHK(c, hipMemcpy(indices, c->col, sizeof(int) * (size_t)c->nnz, hipMemcpyDeviceToHost));
    if (data && c->nnz) HIPCHK(c, hipMemcpy(data, c->val, sizeof(float) * (size_t)c->nnz, hipMemcpyDeviceToHost));
    return 0;
}

#include "plsa_init.hpp"      // factors onto a context and off it: host factors, device initialisation, the MT19937 stream

int plsa_set_arithmetic(plsa_ctx *c, int32_t mode) {
    if (mode & ~(PLSA_REFERENCE_SUMS | PLSA_REFERENCE_LL))
        return fail(c, "plsa_set_arithmetic: mode %d is not a combination of PLSA_REFERENCE_SUMS and PLSA_REFERENCE_LL", mode);
    c->ref_sums = (mode & PLSA_REFERENCE_SUMS) != 0;
    c->ref_ll = (mode & PLSA_REFERENCE_LL) != 0;
    return 0;
}

int plsa_e_step(plsa_ctx *c, float thresh, float *P_out) {
    HIPCHK(c, hipSetDevice(c->device));
    CHK(need_factors(c));
    CHK(run_e_step(c, thresh));
    if (P_out && c->nnz)
        HIPCHK(c, hipMemcpy2DAsync(P_out, sizeof(float) * c->k, p_base(c), sizeof(float) * c->kp,
                                   sizeof(float) * c->k, (size_t)c->nnz, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int plsa_set_p(plsa_ctx *c, const float *P) {
    HIPCHK(c, hipSetDevice(c->device));
    CHK(need_factors(c));
    if (c->P.borrowed || c->p_lent) {
        if (c->P.cap < sizeof(float) * (size_t)(c->nnz + 64) * c->kp)
            return fail(c, "plsa_set_p: the %s P(z|w,d) buffer is too small (it cannot be re-allocated while shared)", c->P.borrowed ? "borrowed" : "lent");
    } else
    CHK(ensure(c, c->P, sizeof(float) * (size_t)(c->nnz + 64) * c->kp + c->p_shift));
    if (c->kp != c->k) HIPCHK(c, hipMemsetAsync(p_base(c), 0, sizeof(float) * (size_t)c->nnz * c->kp, c->stream));
    if (c->nnz)
        HIPCHK(c, hipMemcpy2DAsync(p_base(c), sizeof(float) * c->kp, P, sizeof(float) * c->k,
                                   sizeof(float) * c->k, (size_t)c->nnz, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->p_state.valid = true;
    c->ref_tsum.invalidate();
    return 0;
}

int plsa_m_step(plsa_ctx *c, const float *sw, int32_t update_v, float *norm_pwz, float *norm_pdz) {
    const float *d_sw = nullptr;
    CHK(open_weighted(c, sw, &d_sw));
    CHK(ensure(c, c->norm_pdz, sizeof(float) * (size_t)c->n));
    CHK(run_m_step_from_p(c, d_sw, update_v != 0, c->norm_pdz.as<float>()));
    if (norm_pwz && update_v)
        HIPCHK(c, hipMemcpyAsync(norm_pwz, c->norm_pwz.p, sizeof(float) * (size_t)c->k, hipMemcpyDeviceToHost, c->stream));
    if (norm_pdz)
        HIPCHK(c, hipMemcpyAsync(norm_pdz, c->norm_pdz.p, sizeof(float) * (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int plsa_log_likelihood(plsa_ctx *c, const float *sw, double *ll) {
    const float *d_sw = nullptr;
    CHK(open_weighted(c, sw, &d_sw));
    return run_loglik(c, d_sw, ll);
}

// ---- doc-sharded single fit: local accumulate / (caller all-reduces) / finish -----------------------
int plsa_em_accumulate(plsa_ctx *c, const float *sw, float thresh, double *ll_partial) {
    HIPCHK(c, hipSetDevice(c->device));
    CHK(need_factors(c));
    if (c->ref_sums || c->ref_ll) return fail(c, "plsa_em_accumulate: the reference arithmetic (plsa_set_arithmetic) has no doc-sharded form");
    const float *d_sw = nullptr;
    CHK(upload_sw(c, sw, &d_sw));
    int blocks = 0;
    CHK(run_row_pass(c, false, ll_partial != nullptr, d_sw, thresh, nullptr, &blocks));
    CHK(run_col_pass(c, false, d_sw, thresh));
    if (ll_partial) CHK(finish_ll(c, blocks, ll_partial));    // (its scalar read-back is the only host wait)
    return 0;
}

// The reference's kernel SEQUENCE over the local rows (E-step into P(z|w,d), M-step from it) with the accumulate / finish
// split of the doc-sharded fit: what a doc-block TILE of block_parallel_plsa.py:373-403 does -- responsibilities of the block,
// partial factors of the block (:182-185) -- with the block's P(z|w,d) alive only inside this call.
int plsa_em_accumulate_materialised(plsa_ctx *c, const float *sw, float thresh, double *ll_partial) {
    HIPCHK(c, hipSetDevice(c->device));
    CHK(need_factors(c));
    if (c->ref_sums || c->ref_ll) return fail(c, "plsa_em_accumulate_materialised: the reference arithmetic (plsa_set_arithmetic) has no doc-block form");
    const float *d_sw = nullptr;
    CHK(upload_sw(c, sw, &d_sw));
    if (ll_partial) CHK(run_loglik(c, d_sw, ll_partial));       // log-likelihood of the CURRENT factors, local rows
    CHK(run_e_step(c, thresh));
    CHK(run_row_pass(c, true, false, nullptr, 0.f, nullptr, nullptr));
    CHK(run_col_pass(c, true, d_sw, 0.f));                      // partial sums + per-column sums into the accumulator
    // P(z|w,d) may be another context's by the next call (plsa_p_borrow): its last reader has finished when this returns
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream2));
    c->p_state.invalidate();
    return 0;
}

// P(z|w,d) capacity of this context: at least `bytes` (own allocation); *device_ptr = its address.
int plsa_p_reserve(plsa_ctx *c, int64_t bytes, void **device_ptr) {
    HIPCHK(c, hipSetDevice(c->device));
    if (bytes <= 0 || !device_ptr) return fail(c, "plsa_p_reserve: bad arguments");
    if (c->P.borrowed) return fail(c, "plsa_p_reserve: this context borrows its P(z|w,d) buffer");
    if (c->p_lent && c->P.cap < (size_t)bytes)
        return fail(c, "plsa_p_reserve: the buffer handed out earlier (%.2f GB) cannot grow to %.2f GB while other contexts may hold its "
                       "address: end the loans (plsa_p_borrow(NULL)) and call plsa_release_scratch first", c->P.cap / 1e9, bytes / 1e9);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    CHK(ensure(c, c->P, (size_t)bytes));
    c->p_lent = true;
    c->p_shift = 0;
    c->p_state.invalidate();
    *device_ptr = c->P.p;
    return 0;
}

// Use `device_ptr` (memory of the same device that outlives every later call on this context; e.g. another context's
// plsa_p_reserve) for P(z|w,d) instead of an allocation of one's own; NULL returns to own allocations.  Contexts that
// share a buffer must not run materialising calls concurrently.
int plsa_p_borrow(plsa_ctx *c, void *device_ptr, int64_t bytes) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->P.borrow(device_ptr, (size_t)std::max<int64_t>(bytes, 0));
    c->p_state.invalidate();
    c->p_shift = 0;
    return 0;
}

int plsa_set_sample_weight(plsa_ctx *c, const float *sw) {
    HIPCHK(c, hipSetDevice(c->device));
    c->sw_resident = false;
    if (!sw) return 0;
    if (c->n <= 0) return fail(c, "plsa_set_sample_weight: no matrix uploaded");
    CHK(ensure(c, c->sw_res, sizeof(float) * (size_t)c->n));
    HIPCHK(c, hipMemcpyAsync(c->sw_res.p, sw, sizeof(float) * (size_t)c->n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));          // `sw` may be freed on return
    c->sw_resident = true;
    c->sw_n = c->n;
    return 0;
}

int plsa_em_finish(plsa_ctx *c) {
    HIPCHK(c, hipSetDevice(c->device));
    CHK(need_factors(c));
    CHK(run_v_normalise(c));
    c->cu ^= 1; c->cv ^= 1;
    return 0;                       // stream-ordered: no host synchronisation (readers synchronise)
}

int plsa_accumulator_device(plsa_ctx *c, void **ptr, int64_t *n_floats) {
    CHK(need_factors(c));
    if (ptr) *ptr = c->Vacc.p;
    if (n_floats) *n_floats = c->m * c->kp;
    return 0;
}

int plsa_accumulator_get(plsa_ctx *c, float *host) {
    HIPCHK(c, hipSetDevice(c->device));
    CHK(need_factors(c));
    HIPCHK(c, hipMemcpyAsync(host, c->Vacc.p, sizeof(float) * (size_t)c->m * c->kp, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int plsa_accumulator_set(plsa_ctx *c, const float *host) {
    HIPCHK(c, hipSetDevice(c->device));
    CHK(need_factors(c));
    HIPCHK(c, hipMemcpyAsync(c->Vacc.p, host, sizeof(float) * (size_t)c->m * c->kp, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- multi-GPU exchange over RCCL (xGMI): one communicator per context ------------------------------
int plsa_comm_unique_id(void *id128) {
    if (!id128) return fail(nullptr, "plsa_comm_unique_id: NULL");
    static_assert(sizeof(ncclUniqueId) == PLSA_COMM_ID_BYTES, "RCCL unique id size");
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(nullptr, "ncclGetUniqueId: %s", ncclGetErrorString(r));
    memcpy(id128, &id, sizeof id);
    return 0;
}

int plsa_comm_init(plsa_ctx *c, const void *id128, int32_t rank, int32_t world) {
    HIPCHK(c, hipSetDevice(c->device));
    if (!id128 || world < 1 || rank < 0 || rank >= world) return fail(c, "plsa_comm_init: bad arguments");
    if (c->comm) return fail(c, "plsa_comm_init: this context already has a communicator");
    ncclUniqueId id;
    memcpy(&id, id128, sizeof id);
    NCCLCHK(c, ncclCommInitRank(&c->comm, world, id, rank));
    c->comm_rank = rank; c->comm_world = world;
    CHK(ensure(c, c->comm_small, 4096));
    return 0;
}

int plsa_comm_last_error(plsa_ctx *c, char *buf, int64_t cap) {
    if (!buf || cap <= 0) return 1;
    const char *msg = ncclGetLastError(c ? c->comm : nullptr);     // RCCL keeps one text per process; comm may be NULL
    snprintf(buf, (size_t)cap, "%s", msg ? msg : "");
    return 0;
}

int plsa_comm_destroy(plsa_ctx *c) {
    HIPCHK(c, hipSetDevice(c->device));
    if (c->comm) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream2));
        NCCLCHK(c, ncclCommDestroy(c->comm));
        c->comm = nullptr;
    }
    c->comm_rank = 0; c->comm_world = 1;
    return 0;
}

int plsa_comm_info(plsa_ctx *c, int32_t *rank, int32_t *world) {
    if (rank) *rank = c->comm_rank;
    if (world) *world = c->comm_world;
    return 0;
}

int plsa_comm_barrier(plsa_ctx *c) {
    HIPCHK(c, hipSetDevice(c->device));
    if (c->comm) {
        HIPCHK(c, hipMemsetAsync(c->comm_small.p, 0, sizeof(int), c->stream));
        NCCLCHK(c, ncclAllReduce(c->comm_small.p, c->comm_small.p, 1, ncclInt32, ncclSum, c->comm, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- member stack: the np.vstack of enstop_.py:231 without leaving the GPU ----------------------------
// The topic matrices of the ensemble members a process fits are kept in one device block [slots][k][m]
// (plsa_copy_components_to_device writes a slot -- from this context or from another context of the same
// device: members of a small corpus are fitted by several contexts at once).
int plsa_stack_reserve(plsa_ctx *c, int64_t slots, int64_t m, int32_t k, void **base_device) {
    HIPCHK(c, hipSetDevice(c->device));
    if (slots < 1 || m < 1 || k < 1 || !base_device) return fail(c, "plsa_stack_reserve: bad arguments");
    CHK(ensure(c, c->comm_stack, sizeof(float) * (size_t)slots * (size_t)k * (size_t)m));
    *base_device = c->comm_stack.p;
    return 0;
}

// One exchange for the whole ensemble: slot s of every rank is all-gathered into [s][rank] (all slots in ONE
// grouped RCCL launch), so the gathered block is the stack in RUN order -- run r was fitted by rank r % world
// in slot r / world (enstop_amd/enstop_.py) -- and goes to a page-locked host buffer in one copy.  Without a
// communicator (one process) it is the device stack itself.  *host: [slots * world][k][m], valid until the next
// call on this context.
// dst != nullptr: the gathered stack goes straight into the caller's host array (one pass; a fresh NumPy array costs its
// page faults exactly once, a re-used one nothing: 195 MB in 3.7 ms against 17 ms through the page-locked buffer plus a
// NumPy copy).  dst == nullptr: into the context's page-locked buffer, *host_view receives its address.
static int allgather_stack_impl(plsa_ctx *c, int64_t slots, int64_t m, int32_t k, float *dst, float **host_view) {
    HIPCHK(c, hipSetDevice(c->device));
    if (slots < 1 || m < 1 || k < 1 || (!dst && !host_view)) return fail(c, "plsa_comm_allgather_stack: bad arguments");
    const size_t km = (size_t)k * (size_t)m, world = (size_t)c->comm_world;
    if (c->comm_stack.cap < sizeof(float) * (size_t)slots * km)
        return fail(c, "plsa_comm_allgather_stack: no stack of %lld slots reserved (plsa_stack_reserve)", (long long)slots);
    const size_t bytes = sizeof(float) * (size_t)slots * km * world;
    if (!dst && c->comm_host_cap < bytes) {
        c->comm_host_cap = 0;
        HIPCHK(c, host_alloc(c->comm_host, bytes / sizeof(float)));
        c->comm_host_cap = bytes;
    }
    const float *src = c->comm_stack.as<float>();
    if (c->comm) {
        CHK(ensure(c, c->comm_recv, bytes));
        Scope s(c, "rccl_allgather_stack");
        NCCLCHK(c, ncclGroupStart());
        for (int64_t sl = 0; sl < slots; ++sl)
            NCCLCHK(c, ncclAllGather(c->comm_stack.as<float>() + (size_t)sl * km,
                                     c->comm_recv.as<float>() + (size_t)sl * world * km, km, ncclFloat, c->comm, c->stream));
        NCCLCHK(c, ncclGroupEnd());
        src = c->comm_recv.as<float>();
    }
    float *to = dst ? dst : c->comm_host.get();
    HIPCHK(c, hipMemcpyAsync(to, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (host_view) *host_view = to;
    return 0;
}

int plsa_comm_allgather_stack(plsa_ctx *c, int64_t slots, int64_t m, int32_t k, float **host) {
    return allgather_stack_impl(c, slots, m, k, nullptr, host);
}

int plsa_comm_allgather_stack_to(plsa_ctx *c, int64_t slots, int64_t m, int32_t k, float *dst) {
    if (!dst) return fail(c, "plsa_comm_allgather_stack_to: dst is NULL");
    return allgather_stack_impl(c, slots, m, k, dst, nullptr);
}

int plsa_comm_allgather_host(plsa_ctx *c, const void *send, int64_t bytes, void *recv) {
    HIPCHK(c, hipSetDevice(c->device));
    if (!send || !recv || bytes <= 0) return fail(c, "plsa_comm_allgather_host: bad arguments");
    if (!c->comm) { memmove(recv, send, (size_t)bytes); return 0; }
    CHK(ensure(c, c->comm_send, (size_t)bytes));
    CHK(ensure(c, c->comm_recv, (size_t)bytes * (size_t)c->comm_world));
    HIPCHK(c, hipMemcpyAsync(c->comm_send.p, send, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    NCCLCHK(c, ncclAllGather(c->comm_send.p, c->comm_recv.p, (size_t)bytes, ncclUint8, c->comm, c->stream));
    HIPCHK(c, hipMemcpyAsync(recv, c->comm_recv.p, (size_t)bytes * (size_t)c->comm_world, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int plsa_comm_allreduce_f64(plsa_ctx *c, double *inout, int64_t count, int32_t op) {
    HIPCHK(c, hipSetDevice(c->device));
    if (!inout || count <= 0 || (op != 0 && op != 1)) return fail(c, "plsa_comm_allreduce_f64: bad arguments");
    if (!c->comm) return 0;
    CHK(ensure(c, c->comm_send, sizeof(double) * (size_t)count));
    HIPCHK(c, hipMemcpyAsync(c->comm_send.p, inout, sizeof(double) * (size_t)count, hipMemcpyHostToDevice, c->stream));
    NCCLCHK(c, ncclAllReduce(c->comm_send.p, c->comm_send.p, (size_t)count, ncclDouble, op == 0 ? ncclSum : ncclMax,
                             c->comm, c->stream));
    HIPCHK(c, hipMemcpyAsync(inout, c->comm_send.p, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int plsa_comm_broadcast_host(plsa_ctx *c, void *buf, int64_t bytes, int32_t root) {
    HIPCHK(c, hipSetDevice(c->device));
    if (!buf || bytes <= 0 || root < 0 || root >= c->comm_world) return fail(c, "plsa_comm_broadcast_host: bad arguments");
    if (!c->comm) return 0;
    CHK(ensure(c, c->comm_send, (size_t)bytes));
    if (c->comm_rank == root)
        HIPCHK(c, hipMemcpyAsync(c->comm_send.p, buf, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    NCCLCHK(c, ncclBroadcast(c->comm_send.p, c->comm_send.p, (size_t)bytes, ncclUint8, root, c->comm, c->stream));
    HIPCHK(c, hipMemcpyAsync(buf, c->comm_send.p, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// in-place sum of the un-normalised P(w|z) accumulator over the communicator, enqueued on the context's
// stream (no host synchronisation): the exchange step between plsa_em_accumulate and plsa_em_finish
int plsa_allreduce_accumulator(plsa_ctx *c) {
    HIPCHK(c, hipSetDevice(c->device));
    CHK(need_factors(c));
    if (!c->comm) return 0;
    NCCLCHK(c, ncclAllReduce(c->Vacc.p, c->Vacc.p, (size_t)c->m * c->kp, ncclFloat, ncclSum, c->comm, c->stream));
    return 0;
}

int plsa_reference_chain_info(plsa_ctx *c, int64_t *slow_chunks, int64_t *chunks, int32_t *serial_now) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream2));
    if (c->ref_stats_pending) {
        c->ref_stats_pending = false;
        c->ref_slow_total += c->h_ref_stats[0]; c->ref_chunks_total += c->h_ref_stats[1];
        if (c->ref_chain_mode == 0 && c->h_ref_stats[1] > 0 && c->h_ref_stats[0] * 4 > c->h_ref_stats[1]) c->ref_pairs_off = true;
    }
    if (slow_chunks) *slow_chunks = (int64_t)c->ref_slow_total;
    if (chunks) *chunks = (int64_t)c->ref_chunks_total;
    if (serial_now) *serial_now = (c->ref_chain_mode == 2 || (c->ref_chain_mode == 0 && c->ref_pairs_off)) ? 1 : 0;
    return 0;
}

// include/plsa_hip_blocked.h
int plsa_set_p_budget(plsa_ctx *c, int64_t bytes) {
    if (bytes < 0) return fail(c, "plsa_set_p_budget: %lld bytes (0: no budget)", (long long)bytes);
    c->p_budget = bytes;
    return 0;
}

int plsa_p_block_info(plsa_ctx *c, int64_t *budget, int32_t *blocks, int64_t *largest_block_nnz, int64_t *p_allocated_bytes) {
    const plsa_ctx::PBlockInfo &pi = c->p_block_info;
    if (budget) *budget = pi.budget;
    if (blocks) *blocks = pi.blocks;
    if (largest_block_nnz) *largest_block_nnz = pi.largest;
    if (p_allocated_bytes) *p_allocated_bytes = pi.p_bytes;
    return 0;
}

int plsa_placement_info(plsa_ctx *c, int32_t *candidates, double *best_gbps, double *worst_gbps) {
    if (candidates) *candidates = c->placement_tried;
    if (best_gbps) *best_gbps = c->placement_gbps[0];
    if (worst_gbps) *worst_gbps = c->placement_gbps[1];
    return 0;
}

int plsa_schedule_info(plsa_ctx *c, int32_t *xcd_lo, double *xcd_end_us, int32_t *timed_launches, int32_t *item_len,
                       int64_t *n_items) {
    if (xcd_lo) for (int x = 0; x <= 8; ++x) xcd_lo[x] = c->csc.balanced ? c->bal_lo[x] : 0;
    if (xcd_end_us) for (int x = 0; x < 8; ++x) xcd_end_us[x] = c->bal_launches > 0 ? c->bal_end_us[x] : 0.0;
    if (timed_launches) *timed_launches = c->bal_launches;
    if (item_len) *item_len = c->csc.valid ? c->csc.seg : 0;
    if (n_items) *n_items = c->csc.valid ? c->csc.n_items : 0;
    return 0;
}

int plsa_packed_info(plsa_ctx *c, int32_t *csr, int32_t *csc) {
    if (csr) *csr = c->packed ? c->pk_csr.state() : 0;       // (PLSA_PACKED=0: the arrays, built or not)
    if (csc) *csc = c->packed ? c->pk_csc.state() : 0;
    return 0;
}

int plsa_pass_info(plsa_ctx *c, int32_t *col, int32_t *row, int32_t *wide) {
    if (c->k <= 0) return fail(c, "plsa_pass_info: factors not set (call plsa_set_factors)");
    if (col) { col[0] = c->lpn; col[1] = c->ch; col[2] = c->kp == 4 * c->lpn * c->ch; }
    if (row) { row[0] = c->row_lpn; row[1] = c->row_ch; row[2] = c->kp == 4 * c->row_lpn * c->row_ch; }
    // the tables each fused pass gathers from (dispatch_shape_row, run_col_pass): P(w|z), m rows; P(z|d), n rows
    if (wide) { wide[0] = table_is_wide(c, c->m); wide[1] = table_is_wide(c, c->n); }
    return 0;
}

int plsa_fit_info(plsa_ctx *c, int32_t *info) {
    if (!info) return fail(c, "plsa_fit_info: NULL argument");
    const plsa_ctx::FitInfo &f = c->fit_info;
    info[0] = f.fused; info[1] = f.pipelined; info[2] = f.speculated; info[3] = f.graph_launches;
    info[4] = f.tail; info[5] = f.two_stage; info[6] = f.xcd_split;
    return 0;
}

int plsa_release_scratch(plsa_ctx *c) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // a BORROWED P(z|w,d) stays borrowed (nothing of this context's own would be freed, and silently dropping the loan made
    // the next materialising call allocate a private full-size array); a LENT one is freed: the caller ends the loans first
    c->P.release();
    c->p_lent = false;
    c->p_state.drop();
    c->p_shift = 0;
    // derived structures kept only for the reference arithmetic / the fused passes: rebuilt on demand (the packed entry
    // streams by the next fused pass, from the CSC arrays, which stay)
    c->ref_heavy.drop(); c->ref_tsum.drop(); c->ref_blocks.drop(); c->pk_csr.drop(); c->pk_csc.drop();
    for (DevBuf *b : {&c->ref_terms, &c->ref_csum, &c->ref_pairs, &c->ref_exps, &c->ref_ll_neg, &c->ref_pairs2, &c->ref_exps2,
                      &c->partial, &c->tmp0, &c->tmp1, &c->tmp2, &c->cubtmp, &c->pk_count,
                      &c->mt_words, &c->mt_state, &c->mt_fin, &c->mt_poly, &c->mt_seq,
                      // member stack + gather buffers of the ensemble exchange (16 runs x 64 topics x 100 k words = 0.4 GB):
                      // re-created by the next plsa_stack_reserve / plsa_comm_allgather_stack
                      &c->comm_stack, &c->comm_recv, &c->comm_send, &c->metric_mask, &c->metric_small,
                      &c->score.indptr, &c->score.col, &c->score.val, &c->score.flag, &c->score.out,
                      &c->tempered.U, &c->tempered.Vt, &c->tempered.snapU, &c->tempered.snapVt,
                      &c->smoothed.norm_pdz, &c->smoothed.partials, &c->smoothed.out,
                      &c->lda.A, &c->lda.B, &c->lda.sums, &c->lda.norm_pdz, &c->lda.partials, &c->lda.out,
                      &c->lda_prior.alpha, &c->lda_prior.partials, &c->lda_prior.t})
        b->release();
    c->tempered.have_snap = false;
    c->smoothed.h_out.reset();           // (the stream is idle: nothing is on its way there)
    c->lda.h_out.reset();
    c->lda_prior.h.reset();
    c->lda_prior.h_kp = 0;
    c->lda.a_valid = c->lda.b_valid = false;
    // The page-locked landing buffer of plsa_comm_allgather_stack (c->comm_host) is NOT freed here: the caller may still
    // hold the pointer that call returned (a NumPy view in enstop_amd: gather_stack(view=True)); it lives until the next
    // gather that needs a larger one, or plsa_destroy.
    return 0;
}

int plsa_timing_enable(plsa_ctx *c, int32_t on) {
    if (!on) CHK(timing_flush(c));
    c->timing = on != 0;
    return 0;
}

int plsa_timing_reset(plsa_ctx *c) {
    CHK(timing_flush(c));
    std::fill(c->acc_ms.begin(), c->acc_ms.end(), 0.0);
    std::fill(c->acc_n.begin(), c->acc_n.end(), 0);
    return 0;
}

int plsa_timing_get(plsa_ctx *c, const char *prefix, double *total_ms, int64_t *launches) {
    CHK(timing_flush(c));
    double t = 0.0;
    i64 n = 0;
    const size_t pl = strlen(prefix);
    for (size_t i = 0; i < c->names.size(); ++i)
        if (c->names[i].compare(0, pl, prefix) == 0) { t += c->acc_ms[i]; n += c->acc_n[i]; }
    if (total_ms) *total_ms = t;
    if (launches) *launches = n;
    return 0;
}

int plsa_timing_report(plsa_ctx *c, char *buf, int64_t cap) {
    CHK(timing_flush(c));
    std::string s;
    char line[256];
    for (size_t i = 0; i < c->names.size(); ++i) {
        if (!c->acc_n[i]) continue;
        snprintf(line, sizeof line, "%s %lld %.6f\n", c->names[i].c_str(), (long long)c->acc_n[i], c->acc_ms[i]);
        s += line;
    }
    if (cap > 0) { strncpy(buf, s.c_str(), (size_t)cap - 1); buf[cap - 1] = 0; }
    return 0;
}

int plsa_measure_stream_bandwidth(plsa_ctx *c, int64_t bytes, int32_t kind, int32_t reps, double *gbps) {
    HIPCHK(c, hipSetDevice(c->device));
    if (bytes < (1 << 20) || reps < 1 || kind < 0 || kind > 6) return fail(c, "plsa_measure_stream_bandwidth: bad arguments");
    DevBuf a, b;
    const i64 n4 = bytes / 16;
    CHK(ensure(c, a, (size_t)n4 * 16));
    if (kind == 2) CHK(ensure(c, b, (size_t)n4 * 16));
    Event e0, e1;
    (void)hipEventCreate(&e0.h); (void)hipEventCreate(&e1.h);
    const int grid = grid_for(c, n4, 256);
    for (int r = -1; r < reps; ++r) {          // r == -1: untimed warm-up (page faults, clocks)
        if (r == 0) (void)hipEventRecord(e0, c->stream);
        if (kind == 0) hipLaunchKernelGGL((plsa::k_probe_fill<true>), dim3(grid), dim3(256), 0, c->stream, a.as<float>(), n4);
        else if (kind == 1) hipLaunchKernelGGL((plsa::k_probe_fill<false>), dim3(grid), dim3(256), 0, c->stream, a.as<float>(), n4);
        else if (kind >= 4) hipLaunchKernelGGL(plsa::k_probe_fill_tiled, dim3(grid_for(c, n4, 256 * (kind == 4 ? 16 : kind == 5 ? 4 : 64))), dim3(256), 0, c->stream, a.as<float>(), n4, kind == 4 ? 16 : kind == 5 ? 4 : 64);
        else if (kind == 3) hipLaunchKernelGGL(plsa::k_probe_read, dim3(grid), dim3(256), 0, c->stream, a.as<float>(), a.as<float>(), n4);
        else hipLaunchKernelGGL(plsa::k_probe_copy, dim3(grid), dim3(256), 0, c->stream, a.as<float>(), b.as<float>(), n4);
    }
    (void)hipEventRecord(e1, c->stream);
    hipError_t e = hipStreamSynchronize(c->stream);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    if (e != hipSuccess) return fail(c, "stream probe failed: %s", hipGetErrorString(e));
    const double moved = (double)n4 * 16.0 * (kind == 2 ? 2.0 : 1.0) * reps;
    *gbps = moved / 1e9 / (ms / 1e3);
    return 0;
}

// Synthetic corpus in HBM (see plsa_synth.hpp).  The mean token count per document is calibrated
// by a short secant iteration so that the number of DISTINCT (doc, word) pairs lands within 0.5 %
// of nnz_target; the final matrix depends only on the arguments.
static int generate_synthetic_impl(plsa_ctx *c, int64_t n, int64_t m, int64_t nnz_target, double zipf_s,
                                   uint64_t seed, int k0, double alpha, double background, int64_t *nnz_out) {
    HIPCHK(c, hipSetDevice(c->device));
    if (n <= 0 || m <= 1 || nnz_target < n || n >= INT32_MAX || m >= INT32_MAX)
        return fail(c, "plsa_generate_synthetic: bad arguments (need nnz_target >= n, m > 1)");
    if (k0 < 0 || k0 > 256 || (k0 > 0 && (!(alpha > 0.0) || background < 0.0 || background > 1.0)))
        return fail(c, "plsa_generate_synthetic_topics: need 1 <= k0 <= 256, alpha > 0, 0 <= background <= 1");
    // Zipf CDF over ranks (host, float64) and an affine permutation rank -> word id
    std::vector<double> cdf((size_t)m);
    double tot = 0.0;
    for (int64_t r = 0; r < m; ++r) { tot += std::pow((double)(r + 1), -zipf_s); cdf[(size_t)r] = tot; }
    for (int64_t r = 0; r < m; ++r) cdf[(size_t)r] /= tot;
    cdf[(size_t)m - 1] = 1.0;
    uint64_t a = (uint64_t)((double)m * 0.6180339887498949) | 1ull;
    auto gcd = [](uint64_t x, uint64_t y) { while (y) { uint64_t t = x % y; x = y; y = t; } return x; };
    while (gcd(a, (uint64_t)m) != 1) a += 2;
    const uint64_t b = plsa::mix64(seed ^ 0xABCDEFull) % (uint64_t)m;
    // topical corpus: one affine ranking per latent topic (odd multipliers spread by the hash, made coprime with m),
    // the shared ranking above in slot k0
    std::vector<uint64_t> perm;
    if (k0 > 0) {
        perm.resize(2 * (size_t)(k0 + 1));
        for (int t = 0; t < k0; ++t) {
            uint64_t at = (plsa::mix64(seed ^ plsa::mix64(0x70C1Cull + (uint64_t)t)) % (uint64_t)m) | 1ull;
            while (gcd(at, (uint64_t)m) != 1) at += 2;
            perm[2 * (size_t)t] = at % (uint64_t)m ? at % (uint64_t)m : 1;
            perm[2 * (size_t)t + 1] = plsa::mix64(seed ^ plsa::mix64(0xB0FF5E7ull + (uint64_t)t)) % (uint64_t)m;
        }
        perm[2 * (size_t)k0] = a; perm[2 * (size_t)k0 + 1] = b;
    }
    DevBuf d_cdf, d_tok, d_ptr, d_keys, d_keys2, d_flag, d_pos, d_perm;
#define SYNHIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(c, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)
    CHK(ensure(c, d_cdf, sizeof(double) * (size_t)m));
    SYNHIP(hipMemcpyAsync(d_cdf.p, cdf.data(), sizeof(double) * (size_t)m, hipMemcpyHostToDevice, c->stream));
    CHK(ensure(c, d_tok, sizeof(int) * (size_t)(n + 1)));
    CHK(ensure(c, d_ptr, sizeof(i64) * (size_t)(n + 1)));
    if (k0 > 0) {
        CHK(ensure(c, d_perm, sizeof(uint64_t) * perm.size()));
        SYNHIP(hipMemcpyAsync(d_perm.p, perm.data(), sizeof(uint64_t) * perm.size(), hipMemcpyHostToDevice, c->stream));
    }
    const double sigma = 0.6;
    double mean_tokens = 1.4 * (double)nnz_target / (double)n;
    i64 T = 0;
    int nnz = 0;
    const int dbits = plsa::plan::sort_bits(n);
    for (int round = 0; round < 8; ++round) {
        const double mu = std::log(mean_tokens) - 0.5 * sigma * sigma;
        hipLaunchKernelGGL(plsa::k_synth_doc_tokens, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, c->stream,
                           (int)n, mu, sigma, (int)std::min<i64>(m * 4, 1 << 20), seed, d_tok.as<int>());
        {
            auto in64 = hipcub::TransformInputIterator<i64, hipcub::CastOp<i64>, int *>(d_tok.as<int>(), hipcub::CastOp<i64>());
            auto scan = [&](void *tmp, size_t &bytes) {
                return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, in64, d_ptr.as<i64>(), (int)(n + 1), c->stream);
            };
            CHK(cub_two_phase(c, "hipcub::DeviceScan::ExclusiveSum", scan));
        }
        SYNHIP(hipMemcpyAsync(&T, d_ptr.as<i64>() + n, sizeof(i64), hipMemcpyDeviceToHost, c->stream));
        SYNHIP(hipStreamSynchronize(c->stream));
        if (T >= INT32_MAX) return fail(c, "plsa_generate_synthetic: %lld tokens >= 2^31", (long long)T);
        CHK(ensure(c, d_keys, sizeof(unsigned long long) * (size_t)T));
        CHK(ensure(c, d_keys2, sizeof(unsigned long long) * (size_t)T));
        CHK(ensure(c, d_flag, sizeof(int) * (size_t)T));
        CHK(ensure(c, d_pos, sizeof(int) * (size_t)T));
        if (k0 > 0)
            hipLaunchKernelGGL(plsa::k_synth_draw_topics, dim3(grid_for(c, n, 4)), dim3(256), 0, c->stream, (int)n, (int)m,
                               d_ptr.as<i64>(), d_cdf.as<double>(), d_perm.as<uint64_t>(), k0, alpha, background, seed,
                               d_keys.as<unsigned long long>());
        else
            hipLaunchKernelGGL(plsa::k_synth_draw, dim3(grid_for(c, n, 4)), dim3(256), 0, c->stream, (int)n, (int)m,
                               d_ptr.as<i64>(), d_cdf.as<double>(), a, b, seed, d_keys.as<unsigned long long>());
        {
            auto sort = [&](void *tmp, size_t &bytes) {
                return hipcub::DeviceRadixSort::SortKeys(tmp, bytes, d_keys.as<unsigned long long>(),
                                                         d_keys2.as<unsigned long long>(), T, 0, 32 + dbits, c->stream);
            };
            CHK(cub_two_phase(c, "hipcub::DeviceRadixSort::SortKeys", sort));
        }
        hipLaunchKernelGGL(plsa::k_synth_heads, dim3(grid_for(c, T, 256)), dim3(256), 0, c->stream,
                           d_keys2.as<unsigned long long>(), T, d_flag.as<int>());
        {
            auto scan = [&](void *tmp, size_t &bytes) {
                return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, d_flag.as<int>(), d_pos.as<int>(), (int)T, c->stream);
            };
            CHK(cub_two_phase(c, "hipcub::DeviceScan::ExclusiveSum", scan));
        }
        int last_pos = 0, last_flag = 0;
        SYNHIP(hipMemcpyAsync(&last_pos, d_pos.as<int>() + (T - 1), sizeof(int), hipMemcpyDeviceToHost, c->stream));
        SYNHIP(hipMemcpyAsync(&last_flag, d_flag.as<int>() + (T - 1), sizeof(int), hipMemcpyDeviceToHost, c->stream));
        SYNHIP(hipStreamSynchronize(c->stream));
        nnz = last_pos + last_flag;
        const double rel = ((double)nnz - (double)nnz_target) / (double)nnz_target;
        if (std::fabs(rel) < 0.005 || round == 7) break;
        // distinct pairs grow sub-linearly in tokens: damped multiplicative correction
        mean_tokens *= std::pow((double)nnz_target / (double)nnz, 1.25);
    }
    CHK(ensure(c, c->b_indptr, sizeof(int) * (size_t)(n + 1)));
    CHK(ensure(c, c->b_col, sizeof(int) * (size_t)nnz));
    CHK(ensure(c, c->b_val, sizeof(float) * (size_t)nnz));
    hipLaunchKernelGGL(plsa::k_synth_emit, dim3(grid_for(c, T, 256)), dim3(256), 0, c->stream,
                       d_keys2.as<unsigned long long>(), T, d_flag.as<int>(), d_pos.as<int>(), (int)n, nnz,
                       c->b_indptr.as<int>(), c->b_col.as<int>(), c->b_val.as<float>());
    CHK(launch_check(c, "k_synth_emit"));
    SYNHIP(hipStreamSynchronize(c->stream));
#undef SYNHIP
    c->bn = n; c->bm = m; c->bnnz = nnz;
    c->active_is_base = true;
    set_active_pointers(c);
    c->syn_n = k0 > 0 ? n : 0; c->syn_k0 = k0; c->syn_alpha = alpha; c->syn_seed = seed;
    if (nnz_out) *nnz_out = nnz;
    return 0;
}

int plsa_synthetic_dominant_topics(plsa_ctx *c, int32_t *out /*[n] host*/) {
    HIPCHK(c, hipSetDevice(c->device));
    if (c->syn_n <= 0 || c->syn_n != c->bn) return fail(c, "plsa_synthetic_dominant_topics: the base corpus is not a topical synthetic corpus");
    if (!out) return fail(c, "plsa_synthetic_dominant_topics: out is NULL");
    CHK(ensure(c, c->tmp1, sizeof(int) * (size_t)c->syn_n));
    hipLaunchKernelGGL(plsa::k_synth_dominant_topic, dim3((unsigned)((c->syn_n + 255) / 256)), dim3(256), 0, c->stream,
                       (int)c->syn_n, c->syn_k0, c->syn_alpha, c->syn_seed, c->tmp1.as<int>());
    CHK(launch_check(c, "k_synth_dominant_topic"));
    HIPCHK(c, hipMemcpyAsync(out, c->tmp1.p, sizeof(int) * (size_t)c->syn_n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int plsa_generate_synthetic(plsa_ctx *c, int64_t n, int64_t m, int64_t nnz_target, double zipf_s,
                            uint64_t seed, int64_t *nnz_out) {
    return generate_synthetic_impl(c, n, m, nnz_target, zipf_s, seed, 0, 0.0, 0.0, nnz_out);
}

int plsa_generate_synthetic_topics(plsa_ctx *c, int64_t n, int64_t m, int64_t nnz_target, double zipf_s,
                                   uint64_t seed, int32_t k0, double alpha, double background, int64_t *nnz_out) {
    if (k0 < 1) return fail(c, "plsa_generate_synthetic_topics: need 1 <= k0 <= 256");
    return generate_synthetic_impl(c, n, m, nnz_target, zipf_s, seed, k0, alpha, background, nnz_out);
}

}  // extern "C"

#include "plsa_drivers.hpp"   // plsa_fit, plsa_refit: the call frame of the fit entry points, backends of the loop (plsa_fit_schedule.hpp)
#include "plsa_members.hpp"   // batched ensemble members (include/plsa_hip_members.h)
#include "plsa_nmf.hpp"       // KL-divergence NMF (include/plsa_hip_nmf.h)
#include "plsa_score_kernels.hpp"   // held-out scoring (include/plsa_hip_score.h): the document-owned pass ...
#include "plsa_score.hpp"           // ... and its host side
#include "plsa_tempered_kernels.hpp"   // tempered EM (include/plsa_hip_tempered.h): the power of a factor table ...
#include "plsa_tempered.hpp"           // ... and the loop, the snapshot slot and the diagnostic read-back
#include "plsa_online_kernels.hpp"     // online (stepwise) EM (include/plsa_hip_online.h): the blend of the statistic ...
#include "plsa_online.hpp"             // ... and the state, the step and the fold
#include "plsa_smoothed_kernels.hpp"   // smoothed (MAP) EM (plsa_hip_diag.h): pseudo-counts behind the passes, the log prior ...
#include "plsa_smoothed.hpp"           // ... and the two loops and the objective
#include "plsa_lda_kernels.hpp"        // variational Bayes LDA (plsa_hip_diag.h): exp-digamma tables, priors behind the passes, the bound ...
#include "plsa_lda.hpp"                // ... and the two loops, the bound and the diagnostic read-back
#include "plsa_lda_prior_math.hpp"     // LDA's vector and learned priors (plsa_hip_lda_priors.h): trigamma and the two Newton maximisers ...
#include "plsa_lda_prior_kernels.hpp"  // ... the sums a prior update needs, the vector forms of two kernels ...
#include "plsa_lda_priors.hpp"         // ... and the loop with its prior updates, the refit, the bound and the sums
#include "plsa_lda_online_kernels.hpp" // online LDA (plsa_hip_lda_online.h): the blend of the counts into lambda with its slab sums ...
#include "plsa_lda_online.hpp"         // ... and the state, the step and the fold
#include "plsa_combine_kernels.hpp"    // topic combination: all-pairs Hellinger and KL, cluster representatives ...
#include "plsa_combine.hpp"            // ... and the six entry points, with the coherence counts and the embedding (their kernel headers)
