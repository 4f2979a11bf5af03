/*
 * plsa_hip_blocked.h -- memory plumbing of libplsa_hip.so: the reference arithmetic in bounded memory.
 *
 * The reference arithmetic (PLSA_REFERENCE_SUMS, plsa_set_arithmetic) evaluates the reference's M-step from a stored
 * P(z|w,d), one row of kp floats per non-zero.  None of its sums needs the whole array at once: every chain runs over the
 * non-zeros in document-major order, so with the corpus cut at document boundaries a sum is either complete inside one
 * block (a document's P(z|d) row and norm) or a chain that is handed from one block to the next (a word's P(w|z) column
 * accumulator, norm_pwz).  The carried value is where the next block's accumulator starts: the same additions in the same
 * order, bit for bit the result of the unblocked step.
 *
 * Same conventions as plsa_hip.h: status codes, plsa_last_error(ctx), not thread-safe.
 */
#ifndef PLSA_HIP_BLOCKED_H
#define PLSA_HIP_BLOCKED_H

#include "plsa_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes that P(z|w,d) may take in plsa_fit and plsa_refit while the reference sums are in force (PLSA_REFERENCE_SUMS in
 * `flags`, or plsa_set_arithmetic).  0 (the default): no budget, one array for all non-zeros.
 *   The active matrix' documents are cut greedily, in order, into blocks of whole documents with
 * (block_nnz + 64) * kp * 4 <= bytes; P(z|w,d) is allocated for the largest block and every EM iteration walks the blocks.
 * A plan of one block runs exactly what runs without a budget.  A document whose own rows exceed the budget is a status
 * code (the message names its non-zeros and the bytes it needs), and so is a budget on a context whose P(z|w,d) buffer is
 * borrowed or lent out (plsa_p_borrow / plsa_p_reserve).
 *   Nothing else consults the budget: the default arithmetic never stores P(z|w,d) in its fused schedule, and the
 * kernel-level plsa_e_step / plsa_m_step / plsa_set_p hand the whole array in or out.  PLSA_SHARDED stays refused in the
 * reference arithmetic. */
int plsa_set_p_budget(plsa_ctx *ctx, int64_t bytes);

/* Of the last reference-arithmetic iteration of plsa_fit / plsa_refit: the budget in force, the blocks it ran in (1: not
 * blocked), the non-zeros of the largest block, and the bytes allocated for P(z|w,d).  Any pointer may be NULL. */
int plsa_p_block_info(plsa_ctx *ctx, int64_t *budget, int32_t *blocks, int64_t *largest_block_nnz,
                      int64_t *p_allocated_bytes);

#ifdef __cplusplus
}
#endif
#endif
