/* pda_hip_ssm.h -- the sampled-softmax loss (`--train ssm`: SSM, Wu et al., "On the Effectiveness of Sampled Softmax Loss for Item
 * Recommendation") on libpda_hip.so.
 *
 * Same conventions as pda_hip.h: device pointers, an explicit `void* stream` (hipStream_t), int return codes (PDA_OK / PDA_ERR_*), and every
 * argument check happens before anything is launched.  Kept in its own header, like pda_hip_ips.h.
 *
 * Model: the tables of a BPRMF, U f32 [n_users, d], I f32 [n_items, d], d in {32, 64, 128, 256}.
 * Batch: users i32 [B], pos i32 [B], negs i32 [B, N] row-major, 1 <= N <= PDA_SSM_MAX_NEGS.
 * Logits of row r, with i_0 = I[pos[r]], i_k = I[negs[r, k - 1]] (k = 1 .. N), u = U[users[r]]:
 *     norm == 0:  s_k = (u . i_k) / tau
 *     norm == 1:  s_k = (u^ . i^_k) / tau,   x^ = x / max(|x|, 1e-12),  |x| = sqrt(sum x^2)
 * Loss:
 *     lse  = m + log(sum_{k = 0 .. N} exp(s_k - m)),  m = max_k s_k
 *     l_r  = lse - s_0                                 (a log-softmax: no + 1e-10)
 *     mf   = (1 / B) sum_r l_r
 *     reg  = regs (l2(u) + l2(i_0) + sum_{k >= 1} l2(i_k)) / reg_div     (l2 = 0.5 sum x^2, the term of pda_bpr_step_f32; every OCCURRENCE counts)
 *     loss = mf + reg
 * Gradients: the derivative of the above.  With p_k = exp(s_k - lse), c_0 = (p_0 - 1) / (tau B), c_k = p_k / (tau B), c_reg = regs / reg_div:
 *     norm == 0:  gU[u] += sum_k c_k i_k + c_reg u                      gI[i_k] += c_k u + c_reg i_k          (once per occurrence)
 *     norm == 1:  g_u^ = sum_k c_k i^_k
 *                 gU[u] += (g_u^ - (u^ . g_u^) u^) / max(|u|, 1e-12) + c_reg u
 *                 gI[i_k] += c_k (u^ - (u^ . i^_k) i^_k) / max(|i_k|, 1e-12) + c_reg i_k
 *     (a row whose norm is below 1e-12 takes these very expressions: finite numbers, nothing more is promised).
 * Validity: a row is skipped WHOLE when one of its N + 2 ids lies outside the tables -- it adds nothing to the loss, the gradients or the tags
 * (memory safety only: the callers validate their ids); B divides the mean regardless.  Duplicate negatives inside a row add up, and so does a
 * negative that equals the row's positive (the sampler excludes train items only).
 */
#ifndef PDA_HIP_SSM_H
#define PDA_HIP_SSM_H

#include "pda_hip.h"

#define PDA_SSM_MAX_NEGS 256

#ifdef __cplusplus
extern "C" {
#endif

/* The batch's gradients: ONE launch, d / 4 lanes per row, two passes over the row's N + 1 item rows (the logits never leave the chip).  The
 * gradients are SUMMED into gU [n_users, d] / gI [n_items, d] (equal positives inside a workgroup are combined on chip first, the negatives
 * take float atomics); the rows touched get tagU[user] = tagI[pos] = tagI[neg_k] = step_tag, exactly as pda_adam_step_f32 tags them.
 * flags: PDA_UPD_ANY_ORDER (the batch is not grouped by positive) | PDA_UPD_USERS_DISTINCT (no user id occurs twice: its gU row, zero before the
 * call, takes a plain store).  loss_acc (optional) f32 [3] += (loss, mf, reg).
 * PRECONDITION of PDA_UPD_USERS_DISTINCT, as for pda_adam_step_f32 (pda_hip.h): the plain store is the row's gradient only if gU is zero on every
 * row the batch touches and no user occurs twice.  The sweep of pda_ssm_adam_step_f32 zeroes what the step wrote; a non-OK return between the
 * step and the sweep leaves gU / gI and the tags dirty, and the caller zeroes them before going on.
 * PDA_ERR_ARG: a null pointer (loss_acc aside), B outside 1 .. 2^28, N outside 1 .. PDA_SSM_MAX_NEGS, tau <= 0 or not finite, norm outside
 * {0, 1}, reg_div <= 0, step_tag <= 0, other flags.  PDA_ERR_UNSUPPORTED: d. */
int pda_ssm_step_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* negs,
                     int B, int N, int d, float tau, int norm, float regs, float reg_div, float* gU, float* gI, int32_t* tagU, int32_t* tagI,
                     int step_tag, int flags, float* loss_acc, void* stream);

/* One train step: pda_ssm_step_f32, then TF-1.14's dense-decay Adam over both tables by pda_adam_dense_sweep4_f32 (the sweep of
 * pda_adam_step_f32: g = 0 off the tagged rows, g zeroed behind itself).  Two launches, no host read: capturable in a HIP graph.  flags and
 * cache_policy: those of pda_adam_step_f32. */
int pda_ssm_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI, float* gI,
                          int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* negs, int B, int N, int d,
                          float tau, int norm, float regs, float reg_div, int step_tag, float lr_t, float beta1, float beta2, float eps, int flags,
                          int cache_policy, float* loss_acc, void* stream);

/* The sampler: users and positives are those of pda_sample_triplets for the same (seed, step, row) -- gen_users, user_pool and neg_lo / neg_hi
 * included; no time slots, no popularity columns.  Negative j (0 <= j < N) of row r, attempt a (0 <= a < 4096), is
 *     neg_lo + bounded(draw(seed, step, r, 16 + 4096 j + a), neg_hi - neg_lo)
 * rejected while it is a train item of the user (binary search in the sorted row); after 4096 attempts the last draw stays.  Column 0 is, bit for
 * bit, the negative of pda_sample_triplets, and N = 1 reproduces its batch stream.  One thread per (row, j).  negs i32 [B, N]; B <= 2^22. */
int pda_ssm_sample(int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, int N, const int64_t* train_indptr,
                   const int32_t* train_indices, int neg_lo, int neg_hi, uint64_t seed, uint64_t step, int32_t* pos, int32_t* negs, void* stream);

/* The same with the step taken from DEVICE memory (*step_dev) and, where step_next is given (a DIFFERENT location), *step_dev + 1 stored there:
 * the protocol of pda_sample_triplets_dev. */
int pda_ssm_sample_dev(int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, int N, const int64_t* train_indptr,
                       const int32_t* train_indices, int neg_lo, int neg_hi, uint64_t seed, const uint64_t* step_dev, uint64_t* step_next,
                       int32_t* pos, int32_t* negs, void* stream);

/* Y[r] = X[r] / max(|X[r]|, 1e-12) for the n_rows rows of X f32 [n_rows, d]: the evaluation tables of a norm == 1 model.  The sum of squares is
 * taken in float64 in a fixed order -- lane e of the row's d / 4 lanes adds the squares of elements 4 e .. 4 e + 3 in that order (each product
 * exact in float64), the lanes add by the xor ladder (offsets d / 8, d / 16, .. 1) --, the square root and the quotient are float64 and every
 * element is rounded to float32 once: the same bits run after run.  Y may be X. */
int pda_ssm_normalize_rows_f32(const float* X, size_t n_rows, int d, float* Y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_SSM_H */
