/* pda_hip_temp_pop.h -- BPRMF(t)-pop (the temporal-popularity baseline, `--train temp_pop`) on libpda_hip.so.
 *
 * Same conventions as pda_hip.h: device pointers, an explicit `void* stream` (hipStream_t), int return codes (PDA_OK / PDA_ERR_*), and every
 * argument check happens before anything is launched.  Kept in its own header: the stable header's symbol budget is spent, and the experimental
 * header holds the entry points beyond the drop-in surface of PD / PDA and BPRMF.
 *
 * Model ("BPRMF(t)-pop"): tables U f32 [n_users, d], I f32 [n_items, d], bu f32 [n_users] (the user bias, one column), C f32
 * [n_items, T + 1] (column t < T: the item bias of time slot t, column T: the "init" bias).  Per triplet (u, p, n, t):
 *     ub = b~_u + 1,  b~_u = bu[u] if t == 0 else 0        (the reference's out-of-range gather_nd: see DESIGN.md, quirk 1)
 *     s_p = ub (C[p, T] + C[p, t]) + u . i_p,  s_n the same with n
 *     loss = -mean(log(sigmoid(s_p - s_n) + 1e-10)) + regs (l2(u) + l2(i_p) + l2(i_n)) / reg_div    (the bias tables are not regularised)
 */
#ifndef PDA_HIP_TEMP_POP_H
#define PDA_HIP_TEMP_POP_H

#include "pda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PDA_HEAD_BIAS 2 /* temp_pop 'main_branch': top_k(fl(R + fl(alpha_u beta_i)) + M) -- the heads of pda_hip.h are 0 and 1 */

/* One training step's gradients (one launch).  temps f32 [B]: the time slot of each triplet's positive as a float (the reference feeds it
 * through a float placeholder and casts it to int; a slot outside [0, T) is clamped into it -- callers validate slots when they load data).
 * The batch's gradients are SUMMED into gU [n_users, d], gI [n_items, d], gbu [n_users], gC [n_items, T + 1] (duplicates add up), and the rows
 * touched are tagged: tagU[user] = step_tag (covers U and bu), tagI[pos] = tagI[neg] = step_tag (covers I and C).  loss_acc (optional)
 * f32 [3] += (loss, mf_loss, reg_loss).  d in {32, 64, 128, 256}; T >= 1. */
int pda_temp_pop_step_f32(const float* U, const float* I, const float* bu, const float* C, const int32_t* users, const int32_t* pos,
                          const int32_t* neg, const float* temps, int B, int d, int T, float regs, float reg_div, float* gU, float* gI, float* gbu,
                          float* gC, int32_t* tagU, int32_t* tagI, int step_tag, float* loss_acc, void* stream);

/* TF-1.14 dense-decay Adam over the four tables in one launch: per element the arithmetic of pda_adam_dense_sweep_f32, with g = 0 off the rows
 * tagged step_tag; g is zeroed behind itself on the tagged rows. */
int pda_temp_pop_sweep_f32(float* U, float* mU, float* vU, float* gU, const int32_t* tagU, size_t n_users, float* I, float* mI, float* vI, float* gI,
                           const int32_t* tagI, size_t n_items, float* bu, float* mbu, float* vbu, float* gbu, float* C, float* mC, float* vC,
                           float* gC, int d, int T, int step_tag, float lr_t, float beta1, float beta2, float eps, void* stream);

/* One reference train step (gradients + Adam over all four tables) in two launches: pda_temp_pop_step_f32 then pda_temp_pop_sweep_f32. */
int pda_temp_pop_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI, float* gI,
                               int32_t* tagI, size_t n_items, float* bu, float* mbu, float* vbu, float* gbu, float* C, float* mC, float* vC, float* gC,
                               const int32_t* users, const int32_t* pos, const int32_t* neg, const float* temps, int B, int d, int T, float regs,
                               float reg_div, int step_tag, float lr_t, float beta1, float beta2, float eps, float* loss_acc, void* stream);

/* Score + history mask + top-K with the bias head h = fl(s + fl(alpha_u beta_i)), s the exact fp32 chain of pda_score_topk_f32:
 *   alpha f32 [n_users_blk] per block row, beta f32 [n_items_local] per local item row; everything else as pda_score_topk_f32 (out_keys
 *   int64 [n_splits, n_users_blk, K], merged by pda_topk_merge).  workspace: pda_temp_pop_score_workspace_bytes(n_users_blk) bytes, 16-byte
 *   aligned.  d in {64, 128, 256}; K <= PDA_TOPK_CAP - 1.
 *   Two kernels, the same keys: with prep (pda_item_prep_f32 of I_shard) the pre-filtered one (generation 3: a bf16 MFMA filter whose bound
 *   covers the bias head, a candidate ring, exact fp32 rescoring) wherever it can run (K <= PDA_TOPK_CAP - 4, item ids below 2^27); the exact
 *   one (generation 1, fp32 MFMA) otherwise.  PDA_TEMP_POP_KERNEL=exact | prefiltered forces one.  The kernel writes its identity word at
 *   workspace + 16: generation << 28 | 1 << 15 (bias head) | d / 64. */
/* Buffer contract -- workspace (pda_temp_pop_score_workspace_bytes): needs no initialisation -- every word the call reads it wrote before (the pre-
 * filtered kernel's call clears the whole workspace, stream-ordered; the exact kernel's copies alpha to +64 and writes the identity word); afterwards a
 * caller may read +16 (kernel identity); one workspace serves one call at a time. */
size_t pda_temp_pop_score_workspace_bytes(int n_users_blk);
int pda_temp_pop_score_topk_f32(const float* U, const float* I_shard, const void* prep, const float* alpha, const float* beta, const int32_t* users,
                                int n_users_blk, int item_offset, int n_items_local, int d, const int64_t* hist_indptr, const int32_t* hist_indices,
                                int hist_row_mode, int K, int n_splits, uint64_t* out_keys, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_TEMP_POP_H */
