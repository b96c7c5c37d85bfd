/* pda_hip_det.h -- the bit-reproducible training path (`--deterministic 1`) on libpda_hip.so.
 *
 * Same conventions as pda_hip.h: device pointers, caller-owned buffers, an explicit `void* stream` (hipStream_t), int return codes
 * (PDA_OK / PDA_ERR_*), every argument check before anything is launched, no host synchronisation and no allocation (the calls can
 * be captured in a single-stream HIP graph).  Kept in its own header, like pda_hip_temp_pop.h and pda_hip_pc.h.
 *
 * Contract ("Deterministic training"): every result below is a function of its arguments' CONTENTS alone -- not of
 * timing, of the number of free CUs, of other work on the GPU or of the cache policy.  No float atomic is issued on these paths:
 * sums over the references of a row run in the order of the batch's plan (pda_triplet_plan for B <= 4096, pda_triplet_plan_large
 * above; pda_hip_experimental.h), the long and very long segments in the fixed combination order of pda_bpr_step_plan_f32.
 */
#ifndef PDA_HIP_DET_H
#define PDA_HIP_DET_H

#include "pda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The summed gradient of a batch with DISTINCT users, two launches -- a drop-in for pda_bpr_step_f32 in PDA_UPD_DENSE_GRAD mode.
 *   gU[user]  = the triplet's user gradient, L2 term included                                  (plain stores; one writer per row)
 *   gI[row]   = sum over the row's references, in plan order, of coefficient x user row, + (regs / reg_div) count row
 *   tagU[user] = tagI[row] = step_tag   (tagU and tagI may both be NULL: callers that do not sweep by tag)
 *   loss_acc f32 [3] (or NULL) += (loss, mf_loss, reg_loss): per-workgroup partial sums added in a fixed order, then one plain add
 * Rows outside the batch are not written: like pda_adam_step_f32, a sweep behind this call wants gU / gI zero off the rows of the
 * running step.  plan: the batch's plan (pda_triplet_plan_bytes(B) bytes); scratch: pda_bpr_grad_plan_scratch_bytes(B, d) bytes.
 * A batch the plan rejects (a user occurs twice): loss_acc receives NaN, nothing else is written.
 * d in {32, 64, 128, 256}, else PDA_ERR_UNSUPPORTED.  U, I are read only. */
/* Buffer contract -- scratch (pda_bpr_grad_plan_scratch_bytes): needs no initialisation -- the first launch writes what the second reads; nothing in it
 * is meant for the caller afterwards; one scratch buffer serves one call at a time. */
size_t pda_bpr_grad_plan_scratch_bytes(int B, int d);
int pda_bpr_grad_plan_f32(const float* U, const float* I, const int32_t* users, const int32_t* pos, const int32_t* neg,
                          const float* pos_pop, const float* neg_pop, int B, int d, float regs, float reg_div, const void* plan,
                          float* scratch, float* gU, int32_t* tagU, float* gI, int32_t* tagI, int step_tag, float* loss_acc, void* stream);

/* One reference train step (gradients + TF-1.14 dense-decay Adam over both tables), bit-reproducible: the planned gradient above,
 * then the tagged sweep of pda_adam_step_f32 (element for element the same arithmetic; it is order-free).  Three launches.  The
 * arguments of pda_adam_step_f32 minus `flags`, plus `plan` and `scratch`.  A rejected batch: loss_acc receives NaN; tables, moments,
 * gU, gI and the tags stay as they are (the sweep is skipped on the device). */
int pda_adam_step_plan_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI,
                           float* gI, int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg,
                           const float* pos_pop, const float* neg_pop, int B, int d, float regs, float reg_div, int step_tag, float lr_t,
                           float beta1, float beta2, float eps, int cache_policy, const void* plan, float* scratch, float* loss_acc,
                           void* stream);

/* pda_metrics with an ordered reduction: the same four metrics in the same layout of `sums` (f64 [4][n_ks], added to), but every
 * wave's partial sums go to `workspace` (pda_metrics_ordered_workspace_bytes(n_rows, n_ks) bytes, 8-byte aligned) and a second launch adds
 * them in a fixed order.  Calls that share `sums` must share a stream (the final add is a plain read-modify-write). */
/* Buffer contract -- workspace (pda_metrics_ordered_workspace_bytes): needs no initialisation -- every partial sum is written by its wave before the
 * second launch adds them; nothing in it is meant for the caller afterwards; one workspace serves one call at a time. */
size_t pda_metrics_ordered_workspace_bytes(int n_rows, int n_ks);
int pda_metrics_ordered(const int32_t* topk, int n_rows, int k_cols, const int64_t* tgt_indptr, const int32_t* tgt_indices,
                        const int32_t* Ks, int n_ks, double* sums, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_DET_H */
