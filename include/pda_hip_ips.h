/* pda_hip_ips.h -- inverse propensity scoring on the BPR loss (`--train ips`: IPS, IPS-C, IPS-CN) on libpda_hip.so.
 *
 * Same conventions as pda_hip.h: device pointers, an explicit `void* stream` (hipStream_t), int return codes (PDA_OK / PDA_ERR_*), and every
 * argument check happens before anything is launched.  Kept in its own header, like pda_hip_temp_pop.h and pda_hip_dice.h.
 *
 * Model: the tables of a BPRMF, U f32 [n_users, d], I f32 [n_items, d]; an IPS model differs from a BPRMF only in how it was
 * trained, and every evaluation entry point of pda_hip.h serves it unchanged (PDA_HEAD_RAW).  ipw f32 [n_items]: the weight of an item as a
 * positive, built once per data set on the host (pda_amd.ops.IpsWeights): with n_i the train interactions of item i,
 *     p_i = max(n_i, 1) / max_j n_j  (float64)        w_i = 1 / p_i        clip C > 0: w_i = min(w_i, C)        ipw[i] = (float)w_i
 * Per batch of B triplets (u, p, n): x_t = u.p - u.n (the raw dots: no ELU, no popularity head), ls(x) = log(sigmoid(x) + 1e-10),
 * w_t = ipw[p_t]:
 *     wsum == NULL:  mf = -(1 / B) sum_t w_t ls(x_t)                                              (IPS, IPS-C)
 *     wsum != NULL:  mf = -(1 / S) sum_t w_t ls(x_t),   S = *wsum = sum_t w_t                     (IPS-CN: self-normalised over the batch)
 *     reg  = regs (l2(u) + l2(p) + l2(n)) / reg_div                                               (unweighted: the term of pda_bpr_step_f32)
 *     loss = mf + reg
 * A triplet with an id outside the tables is skipped: it adds nothing to the loss, to the gradients or to S (memory safety only: the callers
 * validate their ids).  d in {32, 64, 128, 256}.
 */
#ifndef PDA_HIP_IPS_H
#define PDA_HIP_IPS_H

#include "pda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* *wsum = S, the sum of ipw[pos[t]] over the batch's valid triplets: one launch of ONE workgroup.  Every thread sums its triplets
 * t = tid, tid + 1024, ... in that order in float64, the workgroup adds its partial sums in a fixed tree, and the result is rounded to fp32 once:
 * the same bits run after run, and within one ulp of the exact sum.  An empty sum stores 0. */
int pda_ips_weight_sum(const float* ipw, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg, int B,
                       float* wsum, void* stream);

/* The batch's gradients (one launch, the layout of pda_bpr_step_f32: d / 4 lanes per triplet).  The coefficient of d loss / dx and the triplet's
 * log term are scaled by w_t / B (wsum == NULL) or by w_t / *wsum (wsum != NULL: read from device memory by the kernel, no host read; *wsum <= 0
 * scales by 0).  The gradients are SUMMED into gU [n_users, d] / gI [n_items, d] (duplicates add up; equal positives inside a workgroup are
 * combined on chip first); the rows touched get tagU[user] = tagI[pos] = tagI[neg] = step_tag, exactly as pda_adam_step_f32 tags them.
 * flags: PDA_UPD_ANY_ORDER (the batch is not grouped by positive) | PDA_UPD_USERS_DISTINCT (no user id occurs twice: its gU row, zero before the
 * call, takes a plain store).  loss_acc (optional) f32 [3] += (loss, mf, reg).
 * PRECONDITION of PDA_UPD_USERS_DISTINCT, as for pda_adam_step_f32 (pda_hip.h): the plain store is the row's gradient only if gU is zero on every
 * row the batch touches and no user occurs twice.  The sweep of pda_ips_adam_step_f32 zeroes what the step wrote; a non-OK return between the
 * step and the sweep leaves gU / gI and the tags dirty, and the caller zeroes them before going on. */
int pda_ips_step_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg,
                     const float* ipw, const float* wsum, int B, int d, float regs, float reg_div, float* gU, float* gI, int32_t* tagU,
                     int32_t* tagI, int step_tag, int flags, float* loss_acc, void* stream);

/* One train step: pda_ips_weight_sum into wsum_ws when it is given (NULL: the 1 / B forms), pda_ips_step_f32, then TF-1.14's dense-decay Adam
 * over both tables by pda_adam_dense_sweep4_f32 (the sweep of pda_adam_step_f32: g = 0 off the tagged rows, g zeroed behind itself).  Two or three
 * launches, no host read: capturable in a HIP graph.  wsum_ws: one float of device memory private to the stream.  flags and cache_policy: those
 * of pda_adam_step_f32. */
/* Buffer contract -- wsum_ws (one float, or NULL: no self-normalisation): needs no initialisation -- the call writes it (pda_ips_weight_sum) before its
 * step reads it; afterwards a caller may read it (the batch's S); one wsum_ws serves one call at a time. */
int pda_ips_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI, float* gI,
                          int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg, const float* ipw,
                          float* wsum_ws, int B, int d, float regs, float reg_div, int step_tag, float lr_t, float beta1, float beta2, float eps,
                          int flags, int cache_policy, float* loss_acc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_IPS_H */
