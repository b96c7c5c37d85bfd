/* pda_hip_pcc.h -- the popularity-correlation regulariser on the BPR loss (`--train pcc`) on libpda_hip.so.
 *
 * Same conventions as pda_hip.h: device pointers, an explicit `void* stream` (hipStream_t), int return codes (PDA_OK / PDA_ERR_*), and every
 * argument check happens before anything is launched.  Kept in its own header, like pda_hip_ips.h.
 *
 * Source: Zhu, Wang, Caverlee, "Popularity-Opportunity Bias in Collaborative Filtering" (WSDM'21): the BPR loss plus the squared Pearson
 * correlation, over the batch, between the predicted score of the observed pairs and the popularity of their items.  The paper was not at hand
 * when this was written: the objective below is its description RESTATED FROM MEMORY, written out in full so that nothing depends
 * on it, and it is the contract the tests hold the kernels to (tests/pcc_ref.py).
 *
 * Model: the tables of a BPRMF, U f32 [n_users, d], I f32 [n_items, d]; a PCC model differs from a BPRMF only in how it was
 * trained, and every evaluation entry point of pda_hip.h serves it unchanged (PDA_HEAD_RAW).  pop f32 [n_items]: the popularity of an item,
 * built once per data set on the host (pda_amd.ops.PccPop) from the train interactions n_i: (float)n_i, or (float)log1p(n_i) taken in float64.
 * Pearson's r is invariant to positive affine maps of either side, so counts, shares and propensities give the same model.
 * Per batch of B triplets (u, p, n), V the valid ones (ids inside the tables), n_v = |V|:
 *     s_p = u.p,  s_n = u.n,  x_t = s_p - s_n                  (the raw dots, fp32)
 *     z_t = s_p (PDA_PCC_ON_POS)  |  x_t (PDA_PCC_ON_MARGIN),   q_t = pop[p_t]
 *     zbar = mean_V z,  qbar = mean_V q,  Szz = sum_V (z - zbar)^2,  Sqq = sum_V (q - qbar)^2,  Szq = sum_V (z - zbar)(q - qbar)
 *     r    = Szq / sqrt(Szz Sqq)  if n_v >= 2 and Szz > 0 and Sqq > 0,  else r = 0             (then the step IS the BPR step)
 *     bpr  = -(1 / B) sum_V log(sigmoid(x_t) + 1e-10)
 *     mf   = bpr + gamma r^2
 *     reg  = regs (l2(u) + l2(p) + l2(n)) / reg_div                                             (the term of pda_bpr_step_f32)
 *     loss = mf + reg
 *     d (gamma r^2) / d z_t = (2 gamma r / sqrt(Szz Sqq)) ((q_t - qbar) - (Szq / Szz)(z_t - zbar))
 * The coefficient goes on the positive's score (ON_POS), or on the positive's score and, negated, on the negative's (ON_MARGIN).
 * The statistic: taken from the fp32 z_t and q_t in float64, CENTRED (the means first, then the centred sums), in a fixed order (thread-strided,
 * wave ladder, waves in order) without float atomics: the same bits run after run, Sqq exactly 0 when every positive has the same popularity and
 * Szz exactly 0 when n_v = 1.  A triplet with an id outside the tables is skipped: it adds nothing to the loss, to the gradients or to the
 * statistic (memory safety only: the callers validate their ids); 1 / B still counts it.  d in {32, 64, 128, 256}.
 */
#ifndef PDA_HIP_PCC_H
#define PDA_HIP_PCC_H

#include "pda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PDA_PCC_ON_POS 0      /* z_t = s_p: the score of the observed pair (Zhu et al.) */
#define PDA_PCC_ON_MARGIN 1   /* z_t = s_p - s_n: the pairwise margin */
#define PDA_PCC_STAT_WORDS 8  /* doubles in `stat` */

/* The batch's statistic, two launches.  The score pass (the layout of pda_bpr_step_f32: d / 4 lanes per triplet) writes z_ws f32 [B]: z_t, and 0
 * for a refused triplet (which triplets count is always decided by the ids, never by the value).  The moments pass is ONE workgroup of 1 024
 * threads looping over B: stat f64 [8] = (n_v, zbar, qbar, Szz, Sqq, Szq, r, 0). */
/* Buffer contract -- z_ws (f32 [B]): needs no initialisation -- the score pass writes every one of its B elements before the moments pass, pda_pcc_grads_f32
 * and the step read them; afterwards a caller may read all of it (the z_t of this batch); one z_ws (with its stat) serves one batch at a time.
 * stat is an output, written in full by the moments pass. */
int pda_pcc_stats_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg,
                      const float* pop, int B, int d, int on, float* z_ws, double* stat, void* stream);

/* The batch's gradients (one launch, the layout of pda_bpr_step_f32) from z_ws and stat as pda_pcc_stats_f32 left them for THIS batch and these
 * tables: every triplet's score gradient is the BPR one plus d (gamma r^2) / d z_t, taken in float64 from the z_t bits of the workspace.  gamma
 * >= 0.  The gradients are SUMMED into gU [n_users, d] / gI [n_items, d] (duplicates add up; equal positives inside a workgroup are combined on
 * chip first); the rows touched get tagU[user] = tagI[pos] = tagI[neg] = step_tag, exactly as pda_adam_step_f32 tags them.
 * flags: PDA_UPD_ANY_ORDER (the batch is not grouped by positive) | PDA_UPD_USERS_DISTINCT (no user id occurs twice: its gU row, zero before the
 * call, takes a plain store).  loss_acc (optional) f32 [3] += (loss, mf, reg): gamma r^2 is added once per step.  pcc_acc (optional) f32 [2] +=
 * (r, r^2), once per step.
 * PRECONDITION of PDA_UPD_USERS_DISTINCT, as for pda_adam_step_f32 (pda_hip.h): the plain store is the row's gradient only if gU is zero on every
 * row the batch touches and no user occurs twice.  The sweep of pda_pcc_adam_step_f32 zeroes what the step wrote; a non-OK return between the
 * step and the sweep leaves gU / gI and the tags dirty, and the caller zeroes them before going on. */
int pda_pcc_step_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg,
                     const float* pop, const float* z_ws, const double* stat, int B, int d, float gamma, int on, float regs, float reg_div,
                     float* gU, float* gI, int32_t* tagU, int32_t* tagI, int step_tag, int flags, float* loss_acc, float* pcc_acc, void* stream);

/* One train step: pda_pcc_stats_f32, pda_pcc_step_f32, then TF-1.14's dense-decay Adam over both tables by pda_adam_dense_sweep4_f32 (the sweep
 * of pda_adam_step_f32: g = 0 off the tagged rows, g zeroed behind itself).  Four launches, no host read: capturable in a HIP graph.  z_ws f32
 * [B] and stat f64 [8]: device memory private to the stream.  flags and cache_policy: those of pda_adam_step_f32. */
int pda_pcc_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI, float* gI,
                          int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg, const float* pop,
                          float* z_ws, double* stat, int B, int d, float gamma, int on, float regs, float reg_div, int step_tag, float lr_t,
                          float beta1, float beta2, float eps, int flags, int cache_policy, float* loss_acc, float* pcc_acc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_PCC_H */
