/* pda_hip_macr.h -- MACR (Wei et al., KDD'21, "Model-Agnostic Counterfactual Reasoning for Eliminating Popularity Bias in Recommender System";
 * `--train macr`) on libpda_hip.so: the three-branch loss of MF/model_api.py:613-651 (create_bce_loss_two_brach_both) and what its
 * counterfactual inference (rubi_ratings_both, :627-628) needs from the item table.
 *
 * Same conventions as pda_hip.h: device pointers, an explicit `void* stream` (hipStream_t), int return codes (PDA_OK / PDA_ERR_*), every
 * argument check happens before anything is launched, and nothing is allocated.  Kept in its own header, like pda_hip_dice.h and pda_hip_ips.h.
 *
 * Model.  Parameters: U f32 [n_users, d], I f32 [n_items, d], and the two branch vectors w_item f32 [d], w_user f32 [d] (the
 * reference's `item_branch` / `user_branch`, [d, 1], no bias).  Per triplet (u, p, n) of a batch of B, raw dots (no ELU, no popularity):
 *     y_p = u.p    y_n = u.n    s_p = sigmoid(p.w_item)    s_n = sigmoid(n.w_item)    s_u = sigmoid(u.w_user)
 *     a_p = y_p s_p s_u         a_n = y_n s_n s_u
 *     L_O = mean_t( -log(sigmoid(a_p) + 1e-10) - log(1 - sigmoid(a_n) + 1e-10) )
 *     L_I = mean_t( -log(s_p + 1e-10)          - log(1 - s_n + 1e-10) )
 *     L_U = mean_t( -log(s_u + 1e-10)          - log(1 - s_u + 1e-10) )      (as the reference writes it: the user is its own negative)
 *     reg = regs (l2(u) + l2(p) + l2(n)) / reg_div                           (l2(x) = sum(x^2) / 2; the branch vectors are not regularised)
 *     loss = L_O + alpha L_I + beta L_U + reg
 * All of it in fp32, in that op order: 1 - sigmoid(x) + 1e-10 is computed as written, so a saturated sigmoid yields log(1e-10), not -inf.
 * There is no stop-gradient (the reference's `*_stop` names are plain aliases): u receives gradient through y_p, y_n and s_u; p through y_p
 * and s_p; n through y_n and s_n; w_item through s_p and s_n (from L_O and L_I); w_user through s_u (from L_O and L_U).
 * A triplet with an id outside the tables is skipped: it adds nothing to the loss or to any gradient (memory safety only: the callers
 * validate their ids).  d in {32, 64, 128, 256}.
 *
 * Inference.  The model scores (y_ui - c) s_i s_u; s_u > 0 does not change a user's ranking, so lists are ranked by (y_ui - c) s_i
 * = u.(s_i I_i) - c s_i, which is the bias head of pda_hip_temp_pop.h on J_i = fl(s_i I_i) with alpha = 1 and beta_i = fl(-c s_i):
 *     a MACR list is top_k( fl(chain(u . J_i) + beta_i) + mask ), ties broken by the lower item id,
 * chain the exact fp32 chain of pda_temp_pop_score_topk_f32.  It differs from fl(fl(y - c) * s_i) by rounding alone (J_i is rounded once per
 * element, the sum once more).  c = 0 is the reference's rubi_ratings_both_nonc.
 */
#ifndef PDA_HIP_MACR_H
#define PDA_HIP_MACR_H

#include "pda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The batch's gradients (one launch, the layout of pda_bpr_step_f32: d / 4 lanes per triplet).  The row gradients are SUMMED into
 * gU [n_users, d] / gI [n_items, d] (duplicates add up; equal positives inside a workgroup are combined on chip first); the rows touched get
 * tagU[user] = tagI[pos] = tagI[neg] = step_tag, exactly as pda_adam_step_f32 tags them.  The gradients of the branch vectors are SUMMED into
 * gW f32 [2, d] (row 0: w_item, row 1: w_user): every workgroup reduces its triplets on chip and adds 2 d values.
 * flags: PDA_UPD_ANY_ORDER (the batch is not grouped by positive) | PDA_UPD_USERS_DISTINCT (no user id occurs twice: its gU row, zero before the
 * call, takes a plain store).  loss_acc (optional) f32 [5] += (loss, L_O, L_I, L_U, reg): L_I and L_U unweighted.
 * PRECONDITION of PDA_UPD_USERS_DISTINCT, as for pda_adam_step_f32 (pda_hip.h): the plain store is the row's gradient only if gU is zero on every
 * row the batch touches and no user occurs twice.  The sweeps of pda_macr_adam_step_f32 zero what the step wrote; a non-OK return between the
 * step and the sweeps leaves gU / gI / gW and the tags dirty, and the caller zeroes them before going on. */
int pda_macr_step_f32(const float* U, const float* I, const float* w_item, const float* w_user, size_t n_users, size_t n_items,
                      const int32_t* users, const int32_t* pos, const int32_t* neg, int B, int d, float alpha, float beta, float regs, float reg_div,
                      float* gU, float* gI, float* gW, int32_t* tagU, int32_t* tagI, int step_tag, int flags, float* loss_acc, void* stream);

/* One train step: pda_macr_step_f32, then TF-1.14's dense-decay Adam over both tables by pda_adam_dense_sweep4_f32 (the sweep of
 * pda_adam_step_f32: g = 0 off the tagged rows, g zeroed behind itself), then the same Adam over the two branch vectors by
 * pda_adam_dense_sweep2_f32 on (w_item, w_user) with n = d each (element for element the arithmetic of the table sweep; gW zeroed behind
 * itself).  Three launches, no host read: capturable in a HIP graph.  mW / vW f32 [2, d]: the moments of (w_item, w_user).  flags and
 * cache_policy: those of pda_adam_step_f32.  gU / gI / gW are zero before the first step and are only written here. */
int pda_macr_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI, float* gI,
                           int32_t* tagI, size_t n_items, float* w_item, float* w_user, float* mW, float* vW, float* gW, const int32_t* users,
                           const int32_t* pos, const int32_t* neg, int B, int d, float alpha, float beta, float regs, float reg_div, int step_tag,
                           float lr_t, float beta1, float beta2, float eps, int flags, int cache_policy, float* loss_acc, void* stream);

/* For the evaluation, one launch over the item table: sig f32 [n_items] = sigmoid(I_i . w_item), J f32 [n_items, d] = fl(sig_i * I_i).
 * d / 4 lanes per row; the row dot is a fixed-order reduction (the lane's four products left to right, then the xor ladder): the same bits run
 * after run. */
int pda_macr_item_prep_f32(const float* I, const float* w_item, size_t n_items, int d, float* sig, float* J, void* stream);

/* beta_i = fl(-c * sig_i), i < n: once per value of c. */
int pda_macr_item_bias_f32(const float* sig, float c, float* beta, size_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_MACR_H */
