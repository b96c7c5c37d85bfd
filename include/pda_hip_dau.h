/* pda_hip_dau.h -- the DirectAU loss (`--train dau`; Wang, Yu, Ma, Zhang, Chen, Liu, Ma, KDD'22, "Towards Representation Alignment and Uniformity in
 * Collaborative Filtering") on libpda_hip.so.  The paper and its code were not at hand when this was written: the objective below is their
 * description RESTATED FROM MEMORY, written out in full so that nothing depends on it, and it is the contract the tests hold the
 * kernels to (tests/dau_ref.py).
 *
 * Same conventions as pda_hip.h and pda_hip_inbatch.h: device pointers, an explicit `void* stream` (hipStream_t), int return codes (PDA_OK /
 * PDA_ERR_*), and every argument check happens before anything is launched.
 *
 * Model: the tables of a BPRMF, U f32 [n_users, d], I f32 [n_items, d], d in {32, 64, 128, 256}.
 * Batch: users i32 [B], pos i32 [B], 1 <= B <= PDA_DAU_MAX_B.  No negatives.  The two [B, B] Gram matrices U^ U^T and I^ I^T exist only as
 * 32 x 32 tiles in the accumulators of v_mfma_f32_32x32x2_f32 (exact f32).
 *     x^         = x / max(|x|, 1e-12)                          (u^_r = unit(U[users[r]]), i^_r = unit(I[pos[r]]))
 *     align      = (1 / B) sum_r |u^_r - i^_r|^2
 *     for a side X in {(u^_r, id = users[r]), (i^_r, id = pos[r])} over the valid rows:
 *       adm(a,b) = a != b  and  (same == PDA_DAU_SAME_KEEP  or  id_a != id_b)
 *       e_ab     = exp(-t (|x^_a|^2 + |x^_b|^2 - 2 x^_a . x^_b))   for adm(a,b), else 0
 *       r_a      = sum_b e_ab          n_a = #{b : adm(a,b)}       G_a = sum_b e_ab x^_b
 *       S        = (1/2) sum_a r_a     P   = (1/2) sum_a n_a       (integers for n, P)
 *       uni_X    = log(S / P)  if P > 0  else 0
 *       d uni_X / d x^_a = (-2 t / S) (r_a x^_a - G_a)             (0 if P = 0)
 *     mf    = align + gamma (uni_U + uni_I) / 2
 *     reg   = regs sum_r (l2(u_r) + l2(i_r)) / reg_div             (every ROW once, l2 = 0.5 sum x^2)
 *     loss  = mf + reg
 *     gU[users[r]] += (g_r - (u^_r . g_r) u^_r) / max(|u_r|, 1e-12) + c_reg u_r ,   g_r = (2 / B)(u^_r - i^_r) + (gamma / 2) d uni_U / d u^_r
 *     gI[pos[r]]   += likewise with  -(2 / B)(u^_r - i^_r)  and  d uni_I / d i^_r ,   c_reg = regs / reg_div
 * PDA_DAU_SAME_KEEP is a pairwise distance over the batch as it stands: two rows that carry the same id are the same table row, their distance
 * is 0 and e_ab = 1 EXACTLY (the step does not take that distance from rounded dot products), with no gradient.  PDA_DAU_SAME_DROP leaves the
 * pairs of equal id out of S and P.  Rows that carry the same item each add their own gI term.  The exponent is clamped at 0 from above, so no
 * pass looks for a maximum; 0 < t <= PDA_DAU_MAX_T keeps exp(-4 t) a normal fp32 number, so S > 0 whenever P > 0.
 * Validity: a row whose users[r] or pos[r] lies outside the tables is dropped from everything (memory safety only: the callers validate their
 * ids); B still divides the alignment mean and reg_div the regulariser.
 * Sums: r and G of a row have one writer per column split and are added in split order; S, P (from the sums the workgroups of the tile pass
 * leave over their 32 rows, taken in a fixed order), align and the regulariser are reduced by ONE workgroup in float64 in a fixed order.
 * loss_acc and stat receive the same bits run after run; only the final scatter of repeated ids into gU / gI takes float atomics.
 */
#ifndef PDA_HIP_DAU_H
#define PDA_HIP_DAU_H

#include "pda_hip.h"

#define PDA_DAU_MAX_B 16384
#define PDA_DAU_MAX_T 20.0f
/* the edge of a Gram tile (one v_mfma_f32_32x32x2_f32 accumulator) */
#define PDA_DAU_TILE 32
#define PDA_DAU_SAME_KEEP 0   /* pairs of rows with the same id count, at distance 0 (a pairwise distance over the batch as it stands) */
#define PDA_DAU_SAME_DROP 1   /* pairs of rows with the same id are left out of S and P */
#define PDA_DAU_STAT_WORDS 4  /* floats in `stat` */

#ifdef __cplusplus
extern "C" {
#endif

/* The number of column ranges the pass over the Gram tiles splits the B columns into (>= 1, <= ceil(B / PDA_DAU_TILE); a function of B alone, 0
 * for a B outside 1 .. PDA_DAU_MAX_B): 2 sides x ceil(B / PDA_DAU_TILE) row tiles x this many workgroups of one wave fill the chip. */
int pda_dau_col_splits(int B);

/* Bytes of the step's workspace: the packed image of the 2 B normalised rows, some words per row, and r and G per side, row and column
 * split.  splits x B is bounded by B + 16 384, so the size is linear in B.  No [B, B] matrix exists in global memory.  0 for a B or d the
 * step refuses. */
/* Buffer contract -- ws (pda_dau_workspace_bytes): needs no initialisation -- every word a kernel of the call reads was written earlier by the same
 * call; nothing in it is meant for the caller afterwards; one workspace serves one call at a time (private to one stream). */
size_t pda_dau_workspace_bytes(int B, int d);

/* The batch's gradients, FOUR launches whatever B (pack the 2 B rows with the alignment term; ONE pass over the Gram tiles of both sides; the
 * one-workgroup reduction; the tail), nothing read on the host: capturable in a HIP graph.  The gradients are SUMMED into gU [n_users, d] / gI
 * [n_items, d]; the rows touched get tagU[user] = tagI[pos] = step_tag.  flags: PDA_UPD_ANY_ORDER | PDA_UPD_USERS_DISTINCT with the meaning and
 * the PRECONDITION written in pda_hip_ssm.h (pda_ssm_step_f32).  loss_acc (optional) f32 [3] += (loss, mf, reg).  stat (optional) f32 [4] +=
 * (align, uni_U, uni_I, 1).  ws: pda_dau_workspace_bytes(B, d) bytes, 16-byte aligned, overwritten.
 * PDA_ERR_ARG: a null pointer (stat, loss_acc aside), B outside 1 .. PDA_DAU_MAX_B, t outside (0, PDA_DAU_MAX_T], gamma < 0 or not finite, same
 * outside {KEEP, DROP}, reg_div <= 0, step_tag <= 0, other flags, ws_bytes too small.  PDA_ERR_UNSUPPORTED: d. */
int pda_dau_step_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, int B, int d,
                     float t, float gamma, int same, float regs, float reg_div, float* gU, float* gI, int32_t* tagU, int32_t* tagI, int step_tag,
                     int flags, void* ws, size_t ws_bytes, float* stat, float* loss_acc, void* stream);

/* One train step: pda_dau_step_f32, then TF-1.14's dense-decay Adam over both tables by pda_adam_dense_sweep4_f32, exactly as
 * pda_inbatch_adam_step_f32 chains them.  flags and cache_policy: those of pda_adam_step_f32. */
int pda_dau_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI, float* gI,
                          int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, int B, int d, float t, float gamma, int same,
                          float regs, float reg_div, int step_tag, float lr_t, float beta1, float beta2, float eps, int flags, int cache_policy,
                          void* ws, size_t ws_bytes, float* stat, float* loss_acc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_DAU_H */
