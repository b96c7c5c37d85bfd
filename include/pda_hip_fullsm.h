/* pda_hip_fullsm.h -- the full-catalogue softmax loss (`--train ssm --ssm_source all`) on libpda_hip.so: the softmax of a row's positive against
 * EVERY item the user has not interacted with, the loss `--ssm_source sampled` (Wu et al., "On the Effectiveness of Sampled Softmax Loss for Item
 * Recommendation") and `--ssm_source batch` (Yi et al., RecSys'19) estimate.
 *
 * Same conventions as pda_hip.h, pda_hip_ssm.h and pda_hip_inbatch.h: device pointers, an explicit `void* stream` (hipStream_t), int return codes
 * (PDA_OK / PDA_ERR_*), every argument check happens before anything is launched, nothing is allocated.
 *
 * Model: the tables of a BPRMF, U f32 [n_users, d], I f32 [n_items, d], d in {32, 64, 128, 256}.
 * Batch: users i32 [B], pos i32 [B], 1 <= B <= PDA_FULLSM_MAX_B.  The columns of the [B, n_items] logit matrix are ALL items c = 0 .. n_items - 1.
 * Optional input: the train graph as a CSR, train_indptr i64 [n_users + 1] and train_indices i32 (item ids, ascending inside a row); both null:
 * no item is excluded.
 *     a_rc  = u_r . i_c                      (norm == 0),   u_r = U[users[r]], i_c = I[c]
 *     a_rc  = u^_r . i^_c                    (norm == 1),   x^ = x / max(|x|, 1e-12)
 *     S_rc  = a_rc / tau
 *     E_r   = {pos[r]} + {c : c is not a train item of users[r]}        (all items without the train graph)
 *     l_r   = lse_{c in E_r} S_rc - S_{r,pos[r]}     (max-subtracted; the loss takes (m - S_pos) + log(se), as pda_ssm.hip does)
 *     mf    = (1 / B) sum_r l_r
 *     reg   = regs sum_r (l2(u_r) + l2(i_pos[r])) / reg_div             (l2 = 0.5 sum x^2; every ROW once, as in-batch)
 *     loss  = mf + reg
 * Gradients: the derivative of the above.  p_rc = exp(S_rc - lse_r) for c in E_r, else 0;  C_rc = (p_rc - [c == pos[r]]) / (tau B);
 * c_reg = regs / reg_div;  n_c = the number of valid rows with pos[r] == c:
 *     norm 0:  gU[users[r]] += sum_c C_rc i_c + c_reg u_r        gI[c] += sum_r C_rc u_r + n_c c_reg i_c
 *     norm 1:  g_r = sum_c C_rc i^_c ;  gU[users[r]] += (g_r - (u^_r . g_r) u^_r) / max(|u_r|, 1e-12) + c_reg u_r
 *              h_c = sum_r C_rc u^_r ;  gI[c]        += (h_c - (i^_c . h_c) i^_c) / max(|i_c|, 1e-12) + n_c c_reg i_c      for EVERY item c
 * Validity: a row whose users[r] or pos[r] lies outside the tables is dropped (memory safety only: the callers validate their ids); B divides
 * the mean regardless.  A row whose every other item is excluded has l_r = 0, p_{r,pos[r]} = 1 and takes only the regulariser.
 */
#ifndef PDA_HIP_FULLSM_H
#define PDA_HIP_FULLSM_H

#include "pda_hip.h"

#define PDA_FULLSM_MAX_B 16384
/* the edges of a logit tile (one v_mfma_f32_32x32x2_f32 accumulator): rows x columns */
#define PDA_FULLSM_ROW_TILE 32
#define PDA_FULLSM_COL_TILE 32

#ifdef __cplusplus
extern "C" {
#endif

/* The number of column ranges the row-statistics pass and the user-side gradient pass split the n_items columns into (>= 1,
 * <= ceil(n_items / PDA_FULLSM_COL_TILE); a function of the two sizes alone, 0 for a B outside 1 .. PDA_FULLSM_MAX_B or an n_items outside
 * 1 .. 2^31 - 1): ceil(B / PDA_FULLSM_ROW_TILE) x this many workgroups fill the chip. */
int pda_fullsm_col_splits(size_t n_items, int B);

/* Bytes of the step's workspace: the packed image of the B user rows, 1 / max(|i_c|, 1e-12) per item, the exclusion bit mask of
 * B x ceil(n_items / 32) words, (m, se) per row and column split, the partial g_r [B, d] per column split and some words per row.  No array of
 * B x n_items logits or probabilities exists.  0 for a B, n_items or d the step refuses. */
/* Buffer contract -- ws (pda_fullsm_workspace_bytes): needs no initialisation -- every word a kernel of the call reads was written earlier by the same
 * call; nothing in it is meant for the caller afterwards; one workspace serves one call at a time (private to one stream). */
size_t pda_fullsm_workspace_bytes(int B, size_t n_items, int d);

/* The batch's gradients, nothing read on the host: capturable in a HIP graph.  The launches: pack the user rows; the items' inverse norms
 * (norm == 1); the exclusion bits (train graph given); row statistics over the logit tiles (row tiles x column splits); (m, se) merged per row
 * in split order; the user-side product C I^ per (row tile, column split) into per-split partial sums; the item-side product C^T U^ by the
 * workgroup that OWNS the column tile, summed over all row tiles in ascending order in registers and written to gI; the tail (the partial g_r
 * added in split order, the projection, c_reg u_r, gU, the tags); the loss terms summed in a fixed order.
 * The gradients are SUMMED into gU [n_users, d] / gI [n_items, d].  tagU[users[r]] = step_tag for the valid rows and tagI[c] = step_tag for EVERY
 * item c (every item takes a gradient).  flags: PDA_UPD_ANY_ORDER | PDA_UPD_USERS_DISTINCT with the meaning and the PRECONDITION written in
 * pda_hip_ssm.h (pda_ssm_step_f32); the batch order plays no part here, PDA_UPD_ANY_ORDER is accepted and ignored.
 * loss_acc (optional) f32 [3] += (loss, mf, reg).  row_stats (optional) f32 [B, 2] = (m_r, log se_r) of row r: m_r = max_{c in E_r} S_rc,
 * se_r = sum_{c in E_r} exp(S_rc - m_r); (0, 0) for a dropped row.  ws: pda_fullsm_workspace_bytes(B, n_items, d) bytes, 16-byte aligned,
 * overwritten.
 * Reproducibility: no float atomic touches the item side, the row statistics, the partial g_r or the loss terms, and every sum has a fixed
 * order.  With PDA_UPD_USERS_DISTINCT the loss terms, gU and gI are the same bits call after call.  Without the flag a user row takes one float
 * atomic per occurrence: a user that occurs more than twice in a batch may differ in the last bits of its gU row from call to call.
 * PDA_ERR_ARG: a null pointer (train_indptr / train_indices, loss_acc, row_stats aside), exactly one of train_indptr / train_indices null,
 * B outside 1 .. PDA_FULLSM_MAX_B, tau <= 0 or not finite, norm outside {0, 1}, reg_div <= 0, step_tag <= 0, other flags, ws not aligned,
 * ws_bytes too small.  PDA_ERR_UNSUPPORTED: d. */
int pda_fullsm_step_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, int B, int d,
                        float tau, int norm, const int64_t* train_indptr, const int32_t* train_indices, float regs, float reg_div, float* gU,
                        float* gI, int32_t* tagU, int32_t* tagI, int step_tag, int flags, void* ws, size_t ws_bytes, float* loss_acc,
                        float* row_stats, void* stream);

/* One train step: pda_fullsm_step_f32, then TF-1.14's dense-decay Adam over both tables by pda_adam_dense_sweep4_f32, exactly as
 * pda_inbatch_adam_step_f32 chains them.  flags and cache_policy: those of pda_adam_step_f32. */
int pda_fullsm_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI, float* gI,
                             int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, int B, int d, float tau, int norm,
                             const int64_t* train_indptr, const int32_t* train_indices, float regs, float reg_div, int step_tag, float lr_t,
                             float beta1, float beta2, float eps, int flags, int cache_policy, void* ws, size_t ws_bytes, float* loss_acc,
                             float* row_stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_FULLSM_H */
