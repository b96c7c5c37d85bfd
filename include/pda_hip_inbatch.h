/* pda_hip_inbatch.h -- the in-batch softmax with logQ correction (`--train ssm --ssm_source batch`; Yi et al., RecSys'19, "Sampling-Bias-
 * Corrected Neural Modeling for Large Corpus Item Recommendations") on libpda_hip.so.
 *
 * Same conventions as pda_hip.h and pda_hip_ssm.h: device pointers, an explicit `void* stream` (hipStream_t), int return codes (PDA_OK /
 * PDA_ERR_*), and every argument check happens before anything is launched.
 *
 * Model: the tables of a BPRMF, U f32 [n_users, d], I f32 [n_items, d], d in {32, 64, 128, 256}.
 * Batch: users i32 [B], pos i32 [B], 1 <= B <= PDA_INBATCH_MAX_B.  The B positives are the columns of ONE [B, B] logit matrix every row shares.
 * Optional inputs (either may be null): logq f32 [n_items];  mask u32 [B, W], W = ceil(B / 32): bit c % 32 of word [r, c / 32] set means
 * column c is excluded from row r.
 *     a_rc  = u_r . i_c                      (norm == 0),   u_r = U[users[r]], i_c = I[pos[c]]
 *     a_rc  = u^_r . i^_c                    (norm == 1),   x^ = x / max(|x|, 1e-12)
 *     S_rc  = a_rc / tau - (logq ? logq[pos[c]] : 0)        (the positive's own column included)
 *     E_r   = {r} + {c != r : pos[c] != pos[r], bit (r, c) of mask clear, row c valid}
 *     l_r   = lse_{c in E_r} S_rc - S_rr     (max-subtracted; the loss takes (m - S_rr) + log(se), as pda_ssm.hip does)
 *     mf    = (1 / B) sum_r l_r
 *     reg   = regs sum_r (l2(u_r) + l2(i_r)) / reg_div      (l2 = 0.5 sum x^2; every ROW once: a column occurrence is not regularised again)
 *     loss  = mf + reg
 * Gradients: the derivative of the above (logq has none).  p_rc = exp(S_rc - lse_r) for c in E_r, else 0;  C_rc = (p_rc - [r == c]) / (tau B);
 * c_reg = regs / reg_div:
 *     norm 0:  gU[users[r]] += sum_c C_rc i_c + c_reg u_r        gI[pos[c]] += sum_r C_rc u_r + c_reg i_c
 *     norm 1:  g_r = sum_c C_rc i^_c ;  gU[users[r]] += (g_r - (u^_r . g_r) u^_r) / max(|u_r|, 1e-12) + c_reg u_r
 *              h_c = sum_r C_rc u^_r ;  gI[pos[c]]  += (h_c - (i^_c . h_c) i^_c) / max(|i_c|, 1e-12) + c_reg i_c
 * Columns that carry the same item each add their own gI term.  The exclusion pos[c] != pos[r] is the step's own, with or without `mask`.
 * Validity: a row whose users[r] or pos[r] lies outside the tables is dropped as a row AND as a column (memory safety only: the callers validate
 * their ids); B divides the mean regardless.  A row whose every other column is excluded has l_r = 0, p_rr = 1 and takes only the regulariser.
 */
#ifndef PDA_HIP_INBATCH_H
#define PDA_HIP_INBATCH_H

#include "pda_hip.h"

#define PDA_INBATCH_MAX_B 16384
/* the edges of a logit tile (one v_mfma_f32_32x32x2_f32 accumulator): rows x columns */
#define PDA_INBATCH_ROW_TILE 32
#define PDA_INBATCH_COL_TILE 32

#ifdef __cplusplus
extern "C" {
#endif

/* The number of column ranges the two passes over the logit tiles split the B columns into (>= 1, <= ceil(B / PDA_INBATCH_COL_TILE); a
 * function of B alone, 0 for a B outside 1 .. PDA_INBATCH_MAX_B): ceil(B / PDA_INBATCH_ROW_TILE) x this many workgroups fill the chip. */
int pda_inbatch_col_splits(int B);

/* Bytes of the step's workspace, linear in B: the packed image of the 2 B gathered rows, two [B, d] gradient buffers, some words per row and
 * (m, se) per row and column split.  The [B, B] matrix never exists in global memory.  0 for a B or d the step refuses. */
/* Buffer contract -- ws (pda_inbatch_workspace_bytes): needs no initialisation -- every word a kernel of the call reads was written earlier by the same
 * call; nothing in it is meant for the caller afterwards; one workspace serves one call at a time (private to one stream). */
size_t pda_inbatch_workspace_bytes(int B, int d);

/* mask u32 [B, ceil(B / 32)]: bit (r, c) is set iff c != r and pos[c] is in the sorted train row of users[r] (binary search, the sampler's own
 * membership test).  Bits of c >= B, of invalid rows and of invalid columns (a user or a positive outside the tables) are zero.  Every word
 * has one writer (a ballot of 32 threads, one per column): the same bits run after run.  PDA_ERR_ARG: a null pointer, B outside
 * 1 .. PDA_INBATCH_MAX_B, empty or too large tables. */
int pda_inbatch_mask(const int32_t* users, const int32_t* pos, int B, const int64_t* train_indptr, const int32_t* train_indices, size_t n_users,
                     size_t n_items, uint32_t* mask, void* stream);

/* The batch's gradients, FOUR launches whatever B (pack the 2 B rows; row statistics over the logit tiles; the gradient products over the tiles
 * again; the tail), nothing read on the host: capturable in a HIP graph.  The gradients are SUMMED into gU [n_users, d] / gI [n_items, d]; the
 * rows touched get tagU[user] = tagI[pos] = step_tag.  flags: PDA_UPD_ANY_ORDER | PDA_UPD_USERS_DISTINCT with the meaning and the PRECONDITION
 * written in pda_hip_ssm.h (pda_ssm_step_f32).  loss_acc (optional) f32 [3] += (loss, mf, reg).  ws: pda_inbatch_workspace_bytes(B, d) bytes,
 * 16-byte aligned, overwritten.  The partial sums of the gradient pass take float atomics: the sums are not bit-reproducible.
 * PDA_ERR_ARG: a null pointer (logq, mask, loss_acc aside), B outside 1 .. PDA_INBATCH_MAX_B, tau <= 0 or not finite, norm outside {0, 1},
 * reg_div <= 0, step_tag <= 0, other flags, ws_bytes too small.  PDA_ERR_UNSUPPORTED: d. */
int pda_inbatch_step_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, int B, int d,
                         float tau, int norm, const float* logq, const uint32_t* mask, float regs, float reg_div, float* gU, float* gI,
                         int32_t* tagU, int32_t* tagI, int step_tag, int flags, void* ws, size_t ws_bytes, float* loss_acc, void* stream);

/* One train step: pda_inbatch_step_f32, then TF-1.14's dense-decay Adam over both tables by pda_adam_dense_sweep4_f32, exactly as
 * pda_ssm_adam_step_f32 chains them.  flags and cache_policy: those of pda_adam_step_f32. */
int pda_inbatch_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI, float* gI,
                              int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, int B, int d, float tau, int norm,
                              const float* logq, const uint32_t* mask, float regs, float reg_div, int step_tag, float lr_t, float beta1,
                              float beta2, float eps, int flags, int cache_policy, void* ws, size_t ws_bytes, float* loss_acc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_INBATCH_H */
