/* pda_hip_pc.h -- BPR-PC (popularity-compensated re-ranking, Zhu et al., WSDM'21) on libpda_hip.so.
 *
 * Same conventions as pda_hip.h: device pointers, an explicit `void* stream` (hipStream_t), int return codes (PDA_OK / PDA_ERR_*), and every
 * argument check happens before anything is launched.  Kept in its own header, like pda_hip_temp_pop.h.
 *
 * Contract ("5b. BPR-PC"), for a trained BPRMF (U, I) over the FULL catalogue of n_items items, RN32 = rounding to fp32:
 *   a = RN32(alpha), b = RN32(beta), w = RN32(1 - beta) (1 - beta in double), e = RN32(0.01), p_i = RN32(1 / pop_i)
 *   s_ui  the exact fp32 score chain of pda_score_topk_f32;  c_ui the number of times item i is listed in u's history row
 *   C_ui = RN32(RN32(RN32(s_ui b) + w) p_i)
 *   A_u  = sum_i (1 - c_ui)^2 s_ui^2,  Bc_u = sum_i (1 - c_ui)^2 C_ui^2   (float64; computed from item moments, see below)
 *   n_u = n_items - sum_i c_ui,  inv_u = |RN32(1 / n_u)|,  U_n = RN32(inv_u sqrt(A_u)),  U_c = RN32(inv_u sqrt(Bc_u))   (duplicates: n_u < 0 can occur)
 *   k_u = RN32(U_n RN32(1 / U_c)), and k_u = 0 where n_u = 0 or U_c = 0 (the reference gives NaN / inf there: a documented deviation)
 *   r_ui = RN32(s_ui + RN32(a RN32(C_ui k_u)))
 *   m_B  = min r_ui over every row of a group of rows_per_min consecutive rows and every item, the listed ones included
 *   g_ui = RN32(RN32(r_ui - m_B) + e); a listed item is worth g after c subtractions of g (0 if listed once)
 *   result: the first K items by (g descending, item id ascending), values g.
 */
#ifndef PDA_HIP_PC_H
#define PDA_HIP_PC_H

#include "pda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PDA_HEAD_PC 3     /* BPR-PC: ranks by r (per-row minimum of r kept), then by g -- the heads of pda_hip.h are 0, 1; temp_pop's is 2 */
#define PDA_PC_MAX_K 50   /* K <= 50: the sweep keeps K' = min(K + 8, PDA_TOPK_CAP - 6) candidates per row, ranked by r */

/* Item moments, float64, once per (I, pop): moments f64 [2 d^2 + d + 1] = G [d][d] = sum_i v_i v_i^T, H [d][d] = sum_i p_i^2 v_i v_i^T,
 * h [d] = sum_i p_i^2 v_i, P = sum_i p_i^2.  workspace: pda_pc_moments_workspace_bytes(n_items, d) bytes.  pop f32 [n_items], > 0. */
/* Buffer contract -- workspace (pda_pc_moments_workspace_bytes): needs no initialisation -- every block's partial moments are written before the second
 * launch adds them; nothing in it is meant for the caller afterwards; one workspace serves one call at a time. */
size_t pda_pc_moments_workspace_bytes(int n_items, int d);
int pda_pc_item_moments_f32(const float* I, const float* pop, int n_items, int d, double* moments, void* workspace, void* stream);

/* Per-row statistics of a block: U_n, U_c, scale (= k_u) f32 [n_users_blk], from the moments above and the row's history (CSR rows
 * sorted, duplicates adjacent; hist_row_mode PDA_HIST_BY_BLOCK_ROW / PDA_HIST_BY_USER_ID; hist_indptr NULL = no history). */
int pda_pc_user_stats_f32(const float* U, const float* I, const float* pop, const double* moments, const int32_t* users, int n_users_blk,
                          int n_items, int d, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode, double beta,
                          float* U_n, float* U_c, float* scale, void* stream);

/* Score + PC head + history mask + top-K, merged: out_idx int32 [n_users_blk, K], out_val f32 [n_users_blk, K] (= g).  scale f32
 * [n_users_blk] is an INPUT (k_u of each row, e.g. from pda_pc_user_stats_f32).  Rows are grouped by rows_per_min (2 048 in the
 * reference's protocol) for m.  Full catalogue only: I holds all n_items rows, item ids are global.  d in {64, 128, 256};
 * 1 <= K <= PDA_PC_MAX_K <= n_items; alpha, beta finite; pop > 0.
 * Synchronises the stream once (to read the number of rows the ranking by r could not settle; those rows alone are swept again,
 * ranked by g).  workspace: pda_pc_score_workspace_bytes(n_users_blk, n_items, d, K) bytes, 256-byte aligned.  Behind the call:
 * workspace + 16 the identity word (1 << 28 | 1 << 16 | d / 64: generation 1, PC head), workspace + 20 the number of fallback rows. */
/* Buffer contract -- workspace (pda_pc_score_workspace_bytes): needs no initialisation -- its first kernel initialises the two block headers, and every
 * row minimum, key and list is written before it is read; afterwards a caller may read +16 (kernel identity) and +20 (rows served by the fallback); one
 * workspace serves one call at a time. */
size_t pda_pc_score_workspace_bytes(int n_users_blk, int n_items, int d, int K);
int pda_pc_score_topk_f32(const float* U, const float* I, const float* pop, const float* scale, const int32_t* users, int n_users_blk,
                          int n_items, int d, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode, double alpha,
                          double beta, int rows_per_min, int K, int32_t* out_idx, float* out_val, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_PC_H */
