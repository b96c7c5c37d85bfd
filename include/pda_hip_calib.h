/* pda_hip_calib.h -- calibrated-popularity re-ranking ("CP": Steck, RecSys 2018; Abdollahpouri et al., UMAP 2021) on libpda_hip.so: the
 * popularity profile of a user's history, the group counts of a list, and the greedy selection of K items out of a user's N candidates whose
 * popularity mix follows the profile -- up to 8 popularity groups, one launch each, one wave per user.
 *
 * Same conventions as pda_hip.h and pda_hip_xquad.h: device pointers, caller-owned buffers, an explicit `void* stream` (hipStream_t), int
 * return codes (PDA_OK / PDA_ERR_*), and every argument check happens before anything is launched.  No workspace, no allocation, no
 * synchronisation, no float atomics: the same bits whatever the launch geometry.  Every slot of every output is written on every call.
 *
 * Common arguments
 *   item_group  u8 [n_items]: the popularity group of each item, 0 = the most popular.  G = the number of groups, 2 <= G <= PDA_CALIB_MAX_G.
 *               An item whose byte is >= G belongs to no group: it is ignored in profiles and list counts and is never a candidate (it ends
 *               the valid prefix exactly as an id outside [0, n_items) does).
 *
 * Contract of pda_calib_rerank ("5w. Calibrated popularity"), per row (user); RN32 = rounding to fp32, every fp32 operation below a
 * separate operation, `/` the correctly rounded division; everything called "double" is IEEE binary64, one operation at a time:
 *   candidates  cand_idx i32 [n_rows, N], cand_val f32 [n_rows, N]: what pda_score_topk_* / pda_deep_topk_* / pda_deep_merge write.
 *               The valid prefix ends before the first position whose id is outside [0, n_items), whose value is not finite (-1, the
 *               -inf completion of a short row, NaN) or whose item has a group byte >= G; n_valid is its length.
 *               Preconditions: the values do not increase over the valid prefix, and no valid position follows an invalid one (the end of
 *               the prefix is searched for, the row is not streamed).  On a list that breaks one of them the result is unspecified, but every
 *               access stays in bounds.
 *   weights     L = RN32(lambda), W = RN32(1 - lambda) (the subtraction in double), 0 <= lambda <= 1.
 *   relevance   lo = val[n_valid - 1], rng = RN32(val[0] - lo), p_v = RN32(RN32(val[v] - lo) / rng);  p_v = 0 when rng is 0 or not finite.
 *   target      prof i32 [n_rows, G] (pda_calib_profile), H = sum_g prof_g, pi_g = prof_g / H in double.  The counts are expected >= 0
 *               (negative counts: an unspecified, in-bounds result).  H = 0: every divergence below is 0, the row keeps the candidates' order.
 *   divergence  t picks so far, n_g of them of group g; for every group c, in double: q_g = (n_g + [g == c]) / (t + 1), and
 *                 PDA_CALIB_JS  m_g = 0.5 (pi_g + q_g),
 *                               term_g = (pi_g > 0 ? pi_g * log2(pi_g / m_g) : 0) + (q_g > 0 ? q_g * log2(q_g / m_g) : 0),
 *                               D_c = 0.5 * (term_0 + term_1 + ... + term_{G-1}), added in ascending g;
 *                 PDA_CALIB_KL  qs_g = (1 - alpha) q_g + alpha pi_g  (1 - alpha one double, each product rounded, then the sum),
 *                               D_c = the sum over ascending g with pi_g > 0 of pi_g * log(pi_g / qs_g)  (natural logarithm);
 *               both are put on an absolute grid: Dq = min(max(rint(D_c * 2^20), 0), 2^23), ties to even, D32_c = (float)Dq * 2^-20 (exact).
 *               (The device's log and a host's need not agree in the last bit; on the grid such a difference shows only when D_c * 2^20 lies
 *               within that error of a half-integer, and structurally equal divergences stay equal.)
 *   selection   min(K, n_valid) times: x_v = RN32(RN32(W p_v) - RN32(L * D32_c)) for every unpicked candidate v of group c;
 *               the largest x_v is picked, ties go to the smallest position in the candidate list.
 *   result      out_idx i32 [n_rows, K] the picks in order, out_val f32 [n_rows, K] = x at the moment of the pick, out_div f32 [n_rows, K]
 *               (may be NULL) = D32_c of the picked group at the pick: the divergence of the list's first t + 1 items.  Slots behind
 *               min(K, n_valid) hold -1, -inf and -inf.
 */
#ifndef PDA_HIP_CALIB_H
#define PDA_HIP_CALIB_H

#include "pda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PDA_CALIB_MAX_G 8       /* popularity groups */
#define PDA_CALIB_MAX_K 64      /* the columns pda_metrics takes */
#define PDA_CALIB_MAX_N 1024    /* = PDA_DEEP_MAX_K: candidates per row, and columns of a counted list */
#define PDA_CALIB_MAX_KS 8      /* cut-offs of one count call */
#define PDA_CALIB_JS 0
#define PDA_CALIB_KL 1

/* prof i32 [n_rows, G]: the distinct history entries of each row per group.  The history is the CSR of pda_hip.h (rows sorted, so duplicates
 * are adjacent and count once; PDA_HIST_BY_BLOCK_ROW: row r of the CSR, PDA_HIST_BY_USER_ID: row users[r]); ids outside [0, n_items) and
 * items of no group are ignored.  hist_indptr NULL: all zeros (nothing else of the history is read).
 * PDA_ERR_ARG: a NULL item_group or prof; n_rows < 1; n_items < 1; G outside 2 .. PDA_CALIB_MAX_G; a history without its indices or with
 * another row mode; PDA_HIST_BY_USER_ID with a history but without `users`.  `users` is not read otherwise. */
int pda_calib_profile(const int32_t* users, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode, int n_rows,
                      const uint8_t* item_group, int n_items, int G, int32_t* prof, void* stream);

/* cnt i32 [n_rows, nK, G]: for each cut-off Ks[j] the entries among the first Ks[j] columns of idx i32 [n_rows, K] whose id lies in
 * [0, n_items) and whose item has a group, per group.  Ks is a HOST array of nK cut-offs, strictly ascending, each in 1 .. K; it is copied
 * before the call returns.
 * PDA_ERR_ARG: a NULL idx, item_group, Ks or cnt; n_rows < 1; n_items < 1; K outside 1 .. PDA_CALIB_MAX_N; G outside 2 .. PDA_CALIB_MAX_G;
 * nK outside 1 .. PDA_CALIB_MAX_KS; cut-offs that are not strictly ascending inside 1 .. K. */
int pda_calib_list_counts(const int32_t* idx, int n_rows, int K, const uint8_t* item_group, int n_items, int G, const int32_t* Ks, int nK,
                          int32_t* cnt, void* stream);

/* The greedy selection above.  alpha is read for PDA_CALIB_KL only.
 * PDA_ERR_ARG: a NULL cand_idx, cand_val, prof, item_group, out_idx or out_val; n_rows < 1; n_items < 1; N outside 1 .. PDA_CALIB_MAX_N;
 * K outside 1 .. min(PDA_CALIB_MAX_K, N); G outside 2 .. PDA_CALIB_MAX_G; lambda outside [0, 1] or NaN; a variant other than the two above;
 * PDA_CALIB_KL with alpha outside (0, 1) or NaN. */
int pda_calib_rerank(const int32_t* cand_idx, const float* cand_val, int n_rows, int N, const int32_t* prof, const uint8_t* item_group,
                     int n_items, int G, double lambda, int variant, double alpha, int K, int32_t* out_idx, float* out_val, float* out_div,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_CALIB_H */
