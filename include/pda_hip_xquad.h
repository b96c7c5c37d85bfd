/* pda_hip_xquad.h -- xQuAD (personalised popularity re-ranking, Abdollahpouri, Burke and Mobasher, FLAIRS 2019) on libpda_hip.so: the greedy
 * selection of K items out of a user's N candidates, two item categories (short head, long tail), one launch, one wave per user.
 *
 * Same conventions as pda_hip.h: device pointers, caller-owned buffers, an explicit `void* stream` (hipStream_t), int return codes
 * (PDA_OK / PDA_ERR_*), and every argument check happens before anything is launched.  Kept in its own header, like pda_hip_pc.h.
 *
 * Contract ("5e. xQuAD"), per row (user); RN32 = rounding to fp32, every operation below a separate fp32 operation, `/` the
 * correctly rounded fp32 division:
 *   candidates  cand_idx i32 [n_rows, N], cand_val f32 [n_rows, N]: what pda_score_topk_* / pda_deep_topk_* / pda_deep_merge write.
 *               The valid prefix ends before the first position whose id is outside [0, n_items) or whose value is not finite (-1, the
 *               -inf completion of a short row, NaN); n_valid is its length.
 *               Preconditions: the values do not increase over the valid prefix, and no valid position follows an invalid one (the end of
 *               the prefix is searched for, the row is not streamed).  On a list that breaks one of them the result is unspecified, but every
 *               access stays in bounds.
 *   categories  item_is_head u8 [n_items]: non-zero = short head (category 1), zero = long tail (category 0).
 *   profile     the user's history row (CSR of pda_hip.h: rows sorted, duplicates counted once, PDA_HIST_BY_BLOCK_ROW /
 *               PDA_HIST_BY_USER_ID; hist_indptr NULL = no profile; ids outside [0, n_items) ignored).  H = its distinct valid entries,
 *               H1 = those that are head:  q_1 = RN32(H1 / H), q_0 = RN32((H - H1) / H) (H, H1 as fp32: exact below 2^24);  H = 0: q_0 = q_1 = 0.
 *   weights     L = RN32(lambda), W = RN32(1 - lambda) (the subtraction in double), 0 <= lambda <= 1.
 *   relevance   lo = val[n_valid - 1], rng = RN32(val[0] - lo), p_v = RN32(RN32(val[v] - lo) / rng);  p_v = 0 when rng is 0 or not finite.
 *   selection   S empty, n_c = picks of category c, t = |S|; min(K, n_valid) times:
 *                 PDA_XQUAD_BINARY  cov_c = 1 if n_c == 0, else 0
 *                 PDA_XQUAD_SMOOTH  cov_c = 1 if t == 0, else RN32(1 - RN32(n_c / t))      (one factor per category)
 *                 x_v = RN32(RN32(W p_v) + RN32(L RN32(q_c cov_c))) for every unpicked candidate v of category c;
 *                 the largest x_v is picked, ties go to the smallest position in the candidate list.
 *   result      out_idx i32 [n_rows, K] the picks in order, out_val f32 [n_rows, K] = x at the moment of the pick; slots behind
 *               min(K, n_valid) hold -1 and -inf.
 *   No workspace, no allocation, no synchronisation, no float atomics: the same bits whatever the launch geometry.
 */
#ifndef PDA_HIP_XQUAD_H
#define PDA_HIP_XQUAD_H

#include "pda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PDA_XQUAD_MAX_K 64      /* the columns pda_metrics takes */
#define PDA_XQUAD_MAX_N 1024    /* = PDA_DEEP_MAX_K */
#define PDA_XQUAD_BINARY 0
#define PDA_XQUAD_SMOOTH 1

/* PDA_ERR_ARG: a NULL cand_idx, cand_val, item_is_head, out_idx or out_val; n_rows < 1; n_items < 1; N outside 1 .. PDA_XQUAD_MAX_N;
 * K outside 1 .. min(PDA_XQUAD_MAX_K, N); lambda outside [0, 1] or NaN; a variant other than the two above; a history without its indices
 * or with another row mode; PDA_HIST_BY_USER_ID with a history but without `users`.  `users` is not read otherwise. */
int pda_xquad_rerank(const int32_t* cand_idx, const float* cand_val, int n_rows, int N, const uint8_t* item_is_head, int n_items,
                     const int32_t* users, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode,
                     double lambda, int variant, int K, int32_t* out_idx, float* out_val, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_XQUAD_H */
