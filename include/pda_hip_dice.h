/* pda_hip_dice.h -- DICE (Zheng et al., WWW'21: interest and conformity embeddings, `--train dice`) on libpda_hip.so.
 *
 * Same conventions as pda_hip.h: device pointers, an explicit `void* stream` (hipStream_t), int return codes (PDA_OK / PDA_ERR_*), and every
 * argument check happens before anything is launched.  Kept in its own header, like pda_hip_temp_pop.h.
 *
 * Model: tables U f32 [n_users, 2d], I f32 [n_items, 2d]; columns [0, d) of a row are the interest embedding, columns
 * [d, 2d) the conformity embedding, so the click score s_int + s_con is the plain dot of two rows (PDA_HEAD_RAW at row width 2d: every
 * evaluation entry point of pda_hip.h serves the model unchanged).  `d` below is always the width of ONE embedding: d in {32, 64, 128}.
 * Per batch of B triplets (u, p, n, m), m = 1 where the negative is the more popular item, ls(x) = log(sigmoid(x) + 1e-10):
 *     x_int = u_int.p_int - u_int.n_int        x_con = u_con.p_con - u_con.n_con
 *     L_click = -mean ls(x_int + x_con)        L_int = -mean m ls(x_int)        L_con = -mean [m ls(-x_con) + (1 - m) ls(x_con)]
 *     L_dis   = dis(I_int[S_i], I_con[S_i]) + dis(U_int[S_u], U_con[S_u])       S_i / S_u: the distinct items / users of the batch
 *     loss    = L_click + w_int L_int + w_con L_con - dis_pen L_dis + regs (l2(u) + l2(p) + l2(n)) / reg_div
 * dis is the mean over the |S| d elements of |a - b| (PDA_DICE_DIS_L1; gradient 0 where a == b) or of (a - b)^2 (PDA_DICE_DIS_L2).
 */
#ifndef PDA_HIP_DICE_H
#define PDA_HIP_DICE_H

#include "pda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PDA_DICE_DIS_L1 0
#define PDA_DICE_DIS_L2 1

/* rows_ws: int32 [pda_dice_rows_ws_words(B)], 16-byte aligned, private to one stream.  Words 0 / 1: |S_u| / |S_i| of the batch seen last
 * (pda_dice_step_f32 zeroes them itself and counts); words from 4 on: the distinct users [B], then the distinct items [2 B]. */
/* Buffer contract -- rows_ws (pda_dice_rows_ws_words): needs no initialisation -- pda_dice_step_f32 clears words 0 .. 3 itself, stream-ordered, and
 * lists a row before pda_dice_dis_f32 reads it; afterwards a caller may read words 0 / 1 (the counts); one rows_ws serves one step (step + dis) at a
 * time. */
size_t pda_dice_rows_ws_words(int B);

/* The batch's gradients of everything except L_dis (a memset of 16 bytes and one launch).  mask u8 [B]: m.  The gradients are SUMMED into
 * gU [n_users, 2d] / gI [n_items, 2d] (duplicates add up); the rows touched get tagU[user] = tagI[pos] = tagI[neg] = step_tag, and the
 * lane group that tags a row first lists it in rows_ws.  A row whose tag already equals step_tag is not listed again: step_tag is a value no
 * earlier call on these tags used (the step number).  loss_acc (optional) f32 [6]: [0 .. 4] += (loss without dis, mf_loss without dis,
 * reg_loss, L_int, L_con); [5] belongs to pda_dice_dis_f32.  A triplet with an id outside the tables is skipped (memory safety only: the
 * callers validate their ids). */
int pda_dice_step_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos,
                      const int32_t* neg, const uint8_t* mask, int B, int d, float w_int, float w_con, float regs, float reg_div, float* gU,
                      float* gI, int32_t* tagU, int32_t* tagI, int step_tag, int32_t* rows_ws, float* loss_acc, void* stream);

/* The L_dis term on the rows pda_dice_step_f32 listed (one launch, row-parallel; the denominators |S| d come from rows_ws): gU / gI +=
 * -dis_pen dL_dis / d(row), loss_acc (optional) [0] and [1] += -dis_pen L_dis, [5] += L_dis.  B: the batch size rows_ws was sized for.  A listed
 * row outside the tables is skipped (memory safety only). */
int pda_dice_dis_f32(const float* U, const float* I, size_t n_users, size_t n_items, int B, int d, int dis_kind, float dis_pen, float* gU,
                     float* gI, const int32_t* rows_ws, float* loss_acc, void* stream);

/* One reference-style train step: pda_dice_step_f32, pda_dice_dis_f32, then TF-1.14's dense-decay Adam over both tables by
 * pda_adam_dense_sweep4_f32 at row width 2d (the sweep of pda_adam_step_f32: g = 0 off the tagged rows, g zeroed behind itself).  Three
 * launches and a 16-byte memset, no host read: capturable in a HIP graph. */
int pda_dice_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI, float* gI,
                           int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg, const uint8_t* mask, int B,
                           int d, float w_int, float w_con, int dis_kind, float dis_pen, float regs, float reg_div, int step_tag, float lr_t,
                           float beta1, float beta2, float eps, int cache_policy, int32_t* rows_ws, float* loss_acc, void* stream);

/* PNSM, DICE's popularity-margin negative sampler.  Users and positives are those of pda_sample_triplets for the same (seed, step, row)
 * (gen_users, user_pool, n_pool, train_indptr, train_indices as there; no time slots).  pop i32 [n_items]: train interactions per item;
 * order i32 [n_items]: the items ascending by (pop, id); sorted_pop i32 [n_items] = pop[order].  With P = (float)pop[pos]:
 *     H = {i : (float)pop[i] > P + margin}   a suffix of order        L = {i : (float)pop[i] < P - margin}   a prefix of order
 * (fp32 arithmetic; both boundaries by binary search in sorted_pop, sizes taken before the user's history is removed).  Both non-empty: bit 31
 * of draw 2 picks H when set; one non-empty: that one; both empty: the negative is drawn from the whole catalogue [0, n_items) and
 * mask = pop[neg] > pop[pos].  Inside the chosen range [lo, lo + span) of order: neg = order[lo + bounded(draw(16 + k), span)], k = 0, 1, ...
 * rejected while neg is a train item of the user, at most 4 096 times (then the last draw stays).  mask u8 [B] = 1 for a negative from H.
 * Draws: draw(seed, step, row, k) of pda_sample.h -- k = 7 the user (B > n_pool), 0 the positive, 2 the side, 16 + k the negatives. */
int pda_dice_sample(int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, const int64_t* train_indptr,
                    const int32_t* train_indices, int n_items, const int32_t* order, const int32_t* sorted_pop, const int32_t* pop, float margin,
                    uint64_t seed, uint64_t step, int32_t* pos, int32_t* neg, uint8_t* mask, void* stream);

/* The same with the step and the margin read from device memory (HIP-graph replay: the margin's decay needs no re-capture); step_next
 * (optional, a different location than step_dev) receives *step_dev + 1, as in pda_sample_triplets_dev. */
int pda_dice_sample_dev(int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, const int64_t* train_indptr,
                        const int32_t* train_indices, int n_items, const int32_t* order, const int32_t* sorted_pop, const int32_t* pop,
                        const float* margin_dev, uint64_t seed, const uint64_t* step_dev, uint64_t* step_next, int32_t* pos, int32_t* neg,
                        uint8_t* mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_DICE_H */
