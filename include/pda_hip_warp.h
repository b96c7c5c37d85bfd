/* pda_hip_warp.h -- the WARP loss (`--train warp`: Weston, Bengio, Usunier, "WSABIE: Scaling Up To Large Vocabulary Image Annotation", IJCAI'11;
 * the ranking loss of LightFM) on libpda_hip.so: a margin-based, rank-weighted pairwise loss whose negative is the FIRST of a stream of uniform
 * candidates that violates the margin, the number of draws it took estimating the positive's rank.
 *
 * Same conventions as pda_hip_dns.h and pda_hip_ips.h: device pointers, an explicit `void* stream` (hipStream_t), int return codes (PDA_OK /
 * PDA_ERR_*), every argument check happens before anything is launched, nothing is allocated.  Kept in its own header.
 *
 * Model: the tables of a BPRMF, U f32 [n_users, d], I f32 [n_items, d], d in {32, 64, 128, 256}; only the raw head.  A WARP model
 * differs from a BPRMF only in how it was trained, and every evaluation entry point of pda_hip.h serves it unchanged (PDA_HEAD_RAW).
 *
 * ---- the draw (pda_warp_sample_f32): row r of a batch of B
 * User, positive, time slot: those of pda_sample_triplets for the same (seed, step, r) -- gen_users, user_pool, the empty train row (positive 0,
 *     the slot drawn from [0, n_slots)) and neg_lo / neg_hi included; the same device functions draw them.
 * Candidates: candidate j (0 <= j < T, 1 <= T <= PDA_WARP_MAX_TRIALS) of row r is column j of pda_ssm_sample (pda_hip_ssm.h): attempt a
 *     (0 <= a < 4096) is neg_lo + bounded(draw(seed, step, r, 16 + 4096 j + a), neg_hi - neg_lo), rejected while it is a train item of the user;
 *     after 4096 attempts the last draw stays.  Candidates are drawn with replacement, exactly as the DNS candidates are.
 * Scores: s_p = u . I[pos], s_j = u . I[c_j], u = U[user], all by the ONE fp32 code path of pda_hip_dns.h: lane e of an item's d / 4 lanes
 *     multiplies elements 4 e .. 4 e + 3 and adds them in that order, the lanes add by the xor ladder (offsets d / 8, d / 16, .. 1).  Equal items
 *     have equal bits, the positive included.
 * Violation: x_j = s_p - s_j is one fp32 subtraction; candidate j VIOLATES iff margin - x_j > 0 in fp32.  A NaN (in s_p, s_j or margin - x_j)
 *     never violates.
 * N_r = 1 + the column of the first violator, 0 when none of the T candidates violates.
 *     neg[r]    = the first violator; without one, candidate T - 1
 *     trials[r] = N_r
 *     coef[r]   = N_r > 0 ? wtab[N_r] : 0
 *     pos_pop[r] = pop[pos[r] * n_slots + slot], neg_pop[r] = pop[neg[r] * n_slots + slot], as pda_sample_triplets writes them, when asked for.
 * wtab f32 [T + 1]: a device table the CALLER builds; the kernel knows nothing of ranks or logarithms.  pda_amd.ops.WarpWeights builds, on the host in
 *     float64 and rounded once to fp32, with rank(N) = floor((n_eligible - 1) / N), n_eligible = neg_hi - neg_lo:
 *         "harmonic": wtab[N] = sum_{k = 1 .. rank(N)} 1 / k   (WSABIE)      "log": wtab[N] = log(max(1, rank(N)))   (LightFM; 0 at rank 1)
 *         "none":     wtab[N] = 1   (the plain hinge on the first violator)   and wtab[0] = 0 always.
 * Memory safety: a row whose user id lies outside [0, n_users) -- possible only for user ids the caller supplies, directly or through user_pool --
 *     reads no table row and no train row: it is drawn as a user without train items, its scores (pos_score too) are 0, no candidate violates:
 *     trials 0, coef 0, and neg[r] is candidate 0 (not candidate T - 1).  Item ids of the train CSR are the caller's to validate.
 * Test outputs (optional): cand i32 [B, T] and cand_score f32 [B, T]: columns j < N_r hold the candidates and their scores (all T columns when
 *     N_r == 0); every other column holds -1 and 0.f, whatever the kernel actually scored.  pos_score f32 [B] = s_p.
 * stat (optional) i64 [2] += (sum of N_r over the rows with a violator, number of rows without one): integer adds, one pair per workgroup after
 *     the workgroup has reduced its rows, so the sums are the same bits in any order.
 * T == 1, margin = +inf and wtab[1] = 1 reproduce pda_sample_triplets bit for bit in users, pos, neg, pos_pop, neg_pop, with coef == 1 on every row
 *     of a known user (finite tables).
 * The call is a function of its arguments alone, bit for bit: no float atomics, no order left to the scheduler (the first violator of a row is a
 *     minimum over integers).  It does not depend on what its output buffers held: every element of every output but stat is written.
 *
 * ---- the step (pda_warp_step_f32): triplet t of a batch of B, coef f32 [B] as the draw wrote it
 *     x_t = u.p - u.n (the raw dots, recomputed on the tables the step is given: the sampler's decision is not trusted)      h_t = margin - x_t
 *     active_t iff coef_t > 0 && h_t > 0
 *     mf   = (1 / B) sum_{active} coef_t h_t                        d mf / d x_t = -coef_t / B when active, else 0
 *     reg  = regs (l2(u) + l2(p) + l2(n)) / reg_div                 over every valid triplet as pda_bpr_step_f32 takes it: an inactive triplet
 *                                                                   still regularises its three rows
 *     loss = mf + reg
 * The step is the gradient of the stated loss.  A triplet with an id outside the tables is skipped: it adds nothing.
 */
#ifndef PDA_HIP_WARP_H
#define PDA_HIP_WARP_H

#include "pda_hip.h"

#define PDA_WARP_MAX_TRIALS 256

#ifdef __cplusplus
extern "C" {
#endif

/* ONE launch: a workgroup of 512 threads owns a few whole rows and runs ROUNDS: each round draws (a thread each) and scores (d / 4 lanes each, four
 * gathered item rows in flight per lane group) the next C candidates of every row of the workgroup that is still open; a row closes at its first
 * violator and draws nothing more; the workgroup leaves the loop when all its rows are closed or T is reached.
 *   users       i32 [B]: written when gen_users != 0 (drawn from user_pool i32 [n_pool], or from [0, n_pool) when user_pool is NULL), read otherwise
 *   train_*     the train CSR: indptr i64 [n_users + 1], indices i32 (ascending inside a row), slots i32 per entry or NULL (slot 0)
 *   pop         f32 [n_items, n_slots] or NULL; required for pos_pop / neg_pop (the scores never read it)
 *   wtab        f32 [T + 1]
 *   pos, neg, trials   i32 [B];   coef f32 [B]
 *   pos_pop, neg_pop   f32 [B], both or neither (NULL)
 *   cand i32 [B, T], cand_score f32 [B, T], pos_score f32 [B], stat i64 [2]: each optional (NULL)
 * PDA_ERR_ARG: U, I, users, train_indptr, train_indices, wtab, pos, neg, trials or coef NULL; gen_users with n_pool <= 0; B outside 1 .. 2^22;
 * tables without rows or with more than 2^31 - 1; T outside 1 .. PDA_WARP_MAX_TRIALS; margin NaN; neg_hi <= neg_lo or [neg_lo, neg_hi) not inside
 * [0, n_items); pop with n_slots <= 0; one of pos_pop / neg_pop without the other, or both without pop.  PDA_ERR_UNSUPPORTED: d. */
int pda_warp_sample_f32(const float* U, const float* I, size_t n_users, size_t n_items, int d, int32_t* users, int gen_users,
                        const int32_t* user_pool, int n_pool, int B, const int64_t* train_indptr, const int32_t* train_indices,
                        const int32_t* train_slots, const float* pop, int n_slots, int neg_lo, int neg_hi, int T, float margin, const float* wtab,
                        uint64_t seed, uint64_t step, int32_t* pos, int32_t* neg, int32_t* trials, float* coef, float* pos_pop, float* neg_pop,
                        int32_t* cand, float* cand_score, float* pos_score, int64_t* stat, void* stream);

/* The same with the step taken from DEVICE memory (*step_dev) and, where step_next is given (a DIFFERENT location), *step_dev + 1 stored there:
 * the protocol of pda_dns_sample_f32_dev.  PDA_ERR_ARG besides: step_dev NULL, step_next == step_dev. */
int pda_warp_sample_f32_dev(const float* U, const float* I, size_t n_users, size_t n_items, int d, int32_t* users, int gen_users,
                            const int32_t* user_pool, int n_pool, int B, const int64_t* train_indptr, const int32_t* train_indices,
                            const int32_t* train_slots, const float* pop, int n_slots, int neg_lo, int neg_hi, int T, float margin,
                            const float* wtab, uint64_t seed, const uint64_t* step_dev, uint64_t* step_next, int32_t* pos, int32_t* neg,
                            int32_t* trials, float* coef, float* pos_pop, float* neg_pop, int32_t* cand, float* cand_score, float* pos_score,
                            int64_t* stat, void* stream);

/* The batch's gradients (one launch, the layout of pda_ips_step_f32: d / 4 lanes per triplet).  The gradients are SUMMED into gU [n_users, d] /
 * gI [n_items, d] (duplicates add up; equal positives inside a workgroup are combined on chip first); the rows touched -- those of inactive
 * triplets too, they carry the regulariser -- get tagU[user] = tagI[pos] = tagI[neg] = step_tag, exactly as pda_adam_step_f32 tags them.
 * flags: PDA_UPD_ANY_ORDER (the batch is not grouped by positive) | PDA_UPD_USERS_DISTINCT (no user id occurs twice: its gU row, zero before the
 * call, takes a plain store).  loss_acc (optional) f32 [3] += (loss, mf, reg).
 * PRECONDITION of PDA_UPD_USERS_DISTINCT, as for pda_adam_step_f32 (pda_hip.h): the plain store is the row's gradient only if gU is zero on every
 * row the batch touches and no user occurs twice.  The sweep of pda_warp_adam_step_f32 zeroes what the step wrote; a non-OK return between the
 * step and the sweep leaves gU / gI and the tags dirty, and the caller zeroes them before going on.
 * PDA_ERR_ARG: a NULL among U, I, users, pos, neg, coef, gU, gI, tagU, tagI; B outside 1 .. 2^28; reg_div <= 0; step_tag <= 0; margin NaN; tables
 * without rows; unknown flags.  PDA_ERR_UNSUPPORTED: d. */
int pda_warp_step_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg,
                      const float* coef, float margin, int B, int d, float regs, float reg_div, float* gU, float* gI, int32_t* tagU, int32_t* tagI,
                      int step_tag, int flags, float* loss_acc, void* stream);

/* One train step: pda_warp_step_f32, then TF-1.14's dense-decay Adam over both tables by pda_adam_dense_sweep4_f32 (the sweep of
 * pda_adam_step_f32: g = 0 off the tagged rows, g zeroed behind itself).  Two launches, no host read: capturable in a HIP graph.  flags and
 * cache_policy: those of pda_adam_step_f32. */
int pda_warp_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI, float* gI,
                           int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg, const float* coef,
                           float margin, int B, int d, float regs, float reg_div, int step_tag, float lr_t, float beta1, float beta2, float eps,
                           int flags, int cache_policy, float* loss_acc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_WARP_H */
