/* pda_hip_dns.h -- dynamic hard-negative sampling (`--neg_sampler dns`: DNS, Zhang et al., "Optimizing Top-N Collaborative Filtering via Dynamic
 * Negative Item Sampling", SIGIR'13; the DNS(M, N) form of Shi et al., "On the Theories Behind Hard Negative Sampling for Recommendation", WWW'23)
 * on libpda_hip.so.
 *
 * Same conventions as pda_hip.h: device pointers, an explicit `void* stream` (hipStream_t), int return codes (PDA_OK / PDA_ERR_*), every argument
 * check happens before anything is launched, nothing is allocated.  Kept in its own header, like pda_hip_ssm.h.
 *
 * The call draws the triplet batch of pda_sample_triplets, except that the negative of a row is one of the `topn` best-scoring of M uniform
 * candidates under the CURRENT tables U f32 [n_users, d], I f32 [n_items, d], d in {32, 64, 128, 256}.
 *
 * User, positive, time slot of row r: those of pda_sample_triplets for the same (seed, step, r) -- gen_users, user_pool, the empty train row
 *     (positive 0, the slot drawn from [0, n_slots)) and neg_lo / neg_hi included; the same device functions draw them.
 * Candidates: candidate j (0 <= j < M, 1 <= M <= PDA_DNS_MAX_CANDIDATES) of row r is column j of pda_ssm_sample (pda_hip_ssm.h): attempt a
 *     (0 <= a < 4096) is neg_lo + bounded(draw(seed, step, r, 16 + 4096 j + a), neg_hi - neg_lo), rejected while it is a train item of the user;
 *     after 4096 attempts the last draw stays.  Candidates are drawn with replacement: duplicates occur.
 * Score of candidate j, c_j its item, u = U[user], i_j = I[c_j]:
 *     PDA_HEAD_RAW:  s_j = u . i_j
 *     PDA_HEAD_POP:  s_j = (elu(u . i_j) + 1) * pop[c_j * n_slots + slot]     (elu(x) + 1 = x > 0 ? x + 1 : expf(x), as the step kernels take it;
 *                                                                              slot: the time slot of the row's positive)
 *     in fp32: lane e of the candidate's d / 4 lanes multiplies elements 4 e .. 4 e + 3 and adds them in that order, the lanes add by the xor
 *     ladder (offsets d / 8, d / 16, .. 1).  One code path scores every candidate: equal items have equal bits in every column of a row.
 * Order of a row's candidates: score descending, then column ascending; a NaN score ranks behind every number, NaNs among themselves by column.
 * Pick: t = bounded(draw(seed, step, r, 3), min(topn, M)); topn == 1 draws nothing (t = 0: the classic DNS, the best of M).  neg[r] is the
 *     candidate at position t of the order, pick_col[r] its column, neg_pop[r] = pop[neg[r] * n_slots + slot] and pos_pop[r] =
 *     pop[pos[r] * n_slots + slot] as pda_sample_triplets writes them.
 * M == 1 reproduces pda_sample_triplets bit for bit in users, pos, neg, pos_pop and neg_pop (no table row is read then unless cand_score is asked).
 * Memory safety: a row whose user id lies outside [0, n_users) -- possible only for user ids the caller supplies, directly or through user_pool --
 *     reads no table row and no train row: it is drawn as a user without train items, its scores are 0 and it takes candidate 0.  Item ids of the
 *     train CSR are the caller's to validate, as for pda_sample_triplets.
 * The call is a function of its arguments alone, bit for bit: no atomics, no order left to the scheduler.
 */
#ifndef PDA_HIP_DNS_H
#define PDA_HIP_DNS_H

#include "pda_hip.h"

#define PDA_DNS_MAX_CANDIDATES 256

#ifdef __cplusplus
extern "C" {
#endif

/* ONE launch: a workgroup of 512 threads owns a few whole rows (at most 512 candidates; as a rule the 8192 / d candidates its lane groups score
 * in one round); it draws their candidates (a thread each), scores them (d / 4 lanes each, four gathered item rows in flight per lane group)
 * and selects (a thread per candidate counts the candidates of its row ahead of it in the order; the one that counts t writes the row's outputs).
 *   users       i32 [B]: written when gen_users != 0 (drawn from user_pool i32 [n_pool], or from [0, n_pool) when user_pool is NULL), read otherwise
 *   train_*     the train CSR: indptr i64 [n_users + 1], indices i32 (ascending inside a row), slots i32 per entry or NULL (slot 0)
 *   pop         f32 [n_items, n_slots] or NULL; required for PDA_HEAD_POP and for pos_pop / neg_pop
 *   pos, neg    i32 [B]
 *   pos_pop, neg_pop   f32 [B], both or neither (NULL)
 *   cand        i32 [B, M] or NULL: the candidates;  cand_score f32 [B, M] or NULL: their scores;  pick_col i32 [B] or NULL
 * PDA_ERR_ARG: U, I, users, train_indptr, train_indices, pos or neg NULL; gen_users with n_pool <= 0; B outside 1 .. 2^22; tables without rows or
 * with more than 2^31 - 1; M outside 1 .. PDA_DNS_MAX_CANDIDATES; topn outside 1 .. M; neg_hi <= neg_lo or [neg_lo, neg_hi) not inside
 * [0, n_items); head neither PDA_HEAD_RAW nor PDA_HEAD_POP; PDA_HEAD_POP without pop; pop with n_slots <= 0; one of pos_pop / neg_pop without the
 * other, or both without pop.  PDA_ERR_UNSUPPORTED: d. */
int pda_dns_sample_f32(const float* U, const float* I, size_t n_users, size_t n_items, int d, int32_t* users, int gen_users,
                       const int32_t* user_pool, int n_pool, int B, const int64_t* train_indptr, const int32_t* train_indices,
                       const int32_t* train_slots, const float* pop, int n_slots, int neg_lo, int neg_hi, int M, int topn, int head, uint64_t seed,
                       uint64_t step, int32_t* pos, int32_t* neg, float* pos_pop, float* neg_pop, int32_t* cand, float* cand_score,
                       int32_t* pick_col, void* stream);

/* The same with the step taken from DEVICE memory (*step_dev) and, where step_next is given (a DIFFERENT location), *step_dev + 1 stored there:
 * the protocol of pda_sample_triplets_dev.  PDA_ERR_ARG besides: step_dev NULL, step_next == step_dev. */
int pda_dns_sample_f32_dev(const float* U, const float* I, size_t n_users, size_t n_items, int d, int32_t* users, int gen_users,
                           const int32_t* user_pool, int n_pool, int B, const int64_t* train_indptr, const int32_t* train_indices,
                           const int32_t* train_slots, const float* pop, int n_slots, int neg_lo, int neg_hi, int M, int topn, int head,
                           uint64_t seed, const uint64_t* step_dev, uint64_t* step_next, int32_t* pos, int32_t* neg, float* pos_pop, float* neg_pop,
                           int32_t* cand, float* cand_score, int32_t* pick_col, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_DNS_H */
