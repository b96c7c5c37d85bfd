/* pda_hip_negpop.h -- popularity-weighted negative sampling (`--neg_sampler pop`: negatives drawn with q_i ~ (c_i + 1)^beta, the unigram^0.75
 * sampler of word2vec and the popularity-oversampled negatives of the BPR line of work) on libpda_hip.so.
 *
 * Same conventions as pda_hip.h: device pointers, an explicit `void* stream` (hipStream_t), int return codes (PDA_OK / PDA_ERR_*), every argument
 * check happens before anything is launched, nothing is allocated.  Kept in its own header, like pda_hip_dns.h.
 *
 * The calls are the uniform samplers (pda_sample_triplets, pda_sample_triplets_dev, pda_sample_batches_dev of pda_hip.h; pda_ssm_sample,
 * pda_ssm_sample_dev of pda_hip_ssm.h) with ONE thing changed: where they draw a negative uniformly from [neg_lo, neg_hi), these draw it from an
 * alias table over that range.
 *
 * The table: alias u64 [n], n = neg_hi - neg_lo, one 8-byte load per try.  Low word: thr, a u32 threshold; high word: other, a u32 slot in [0, n).
 *     A slot with other == slot keeps its whole mass (thr is not looked at).  Slot s is therefore kept with probability thr / 2^32 and hands the
 *     rest to `other`; how the caller fills it from a distribution (Vose's method in pda_amd.ops.NegPopTable) is not this library's business.
 * User, positive, time slot of row r: those of pda_sample_triplets for the same (seed, step, r) -- gen_users, user_pool and the empty train row
 *     (positive 0, the slot drawn from [0, n_slots)) included; the same device functions draw them.
 * Try a (0 <= a < 4096) of negative j of row r, with k = 16 + 4096 j + a the draw number the uniform samplers use:
 *     slot = bounded(draw(seed, step, r, k), n)
 *     coin = draw(seed, step, r, 0x80000000 | k)
 *     x    = (other[slot] == slot || coin < thr[slot]) ? slot : other[slot]
 *     item = neg_lo + x
 *     rejected while it is a train item of the user (binary search in the sorted row); after 4096 tries the last draw stays.
 * A table whose slots all keep their mass draws, bit for bit, what the uniform twin draws on the same arguments.
 * Memory safety: `other` is an index the kernels add to neg_lo and look up in the train row (a search that reads the row only) and, with
 *     popularity columns, in pop_matrix.  Slots outside [0, n) are the caller's to refuse, as item ids of the train CSR are for
 *     pda_sample_triplets; pda_amd.ops validates every table before it is uploaded.
 * The calls are functions of their arguments alone, bit for bit: no atomics, no order left to the scheduler.
 */
#ifndef PDA_HIP_NEGPOP_H
#define PDA_HIP_NEGPOP_H

#include "pda_hip.h"
#include "pda_hip_ssm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pda_sample_triplets with the table: one thread per row.  Writes users (gen_users != 0), pos, neg and, with pop_matrix, pos_pop / neg_pop; reads
 * train_slots (or NULL: slot 0) and pop_matrix f32 [n_items, n_slots].  PDA_ERR_ARG: alias NULL, and whatever pda_sample_triplets refuses. */
int pda_negpop_sample_triplets(int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, const int64_t* train_indptr,
                               const int32_t* train_indices, const int32_t* train_slots, int neg_lo, int neg_hi, const uint64_t* alias,
                               const float* pop_matrix, int n_slots, uint64_t seed, uint64_t step, int32_t* pos, int32_t* neg, float* pos_pop,
                               float* neg_pop, void* stream);

/* The same with the step taken from DEVICE memory (*step_dev) and, where step_next is given (a DIFFERENT location), *step_dev + 1 stored there:
 * the protocol of pda_sample_triplets_dev.  PDA_ERR_ARG besides: step_dev NULL, step_next == step_dev. */
int pda_negpop_sample_triplets_dev(int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, const int64_t* train_indptr,
                                   const int32_t* train_indices, const int32_t* train_slots, int neg_lo, int neg_hi, const uint64_t* alias,
                                   const float* pop_matrix, int n_slots, uint64_t seed, const uint64_t* step_dev, uint64_t* step_next,
                                   int32_t* pos, int32_t* neg, float* pos_pop, float* neg_pop, void* stream);

/* n_batches (1 .. 65535) batches in ONE launch into [n_batches][B] buffers: row j is, bit for bit, what pda_negpop_sample_triplets_dev draws with
 * step *step_dev + j; step_next (a DIFFERENT location, or NULL) receives *step_dev + n_batches -- the two-slot counter protocol of
 * pda_sample_batches_dev, without its grouping by positive. */
int pda_negpop_sample_batches_dev(int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, int n_batches,
                                  const int64_t* train_indptr, const int32_t* train_indices, const int32_t* train_slots, int neg_lo, int neg_hi,
                                  const uint64_t* alias, const float* pop_matrix, int n_slots, uint64_t seed, const uint64_t* step_dev,
                                  uint64_t* step_next, int32_t* pos, int32_t* neg, float* pos_pop, float* neg_pop, void* stream);

/* pda_ssm_sample with the table: negs i32 [B, N], 1 <= N <= PDA_SSM_MAX_NEGS, B <= 2^22, one thread per (row, j); column 0 is, bit for bit, the
 * negative of pda_negpop_sample_triplets.  PDA_ERR_ARG: alias NULL, and whatever pda_ssm_sample refuses. */
int pda_negpop_ssm_sample(int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, int N, const int64_t* train_indptr,
                          const int32_t* train_indices, int neg_lo, int neg_hi, const uint64_t* alias, uint64_t seed, uint64_t step, int32_t* pos,
                          int32_t* negs, void* stream);

/* The same with the step taken from device memory: the protocol of pda_ssm_sample_dev. */
int pda_negpop_ssm_sample_dev(int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, int N, const int64_t* train_indptr,
                              const int32_t* train_indices, int neg_lo, int neg_hi, const uint64_t* alias, uint64_t seed,
                              const uint64_t* step_dev, uint64_t* step_next, int32_t* pos, int32_t* negs, void* stream);

/* The sampled-softmax step under a logQ correction: pda_ssm_step_f32 and pda_ssm_adam_step_f32 (pda_hip_ssm.h, whose contract holds in every other
 * respect) with one more argument, logq f32 [n_items], log q_i of the distribution the negatives were drawn from:
 *     s_k = (u . i_k) / tau - logq[item_k]      (norm == 1: u^ . i^_k)      for EVERY k = 0 .. N, the positive's own logit included
 * -- the convention of pda_hip_inbatch.h.  logq is read at the N + 1 item ids of a valid row only and has no gradient; the loss, the gradients,
 * the tags, the flags and the errors are those of the two calls with these logits.  logq NULL: no correction, the two calls themselves (they are
 * these with NULL).  Declared here, beside the proposal it corrects for; the kernel is a template flag of the step kernel of pda_ssm.hip, so the
 * existing entries keep their instantiation. */
int pda_ssm_step_logq_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos,
                          const int32_t* negs, const float* logq, int B, int N, int d, float tau, int norm, float regs, float reg_div, float* gU,
                          float* gI, int32_t* tagU, int32_t* tagI, int step_tag, int flags, float* loss_acc, void* stream);
int pda_ssm_adam_step_logq_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI, float* gI,
                               int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* negs, const float* logq,
                               int B, int N, int d, float tau, int norm, float regs, float reg_div, int step_tag, float lr_t, float beta1,
                               float beta2, float eps, int flags, int cache_policy, float* loss_acc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_NEGPOP_H */
