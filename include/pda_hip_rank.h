/* pda_hip_rank.h -- exact full-catalogue ranks of chosen (user, item) pairs on libpda_hip.so: where a held-out item stands in the user's masked
 * ranking of ALL items, without the [users, items] rating matrix and without a list (`--rank_report 1`: AUC, MRR, percentile rank).
 *
 * Same conventions as pda_hip_deep.h: device pointers, caller-owned buffers, an explicit `void* stream` (hipStream_t), int return codes
 * (PDA_OK / PDA_ERR_*), every argument check happens before anything is launched, no call allocates, and there is no workspace.
 *
 * Contract ("5q. Ranks of held-out items"):
 *   scores   the exact fp32 chain of pda_score_dense_f32 / pda_deep_topk_f32 (v_mfma_f32_32x32x2_f32, two chains added once, k = 8c + 4h + s):
 *            the head value of a pair equals, bit for bit, what those give for it.  Heads PDA_HEAD_RAW and PDA_HEAD_POP.
 *   order    packed keys as in pda_hip.h: orderable_bits(value) << 32 | (0xFFFFFFFF - global item id) -- value descending, id ascending
 *   ranks    an item RANKS for a user iff it lies in the shard, is not in the user's history row (CSR sorted ascending, duplicates allowed,
 *            PDA_HIST_BY_BLOCK_ROW / PDA_HIST_BY_USER_ID) and its head value is > -inf (NaN and -inf never rank, as in the lists)
 *   targets  a CSR by block row: tgt_indptr i64 [n_users_blk + 1], tgt_indices i32 global item ids; rows may be unsorted, hold duplicates or
 *            be empty; an id outside the shard (or outside the catalogue) is skipped
 *   d in {32, 64, 128, 256}, else PDA_ERR_UNSUPPORTED
 *
 * Two calls, because over item shards counts add and keys combine by maximum (a pair's key is non-zero on one shard at most):
 *   pda_rank_keys_*    tgt_keys[e] = the packed key of entry e if its item ranks for its user, else 0 -- for every entry whose id lies in
 *                      [item_offset, item_offset + n_items_local).  Other entries are NOT written: the caller zero-fills once.
 *   pda_rank_count_*   above[e] += the number of ranking items of this shard whose key is > tgt_keys[e], for every entry with a non-zero key
 *                      (zero keys are left alone);  n_ranked[r] += the number of ranking items of this shard for block row r.
 *                      Both i32 and ADDED to: summed over the shards, above[e] is the entry's 0-based rank and n_ranked[r] the length of
 *                      the row's ranking.  Integer adds only: the same bits whatever the geometry, from run to run, with or without splits.
 *                      n_splits cuts the item range into that many workgroups per 128 users; 0: the call chooses; < 0: PDA_ERR_ARG.
 *                      max_tgt_row: the longest target row, or any upper bound of it (the caller built the CSR); a row's keys are taken
 *                      PDA_RANK_TCHUNK at a time, one sweep of launches per chunk, and workgroups without a target in a chunk return at
 *                      once.  max_tgt_row = 0: one sweep that only counts n_ranked.  Entries behind max_tgt_row in a row are not counted.
 */
#ifndef PDA_HIP_RANK_H
#define PDA_HIP_RANK_H

#include "pda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PDA_RANK_TCHUNK 32

int pda_rank_keys_f32(const float* U, const float* I_shard, const float* pop_shard, const int32_t* users, int n_users_blk, int item_offset,
                      int n_items_local, int d, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode,
                      const int64_t* tgt_indptr, const int32_t* tgt_indices, int head, uint64_t* tgt_keys, void* stream);

/* The same on bf16 tables (U, I_shard: bf16 bit patterns), rows widened to fp32 on load: identical to the fp32 call on the widened tables. */
int pda_rank_keys_bf16(const uint16_t* U, const uint16_t* I_shard, const float* pop_shard, const int32_t* users, int n_users_blk,
                       int item_offset, int n_items_local, int d, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode,
                       const int64_t* tgt_indptr, const int32_t* tgt_indices, int head, uint64_t* tgt_keys, void* stream);

int pda_rank_count_f32(const float* U, const float* I_shard, const float* pop_shard, const int32_t* users, int n_users_blk, int item_offset,
                       int n_items_local, int d, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode,
                       const int64_t* tgt_indptr, const uint64_t* tgt_keys, int max_tgt_row, int head, int n_splits, int32_t* above,
                       int32_t* n_ranked, void* stream);

int pda_rank_count_bf16(const uint16_t* U, const uint16_t* I_shard, const float* pop_shard, const int32_t* users, int n_users_blk,
                        int item_offset, int n_items_local, int d, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode,
                        const int64_t* tgt_indptr, const uint64_t* tgt_keys, int max_tgt_row, int head, int n_splits, int32_t* above,
                        int32_t* n_ranked, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_RANK_H */
