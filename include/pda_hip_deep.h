/* pda_hip_deep.h -- deep lists on libpda_hip.so: exact score + history mask + top-K for K up to 1 024, and metrics on lists that long.
 *
 * Same conventions as pda_hip.h: device pointers, caller-owned buffers, an explicit `void* stream` (hipStream_t), int return codes
 * (PDA_OK / PDA_ERR_*), every argument check happens before anything is launched, and no call allocates.  Kept in its own header, like
 * pda_hip_temp_pop.h and pda_hip_pc.h.
 *
 * Contract ("5d. Deep lists"):
 *   scores   the exact fp32 chain of pda_score_topk_f32 / pda_score_dense_f32 (v_mfma_f32_32x32x2_f32, two chains added once): a value
 *            returned here equals, bit for bit, what those give for the same (user, item) pair.  Heads PDA_HEAD_RAW and PDA_HEAD_POP.
 *   order    (value descending, global item id ascending); packed keys as in pda_hip.h: orderable_bits(score) << 32 | (0xFFFFFFFF - item)
 *   history  CSR rows sorted ascending (duplicates allowed, counted once), PDA_HIST_BY_BLOCK_ROW / PDA_HIST_BY_USER_ID; a listed item is
 *            worth -inf.  A row with fewer than K unlisted items is completed with its listed items of this shard, lowest id first,
 *            value -inf, key 0 (tf.nn.top_k on the masked row); slots that stay empty behind those hold id -1.
 *   NaN      an item whose head value is NaN (NaN popularity) never ranks.
 *   d in {32, 64, 128, 256}, else PDA_ERR_UNSUPPORTED;  1 <= K <= min(PDA_DEEP_MAX_K, n_items_local), else PDA_ERR_ARG;
 *   a workspace smaller than pda_deep_topk_workspace_bytes says: PDA_ERR_WORKSPACE.  The workspace is 16-byte aligned.
 *   Behind the call: workspace + 16 the identity word  8 << 28 | bf16 << 14 | head << 13 | d / 64  (generation 8 = the deep path).
 *
 * Item shards ("Deep lists on item shards"): every shard runs pda_deep_topk_* on its rows with min(K, n_items_local) columns and
 * out_keys alone, the lists are exchanged, and pda_deep_merge merges them -- pda_topk_merge's contract for 1 <= K <= PDA_DEEP_MAX_K:
 *   in       u64 [R, n_users_blk, K]; every list best first, 0 = an empty slot, zeros only behind a list's last key; the non-zero keys of a
 *            row are distinct across its lists (a precondition: the shards are disjoint)
 *   out      the K largest keys of the row's union, descending, as out_keys and / or out_idx + out_val; a slot that stays empty holds key 0
 *            and value -inf.  With out_idx, empty slots take the user's WHOLE history row (hist_indptr != NULL; PDA_HIST_BY_USER_ID needs
 *            `users`), lowest id first, duplicates once, then -1 -- what a one-GPU pda_deep_topk_* call writes; without a history -1.
 *   errors   R < 1, K outside 1 .. PDA_DEEP_MAX_K, n_users_blk < 1, in_keys NULL, out_keys and out_idx both NULL: PDA_ERR_ARG;
 *            R * K > PDA_DEEP_MERGE_MAX_KEYS (64 KB of keys in a CU's 160 KB of LDS): PDA_ERR_UNSUPPORTED -- merge groups of lists to keys first
 *            (the order is total: merging in groups is exact).  No workspace; integers only: the same bits whatever the launch geometry.
 */
#ifndef PDA_HIP_DEEP_H
#define PDA_HIP_DEEP_H

#include "pda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PDA_DEEP_MAX_K 1024

/* Bytes of workspace of a pda_deep_topk_* call (0 for arguments the call refuses).  Non-decreasing in n_users_blk and in K. */
/* Buffer contract -- workspace (pda_deep_topk_workspace_bytes): needs no initialisation -- the call clears the 256-byte header itself, stream-ordered,
 * and writes every count and list entry before it reads it; afterwards a caller may read the identity word at +16 (the other header words are zero); one
 * workspace serves one call at a time. */
size_t pda_deep_topk_workspace_bytes(int n_users_blk, int n_items_local, int d, int K);

/* Score + head + history mask + top-K of a block of users over an item shard, without the rating matrix.
 *   out_keys u64 [n_users_blk, K] or NULL, out_idx i32 [n_users_blk, K] or NULL, out_val f32 [n_users_blk, K] or NULL: at least one. */
int pda_deep_topk_f32(const float* U, const float* I_shard, const float* pop_shard, const int32_t* users, int n_users_blk, int item_offset,
                      int n_items_local, int d, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode, int K, int head,
                      uint64_t* out_keys, int32_t* out_idx, float* out_val, void* workspace, size_t workspace_bytes, void* stream);

/* The same on bf16 tables (U, I_shard: bf16 bit patterns), rows widened to fp32 on load: identical to the fp32 call on the widened tables. */
int pda_deep_topk_bf16(const uint16_t* U, const uint16_t* I_shard, const float* pop_shard, const int32_t* users, int n_users_blk,
                       int item_offset, int n_items_local, int d, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode,
                       int K, int head, uint64_t* out_keys, int32_t* out_idx, float* out_val, void* workspace, size_t workspace_bytes,
                       void* stream);

/* pda_metrics on lists of 1 .. PDA_DEEP_MAX_K columns: sums f64 [4, n_ks] of precision, recall, ndcg, hit over the rows (added to `sums`);
 * r[:K] on a k_cols-long row, divided by min(K, k_cols).  workspace NULL: float atomics; else pda_metrics_deep_workspace_bytes(n_rows, n_ks)
 * bytes and the ordered reduction of pda_metrics_ordered (the same bits run after run). */
/* Buffer contract -- workspace (pda_metrics_deep_workspace_bytes, or NULL): needs no initialisation -- every partial sum is written by its workgroup
 * before the second launch adds them; nothing in it is meant for the caller afterwards; one workspace serves one call at a time. */
size_t pda_metrics_deep_workspace_bytes(int n_rows, int n_ks);
int pda_metrics_deep(const int32_t* topk, int n_rows, int k_cols, const int64_t* tgt_indptr, const int32_t* tgt_indices, const int32_t* Ks,
                     int n_ks, double* sums, void* workspace, void* stream);

/* Merge of R sorted lists of K keys per user (the lists of R item shards) into one: see "Item shards" above. */
#define PDA_DEEP_MERGE_MAX_KEYS 8192
int pda_deep_merge(const uint64_t* in_keys, int R, int n_users_blk, int K, uint64_t* out_keys, int32_t* out_idx, float* out_val,
                   const int32_t* users, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_DEEP_H */
