/* pda_hip_exposure.h -- item exposure of ranked lists on libpda_hip.so: per item, how often the lists show it and how often that is a hit,
 * split by column bucket.  The histogram under every popularity-bias statistic of pda_amd/exposure.py (recommendation rate per popularity
 * group, ARP, coverage, Gini, APLT, recall per group).
 *
 * Same conventions as pda_hip.h: device pointers, caller-owned buffers, an explicit `void* stream` (hipStream_t), int return codes
 * (PDA_OK / PDA_ERR_*), every argument check before anything is launched, no allocation, no synchronisation.  Kept in its own header, like
 * pda_hip_xquad.h.
 *
 * Contract ("5k. Bias report"):
 *   lists      topk i32 [n_rows, k_cols], 1 <= k_cols <= 1024: what every recommend_* call and pda_xquad_rerank write.
 *   invalid    an id outside [0, n_items) is ignored wherever it stands (the -1 of a short row, an id >= n_items); a valid id behind an
 *              invalid one still counts: every column counts on its own.
 *   Ks         i32 [n_ks] on the device, strictly ascending, 1 <= Ks[0], 1 <= n_ks <= PDA_EXPOSURE_MAX_KS; a Ks[b] > k_cols is read as k_cols,
 *              as pda_metrics reads it.  The order cannot be checked here (the values live on the device): on other values every access
 *              stays in bounds and column j lands in the first bucket b with j < Ks[b].
 *   buckets    bucket b = the columns j with Ks[b-1] <= j < Ks[b] (Ks[-1] = 0); columns >= Ks[n_ks-1] are in no bucket.  The count at the
 *              cut-off Ks[b] is the sum of the buckets <= b: the caller forms it.
 *   shown      shown[b][i] += the list entries of bucket b that hold item i                                       i32 [n_ks, n_items]
 *   hit        hit[b][i]   += those of them whose id also occurs in the row's target row tgt_indices[tgt_indptr[r] .. tgt_indptr[r+1])
 *              (rows may be unsorted, hold duplicates, be empty: the membership rule of pda_metrics)                i32 [n_ks, n_items]
 *              tgt_indptr, tgt_indices and hit all NULL: no hit counts.
 *   Precondition: the rows accumulated into one buffer stay below 2^31.
 *   Integer adds only: the same bits whatever the launch geometry and from run to run.
 */
#ifndef PDA_HIP_EXPOSURE_H
#define PDA_HIP_EXPOSURE_H

#include "pda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PDA_EXPOSURE_MAX_KS 8

/* PDA_ERR_ARG: a NULL topk, Ks or shown; some but not all of tgt_indptr, tgt_indices and hit; n_rows < 1; n_items < 1; k_cols outside
 * 1 .. 1024; n_ks outside 1 .. PDA_EXPOSURE_MAX_KS.
 * One workgroup per slab of rows combines its entries in an LDS table keyed by item id and adds every occupied slot to the buffers once;
 * what finds no slot goes to the buffers directly. */
int pda_list_exposure(const int32_t* topk, int n_rows, int k_cols, int n_items, const int64_t* tgt_indptr, const int32_t* tgt_indices,
                      const int32_t* Ks, int n_ks, int32_t* shown, int32_t* hit, void* stream);

/* The same contract and the same result with one global atomic add per list entry and no LDS table: the baseline the combining kernel is
 * measured against (tools/exposure_timing.py) and checked against (tests/test_gpu_exposure.py). */
int pda_list_exposure_plain(const int32_t* topk, int n_rows, int k_cols, int n_items, const int64_t* tgt_indptr, const int32_t* tgt_indices,
                            const int32_t* Ks, int n_ks, int32_t* shown, int32_t* hit, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_EXPOSURE_H */
