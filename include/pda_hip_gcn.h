/* pda_hip_gcn.h -- the LightGCN backbone (He et al., SIGIR'20, "LightGCN: Simplifying and Powering Graph Convolution Network for
 * Recommendation"; `--model lightgcn`) on libpda_hip.so: the sparse x dense product over the train graph that its forward and backward
 * passes are made of, and the regulariser of its ego rows.
 *
 * Same conventions as pda_hip.h: device pointers, an explicit `void* stream` (hipStream_t), int return codes (PDA_OK / PDA_ERR_*), every
 * argument check happens before anything is launched, and nothing is allocated.  Kept in its own header, like pda_hip_macr.h.
 *
 * Model.  Parameters: the ego tables U0 f32 [n_users, d] and I0 f32 [n_items, d].
 * Graph: the edges are the DISTINCT (u, i) pairs of the train set (a pair that occurs twice is one edge); deg_u / deg_i count edges;
 *     w_ui = fl32(1 / sqrt(float64(deg_u deg_i))), computed once on the host and rounded once: an input of the kernels, like the tables.
 * A node without edges has no neighbours: its propagated layers are 0.
 * Propagation, L layers:   E^(0) = (U0; I0)    E^(k+1)_u = sum_i w_ui E^(k)_i    E^(k+1)_i = sum_u w_ui E^(k)_u
 *                          F = (1 / (L + 1)) sum_{k = 0 .. L} E^(k)                                     (the final tables F_U, F_I)
 * Loss of a batch: the matching term of pda_bpr_step_f32 on F_U, F_I (the PD head with pos_pop / neg_pop, the raw head without; the mean is
 *     -mean log(sigmoid(.) + 1e-10)) + regs (l2(U0[u]) + l2(I0[p]) + l2(I0[n])) / reg_div on the EGO rows of the batch, per occurrence,
 *     l2(x) = sum(x^2) / 2, reg_div the --batch_size constant.
 * Gradient: with G = d(matching term) / dF (pda_bpr_step_f32(PDA_UPD_DENSE_GRAD) at regs = 0) and A the symmetric normalised adjacency,
 *     d loss / d E0 = (1 / (L + 1)) sum_{k = 0 .. L} A^k G + (regs / reg_div) (ego rows of the batch)
 * the sum in Horner form, H <- G + A H, L times from H = G, the last one scaled; the regulariser is added AFTER it and does not propagate.
 * Optimiser: the reference's Adam on the dense gradient, pda_adam_dense_sweep2_f32 over both ego tables.
 *
 * One stacked buffer: every table of the passes is one f32 [n_users + n_items, d] buffer, users first; the graph is the symmetric CSR over
 * its n_users + n_items rows (a user row lists n_users + i, an item row lists u), so that ONE launch per layer serves both directions.
 */
#ifndef PDA_HIP_GCN_H
#define PDA_HIP_GCN_H

#include "pda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A row with more edges than this is cut into chunks of this many edges (the last one shorter) that separate lane groups sum; the row's
 * partial sums are then added in chunk order by a second, small launch.  Item degrees are Zipf-distributed: without the cut a launch runs as
 * long as its most loaded wave. */
#define PDA_GCN_CHUNK 512

/* The work list of a graph, built ONCE per graph by the caller (pda_amd.ops.GcnGraph):
 *   work      i64 [n_work, 4]: (row, first edge, end edge, slot).  Every row has at least one entry (a row without edges: first == end);
 *             a row of at most PDA_GCN_CHUNK edges has exactly one, with slot = -1, and its lane group finishes the row.  A longer row has
 *             ceil(deg / PDA_GCN_CHUNK) consecutive entries in edge order with consecutive slots: entry j writes its partial sum to row
 *             slot of the workspace.
 *   long_rows i64 [n_long, 3]: (row, first slot, number of chunks) of every cut row; NULL when n_long == 0.
 * The kernels trust the list and the CSR (the caller validates them once, on the host): first <= end <= nnz, indices < n_rows,
 * row < n_rows, slot < n_slots, every row finished by exactly one entry of `work` or of `long_rows`. */

/* Bytes of workspace a product over a graph with n_slots partial-sum rows needs (0 slots: 0 bytes, workspace may be NULL). */
/* Buffer contract -- workspace (pda_gcn_spmm_workspace_bytes; may be NULL when n_slots == 0): needs no initialisation -- every chunk's partial row is
 * written before the row's sum reads it; nothing in it is meant for the caller afterwards; one workspace serves one call at a time. */
size_t pda_gcn_spmm_workspace_bytes(size_t n_slots, int d);

/* One weighted CSR x dense product with the fused forms of the two passes, for every row r of the n_rows:
 *     y   = (add ? add[r, :] : 0) + sum_{e in row r} w[e] X[indices[e], :]
 *     no sum_in:   Y[r, :] = scale y                                                  (the Horner step, H <- G + A H; the last one scaled)
 *     sum_in:      Y[r, :] = y (where Y != NULL),  sum_out[r, :] = scale (sum_in[r, :] + y)          (the layer mean; the last layer scaled)
 * indptr i64 [n_rows + 1], indices i32 [nnz], w f32 [nnz] (the HistoryCSR conventions); X, add, Y, sum_in, sum_out f32 [n_rows, d];
 * d in {32, 64, 128, 256}.  X must not alias Y or sum_out; sum_out may be sum_in (the row's owner reads, then writes it); add may be any
 * buffer that is not written.  sum_in and sum_out come together; without them Y is required.  scale is finite (1: an exact multiplication).
 * Order of every sum: the edges of an entry of `work` left to right onto a zero accumulator (fl(acc + fl(w x)) per element: the library is
 * built without contraction), a cut row's partial sums in chunk order onto zero, then `add + .`, then `sum_in + .`, then `scale * .`.  It is
 * a function of the CSR and of PDA_GCN_CHUNK alone: no atomics, the same bits run after run.
 * Layout: d / 4 lanes per entry of `work`, each lane one 16-byte piece of every gathered row, four edges' loads in flight per lane group.
 * Two launches when n_long > 0 (the products, then the cut rows), one otherwise. */
int pda_gcn_spmm_f32(const int64_t* indptr, const int32_t* indices, const float* w, size_t n_rows, const int64_t* work, size_t n_work,
                     const int64_t* long_rows, size_t n_long, size_t n_slots, const float* X, int d, const float* add, float* Y,
                     const float* sum_in, float* sum_out, float scale, void* workspace, size_t workspace_bytes, void* stream);

/* The regulariser of the batch's EGO rows, after the backward pass: for every triplet t (d / 4 lanes each)
 *     gU[users[t], :] += c U0[users[t], :]    gI[pos[t], :] += c I0[pos[t], :]    gI[neg[t], :] += c I0[neg[t], :]        c = fl(regs / reg_div)
 * per occurrence (duplicates add up; float atomics: 3 B rows), and loss_acc (optional) f32 [3]: [0] += reg, [2] += reg,
 * reg = c 0.5 sum_t (|U0[u]|^2 + |I0[p]|^2 + |I0[n]|^2) -- the matching term is already in [0] and [1] from the triplet kernel.
 * A triplet with an id outside the tables is skipped, as in the other step kernels. */
int pda_gcn_reg_f32(const float* U0, const float* I0, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos,
                    const int32_t* neg, int B, int d, float regs, float reg_div, float* gU, float* gI, float* loss_acc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_GCN_H */
