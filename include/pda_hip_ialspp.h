/* pda_hip_ialspp.h -- iALS++ (`--train ials --ials_solver block`) on libpda_hip.so: the block-wise (subspace) solver of the iALS objective, after
 * Rendle, Krichene, Zhang and Koren, "iALS++: Speeding up Matrix Factorization with Subspace Optimization" (2021).  The method is restated
 * here in full; nothing depends on a recollection of the paper.  Embedding sizes 32, 64, 128 and 256.
 *
 * Same conventions as pda_hip_ials.h: device pointers, an explicit `void* stream` (hipStream_t), int return codes (PDA_OK / PDA_ERR_*), every
 * argument check happens before anything is launched, nothing is allocated, no float atomics, the same bits call after call, and a row's
 * result is a function of its own work entries alone.
 *
 * Model.  The objective L(X, Y) is exactly that of pda_hip_ials.h (alpha0, nu, lambda, lam_row); nothing about it changes.  The d coordinates
 * are cut into d / k consecutive blocks pi = [p0, p0 + k).  For a row r of the side being solved, with Z the other table held fixed,
 * G = Z^T Z over ALL rows of Z, S_r the row's distinct partners and e_c = x_r . z_c the current prediction of the pair (r, c), one BLOCK STEP
 * is the exact minimiser of L over x_{r,pi} with everything else fixed:
 *     H     = sum_{c in S_r} z_{c,pi} z_{c,pi}^T + alpha0 G[pi, pi] + lam_row[r] I          (k x k, SPD because lam_row > 0)
 *     g     = sum_{c in S_r} (e_c - 1) z_{c,pi}  + alpha0 G[pi, :] x_r + lam_row[r] x_{r,pi}
 *     delta = H^{-1} g
 *     x_{r,pi} <- x_{r,pi} - delta
 *     e_c      <- e_c - z_{c,pi} . delta     for c in S_r
 * With k = d this is x_r <- A_r^{-1} b_r, the half-sweep of pda_hip_ials.h (up to rounding: a row without pairs comes out as x - H^{-1} H x,
 * not as an exact zero).  A block step starts from x: unlike the exact solver, the result depends on the tables' initialisation.
 * An EPOCH (pda_amd.ops.ialspp_epoch) is: (1) every e recomputed from the full tables (pda_ialspp_predict_f32), so that the cache never drifts
 * across epochs and never enters a checkpoint; (2) for each block in ascending order, the user pass on that block with G = Y^T Y, then the item
 * pass on that block with G = X^T X; (3) the objective from the tables, not from the cache (pda_ialspp_loss_f32).
 *
 * The prediction cache e is f32 [nnz] in the USER CSR's pair order.  The item side addresses it through pair_perm i64 [nnz]: pair_perm[q] is
 * the position in the user CSR of the pair at position q of the item CSR (built once on the host).
 *
 * Arithmetic: exact fp32, the library is built without contraction.  The order of every sum is a function of the CSR, of the work list, of
 * PDA_IALS_CHUNK, of PDA_IALS_GRAM_ROWS, of d and of k:
 *   - w_c = fl(e_c - 1), rounded once;
 *   - an entry (i, j) of a chunk's sum of z z^T: the fmaf chain over the chunk's pairs in CSR order onto zero (v_mfma_f32_32x32x2_f32 is that
 *     chain, lower-triangle 32 x 32 tiles mirrored); an entry i of its sum of w z: acc = fmaf(w_c, z_c[p0 + i], acc) in the same order onto zero;
 *   - a cut row: its chunks' partial (H, g) in chunk order onto zero;
 *   - H_ij = fl(fl(sum_ij + fl(alpha0 G[p0 + i, p0 + j])) + (i == j ? lam_row[r] : 0));
 *   - t = G[pi, :] x_r is read as G[:, pi]^T x_r (G is symmetric): the d columns are cut into Q = 2 (k = 32 or 128) or 4 (k = 64) consecutive
 *     parts, each part an fmaf chain fmaf(G[j, p0 + i], x_r[j], .) over its j ascending onto zero, the parts added in order onto zero;
 *     g_i = fl(fl(sum_i + fl(alpha0 t_i)) + fl(lam_row[r] x_r[p0 + i]));
 *   - the factorisation H = L L^T and the two substitutions: exactly the orders of pda_hip_ials.h with d replaced by k;
 *   - x_{r,pi}[i] = fl(x_r[p0 + i] - delta_i);
 *   - z_{c,pi} . delta: k / 4 lanes, four products per lane added as (p0 + p1) + (p2 + p3), then the lanes by a butterfly (offsets k / 8, ..., 1);
 *     e_c = fl(e_c - dot);
 *   - a prediction x . z (predict, loss): d / 4 lanes, the same four-product sum and butterfly;
 *   - G at d = 256: per block of PDA_IALS_GRAM_ROWS consecutive rows of Z and per 32 x 32 tile, the fmaf chain in row order onto zero, then the
 *     blocks in order onto zero (the order pda_hip_ials.h states for d <= 128, which this entry point runs there).
 * Failed pivots: a pivot that is not a finite number > 0 cannot occur with lam_row > 0 on finite tables and a finite e.  If one does, the row's
 * block x_{r,pi} and the row's e are written as NaN and *fail_count is raised by one per such row; nothing faults.
 */
#ifndef PDA_HIP_IALSPP_H
#define PDA_HIP_IALSPP_H

#include "pda_hip_ials.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Scratch sizes, as formulas (no size function is exported):
 *   - the slots of a block pass: n_slots slots of k * k + k floats (H row-major, then g), the slot size of pda_hip_ials.h at width k;
 *   - the delta buffer of a block pass: k floats per slot;
 *   - the Gram workspace: one slot of d * d + d floats per block of PDA_IALS_GRAM_ROWS rows, at every d. */
#define PDA_IALSPP_SLOT_FLOATS(k) ((size_t)(k) * (size_t)(k) + (size_t)(k))
#define PDA_IALSPP_DELTA_FLOATS(n_slots, k) ((size_t)(n_slots) * (size_t)(k))
#define PDA_IALSPP_GRAM_WS_FLOATS(n_rows, d) \
    ((((size_t)(n_rows) + PDA_IALS_GRAM_ROWS - 1) / PDA_IALS_GRAM_ROWS) * ((size_t)(d) * (size_t)(d) + (size_t)(d)))
/* Buffer contract -- slots, delta buffer, Gram workspace, the loss rows: none needs initialisation; every word that is read was written by the
 * same call before.  Nothing in the workspaces is meant for the caller afterwards; one workspace serves one call at a time. */

/* e[p] = x_row(p) . z_col(p) for every pair p of the CSR (indptr i64 [n_rows + 1], indices i32 [nnz]), in the CSR's pair order: X f32
 * [n_rows, d], Z f32 [n_z, d], e f32 [nnz], d in {32, 64, 128, 256}.  One workgroup per row, d / 4 lanes per pair.  A column id outside Z counts
 * as a zero row.  One launch. */
int pda_ialspp_predict_f32(const int64_t* indptr, const int32_t* indices, size_t n_rows, size_t nnz, const float* X, const float* Z, size_t n_z,
                           int d, float* e, void* stream);

/* One pass of the block [p0, p0 + k) over the rows of the work list (work / long_rows / n_slots: exactly the lists of pda_hip_ials.h, with
 * PDA_IALS_CHUNK unchanged; any subset of the rows in any order, the others are left as they are).
 * indptr, indices: the CSR of the side being solved; pair_perm i64 [nnz]: position q of this CSR -> position in e (NULL: the identity, the
 * user side); Z f32 [n_z, d] the other table, G f32 [d, d] its Gram matrix (symmetric), alpha0 >= 0 finite, lam_row f32 [n_rows];
 * X f32 [n_rows, d] (not Z): x_{r,pi} is updated IN PLACE, the other coordinates are read and left as they are; e f32 [nnz]: the entries of the
 * listed rows are read and updated; fail_count i32 [1]; d in {32, 64, 128, 256}, k in {32, 64, 128}, k divides d, p0 a multiple of k below d.
 * dbg, optional (NULL in the product), f32 [n_rows, k * k + k]: row r receives H row-major and then g, exactly as they enter the factorisation.
 * slots: n_slots * PDA_IALSPP_SLOT_FLOATS(k) floats, delta_ws: PDA_IALSPP_DELTA_FLOATS(n_slots, k) floats (both NULL when n_slots == 0);
 * slot_floats and delta_floats are the sizes handed over, in floats.
 * Layout: one workgroup per entry of `work` (64 lanes at k = 32, 256 otherwise) gathers the k-float slice of each partner row and e (4 k + 4
 * bytes per pair), staged in LDS in blocks of 32 pairs; H on v_mfma_f32_32x32x2_f32, factorised in place in LDS.  A whole row is solved,
 * stored and its e updated by the workgroup that summed it.  Cut rows take three phases: the chunks write their partial (H, g) to their
 * slots; one workgroup per cut row adds the slots in chunk order, solves, stores x and writes delta to delta_ws once per slot of the row; the
 * chunks gather again and update their e.  One launch when n_long == 0, three otherwise. */
int pda_ialspp_block_pass_f32(const int64_t* indptr, const int32_t* indices, const int64_t* pair_perm, size_t n_rows, size_t nnz,
                              const int64_t* work, size_t n_work, const int64_t* long_rows, size_t n_long, size_t n_slots, const float* Z,
                              size_t n_z, const float* G, int d, int k, int p0, float alpha0, const float* lam_row, float* X, float* e,
                              int32_t* fail_count, float* dbg, float* slots, size_t slot_floats, float* delta_ws, size_t delta_floats,
                              void* stream);

/* G = Z^T Z, f32 [d, d] row-major and symmetric bit for bit, over the n_rows rows of Z f32 [n_rows, d]; d in {32, 64, 128, 256}.  workspace:
 * at least PDA_IALSPP_GRAM_WS_FLOATS(n_rows, d) floats (workspace_floats is the size handed over).  Two launches. */
int pda_ialspp_gram_f32(const float* Z, size_t n_rows, int d, float* G, float* workspace, size_t workspace_floats, void* stream);

/* The three per-row terms of the objective, out f32 [n_rows, 3], exactly as pda_hip_ials.h states them for its loss entry point, with the
 * predictions taken fresh from the tables; d in {32, 64, 128, 256} (d <= 128 runs that entry point's kernels). */
int pda_ialspp_loss_f32(const int64_t* indptr, const int32_t* indices, size_t n_rows, size_t nnz, const float* X, const float* Z, size_t n_z,
                        const float* G, int d, const float* lam_row, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_IALSPP_H */
