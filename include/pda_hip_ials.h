/* pda_hip_ials.h -- the iALS baseline (`--train ials`) on libpda_hip.so: implicit alternating least squares (Hu, Koren and Volinsky, "Collaborative
 * Filtering for Implicit Feedback Datasets", ICDM'08) in the form of Rendle, Krichene, Zhang and Koren, "Revisiting the Performance of iALS on
 * Item Recommendation Benchmarks" (RecSys'22): the Gram matrix of a table, the exact row-wise half-sweep and the objective.
 *
 * Same conventions as pda_hip_gcn.h: device pointers, an explicit `void* stream` (hipStream_t), int return codes (PDA_OK / PDA_ERR_*), every
 * argument check happens before anything is launched, and nothing is allocated.  Kept in its own header, like pda_hip_gcn.h.
 *
 * Model.  Parameters: X f32 [n_users, d] and Y f32 [n_items, d].  S is the set of DISTINCT (u, i) pairs of the train set (a
 * pair that occurs twice counts once); n_u and n_i are the degrees in S.
 *     L(X, Y) =  sum_{(u,i) in S} (x_u . y_i - 1)^2
 *              + alpha0 sum_u sum_i (x_u . y_i)^2
 *              + lambda [ sum_u (n_u + alpha0 n_items)^nu |x_u|^2  +  sum_i (n_i + alpha0 n_users)^nu |y_i|^2 ]
 * alpha0 >= 0 (`--ials_alpha0`) weighs the unobserved pairs, 0 <= nu <= 1 (`--ials_nu`) scales the regulariser with frequency (0: plain L2),
 * lambda > 0 is `--regs`.  Hu et al. write the same family as c_ui = 1 + alpha on observed pairs over a weight 1 everywhere and a plain L2 term
 * lambda_hu: dividing their objective by alpha gives this one at alpha0 = 1 / alpha, lambda = lambda_hu / alpha and nu = 0.  (An observed pair
 * then carries (1 + alpha0) (x.y - 1)^2 where this form has (x.y - 1)^2 + alpha0 (x.y)^2: the two differ by alpha0 (1 - 2 x.y) per observed
 * pair, small next to the fit term at the usual alpha0 << 1.  The classic flags map as a rescaling, not bit for bit.)
 *
 * One half-sweep holds the other table Z fixed (Z = Y for the user side, X for the item side).  With G = Z^T Z over ALL rows of Z, every row r
 * of the side being solved is replaced by the exact minimiser
 *     A_r = alpha0 G + sum_{c in S_r} z_c z_c^T + lambda_r I          b_r = sum_{c in S_r} z_c          x_r = A_r^{-1} b_r
 * lambda_r = fl32(lambda * float64(n_r + alpha0 n_other)^nu) is computed once on the host and rounded once: an INPUT of the kernels (lam_row),
 * like w of the LightGCN graph.  A row without pairs has b = 0 and becomes exactly 0.  An epoch is the user half-sweep, then the item one.
 *
 * Arithmetic: exact fp32, no atomics in any sum, the same bits call after call; a row's result depends on its own work entries alone.
 * The order of every sum is a function of the CSR, of PDA_IALS_CHUNK, of PDA_IALS_GRAM_ROWS and of d:
 *   - an entry (i, j) of a chunk's sum of z z^T: the fmaf chain over the chunk's pairs in CSR order onto zero, acc = fmaf(z_c[i], z_c[j], acc)
 *     (v_mfma_f32_32x32x2_f32 is that chain); an entry of its sum of z: fl(acc + z_c[i]) in the same order onto zero;
 *   - a cut row: its chunks' partial sums in chunk order onto zero;
 *   - then A_ij = fl(fl(sum_ij + fl(alpha0 G_ij)) + (i == j ? lambda_r : 0)) -- the library is built without contraction;
 *   - G: the fmaf chains of blocks of PDA_IALS_GRAM_ROWS consecutive rows of Z, in row order onto zero, then the blocks in order onto zero;
 *   - the factorisation A = L L^T, column by column: s_ij = the fmaf chain A_ij, then fmaf(-L_ik, L_jk, .) for k = 0 .. j - 1 in this order;
 *     L_jj = sqrtf(s_jj), L_ij = s_ij / L_jj -- the inner products ARE fmaf chains;
 *   - L y = b: y_j = s_j / L_jj with s_j the fmaf chain b_j, then fmaf(-L_jk, y_k, .) for k = 0 .. j - 1; L^T x = y: x_j = s_j / L_jj with s_j
 *     the chain y_j, then fmaf(-L_kj, x_k, .) for k = d - 1 down to j + 1.
 * Failed pivots: a pivot s_jj that is not a finite number > 0 cannot occur with lambda_r > 0 on finite tables.  If one does, the whole row is
 * written as NaN and *fail_count is raised by one per such row; nothing faults.
 */
#ifndef PDA_HIP_IALS_H
#define PDA_HIP_IALS_H

#include "pda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A row with more pairs than this is cut into chunks of this many pairs (the last one shorter), each summed by a workgroup of its own into a
 * workspace slot of d * d + d floats (A row-major, then b); a second launch adds a cut row's slots in chunk order and solves.  Item degrees are
 * Zipf-distributed: without the cut the half-sweep runs as long as its longest row. */
#define PDA_IALS_CHUNK 4096
/* G = Z^T Z is summed over blocks of this many consecutive rows, one workspace slot each. */
#define PDA_IALS_GRAM_ROWS 256

/* The work list of one side, built ONCE per graph by the caller (pda_amd.ops.IalsGraph), with the conventions of pda_hip_gcn.h:
 *   work      i64 [n_work, 4]: (row, first pair, end pair, slot).  A row of at most PDA_IALS_CHUNK pairs has one entry with slot = -1 (a row
 *             without pairs: first == end) and the workgroup that sums it also solves it.  A longer row has ceil(deg / PDA_IALS_CHUNK)
 *             entries in pair order with consecutive slots.
 *   long_rows i64 [n_long, 3]: (row, first slot, number of chunks) of every cut row in the list; NULL when n_long == 0.
 * A call may list ANY subset of the rows, in any order: the rows it does not list are left as they are.
 * The kernels trust the list and the CSR (the caller validates them once, on the host).  As a last line of defence an entry whose row, pair
 * range or slot lies outside the given sizes is skipped and a column id outside Z counts as a zero row, so that nothing is read or written out
 * of bounds. */

/* Bytes of n_slots workspace slots of d * d + d floats (0 slots or an unsupported d: 0 bytes). */
/* Buffer contract -- workspace (pda_ials_workspace_bytes; may be NULL when n_slots == 0): needs no initialisation -- every slot is written by its chunk
 * (its block of rows, for the Gram matrix) before it is added up; nothing in it is meant for the caller afterwards; one workspace serves one call at a
 * time. */
size_t pda_ials_workspace_bytes(size_t n_slots, int d);

/* G = Z^T Z, f32 [d, d] row-major, over the n_rows rows of Z f32 [n_rows, d]; d in {32, 64, 128}.  The workspace holds
 * ceil(n_rows / PDA_IALS_GRAM_ROWS) slots.  Two launches. */
int pda_ials_gram_f32(const float* Z, size_t n_rows, int d, float* G, void* workspace, size_t workspace_bytes, void* stream);

/* One half-sweep over the rows of `work`: X_out[r, :] = A_r^{-1} b_r.
 * indptr i64 [n_rows + 1], indices i32 [nnz] ascending within a row (the HistoryCSR conventions) of the side being solved; Z f32 [n_z, d] the
 * other table, G f32 [d, d] its Gram matrix, alpha0 >= 0 finite, lam_row f32 [n_rows], X_out f32 [n_rows, d] (not Z), fail_count i32 [1]
 * (raised, never reset, by the rows with a failed pivot), d in {32, 64, 128}: d = 256 is PDA_ERR_UNSUPPORTED, a 256 x 256 fp32 matrix does
 * not fit the 160 KiB of LDS.  dbg_normal, optional (NULL in the product), f32 [n_rows, d * d + d]: row r receives A_r row-major and then b_r,
 * exactly as they enter the factorisation.  The workspace holds n_slots slots (NULL when n_slots == 0).
 * Layout: one workgroup per entry of `work` (64 lanes at d = 32, 256 otherwise).  The gathered rows are staged in LDS in blocks of 32, the next
 * block's 16-byte loads in flight while the lower-triangle 32 x 32 tiles of the block are accumulated by v_mfma_f32_32x32x2_f32; A (stride
 * d + 1) is factorised in place in LDS.  Two launches when n_long > 0, one otherwise. */
int pda_ials_half_sweep_f32(const int64_t* indptr, const int32_t* indices, size_t n_rows, size_t nnz, const int64_t* work, size_t n_work,
                            const int64_t* long_rows, size_t n_long, size_t n_slots, const float* Z, size_t n_z, const float* G, int d,
                            float alpha0, const float* lam_row, float* X_out, int32_t* fail_count, float* dbg_normal, void* workspace,
                            size_t workspace_bytes, void* stream);

/* The objective's terms of one side, per row r of X f32 [n_rows, d] (d / 4 lanes each), out f32 [n_rows, 3]:
 *     [0] sum_{c in S_r} (x_r . z_c - 1)^2        [1] x_r^T G x_r        [2] lam_row[r] |x_r|^2
 * The caller sums the columns in float64 (no atomics): L = sum [0] + alpha0 sum [1] + sum [2] + the regulariser of the other side.
 * Order: a dot product is four partial products per lane added as (p0 + p1) + (p2 + p3), then the lanes by a butterfly; [0] adds its terms in
 * CSR order; t = G x adds its d terms in index order. */
int pda_ials_loss_f32(const int64_t* indptr, const int32_t* indices, size_t n_rows, size_t nnz, const float* X, const float* Z, size_t n_z,
                      const float* G, int d, const float* lam_row, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_IALS_H */
