/* pda_hip_ials_itemw.h -- item-weighted iALS (`--train ials --ials_item_power beta`, either solver) on libpda_hip.so: the unobserved pairs of
 * item i are weighed by alpha0 w_i with w_i rising with the item's popularity, where pda_hip_ials.h weighs every one of them by alpha0.  This
 * is the weighting of eALS (He, Zhang, Kan and Chua, "Fast Matrix Factorization for Online Recommendation with Implicit Feedback", SIGIR'16;
 * PAPERS.md) put on the objective of pda_hip_ials.h and solved by its two solvers; the method is restated here in full.
 *
 * Same conventions as pda_hip_ials.h and pda_hip_ialspp.h: device pointers, an explicit `void* stream` (hipStream_t), int return codes
 * (PDA_OK / PDA_ERR_*), every argument check happens before anything is launched, nothing is allocated, no float atomics, the same bits call
 * after call, out-of-range entries skipped, a failed pivot writes NaN and raises the counter, the dbg outputs as they are there.
 *
 * Model.  c_i: the distinct train pairs of item i; beta = `--ials_item_power`, 0 <= beta <= 4 (0: the unweighted model).
 *     q_i     = (c_i + 1)^beta / sum_j (c_j + 1)^beta                 float64 on the host (the q of pda_hip_negpop.h)
 *     s_i     = fl32(sqrt(n_items q_i))                               rounded once on the host: the input scale_row of the Gram matrix
 *     w_i    := float64(s_i)^2                                        THE weight of the model; its mean is 1 up to rounding
 *     alpha_i = fl32(alpha0 w_i)                                      rounded once on the host: the input alpha_row, as lam_row is an input
 * beta = 0 gives s = w = 1 exactly and alpha_i = fl32(alpha0).
 *     L(X, Y) =  sum_{(u,i) in S} (x_u . y_i - 1)^2
 *              + alpha0 sum_u sum_i w_i (x_u . y_i)^2
 *              + lambda [ sum_u (n_u + alpha0 n_items)^nu |x_u|^2  +  sum_i (n_i + alpha0 w_i n_users)^nu |y_i|^2 ]
 * (the item's regulariser counts its unobserved mass as the objective weighs it; the user's sum_i alpha0 w_i = alpha0 n_items is unchanged).
 *
 * The user side (Z = Y held fixed):  A_u = alpha0 G_w + sum_{i in S_u} y_i y_i^T + lam_u I,   G_w = sum_i (s_i y_i)(s_i y_i)^T,   b_u unchanged.
 *     This is the half-sweep, the block pass and the loss kernel of the two headers as they are, handed G_w where they took G.
 * The item side (Z = X held fixed):  A_i = alpha_i G + sum_{u in S_i} x_u x_u^T + lam_i I,    G = X^T X,   b_i unchanged;
 *     a block step has H = .. + alpha_i G[pi, pi] + .. and g = .. + alpha_i G[pi, :] y_i + ..
 *     This is the existing arithmetic with alpha_row[r] where it read the scalar alpha0.
 *
 * Arithmetic: the order of every sum is that of pda_hip_ials.h and pda_hip_ialspp.h, with
 *   - one new rounding: a scaled row is z'_c[j] = fl(s_c z_c[j]), one rounding per element, no contraction; the chains of the Gram matrix run
 *     on z'.  Both operands of an entry G_w[i, j] are the same rounded numbers as those of G_w[j, i], so G_w is symmetric bit for bit, as the
 *     block pass assumes;
 *   - one replaced input: fl(alpha_row[r] G_ij) and fl(alpha_row[r] t_i) stand where fl(alpha0 G_ij) and fl(alpha0 t_i) stood.
 * With scale_row all 1 and alpha_row constant the three entry points give the bits of pda_ials_gram_f32 / pda_ialspp_gram_f32,
 * pda_ials_half_sweep_f32 and pda_ialspp_block_pass_f32.  Those entry points keep their kernels, instruction for instruction
 * (profiles/ials_itemw_resource_usage.txt).
 */
#ifndef PDA_HIP_IALS_ITEMW_H
#define PDA_HIP_IALS_ITEMW_H

#include "pda_hip_ialspp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* G = sum_c (scale_row[c] z_c)(scale_row[c] z_c)^T, f32 [d, d] row-major and symmetric bit for bit, over the n_rows rows of Z f32 [n_rows, d];
 * scale_row f32 [n_rows]; d in {32, 64, 128, 256}.  The scale is fused into the row fetch (one 4-byte load per row): there is no scaled copy
 * of the table.  Blocks of PDA_IALS_GRAM_ROWS rows in row order onto zero, the blocks in order onto zero, as in pda_ials_gram_f32 (d <= 128)
 * and pda_ialspp_gram_f32 (d = 256).  workspace: at least PDA_IALSPP_GRAM_WS_FLOATS(n_rows, d) floats, no initialisation needed
 * (workspace_floats is the size handed over).  G is neither Z nor scale_row.  Two launches. */
int pda_ials_gram_scaled_f32(const float* Z, const float* scale_row, size_t n_rows, int d, float* G, float* workspace, size_t workspace_floats,
                             void* stream);

/* The d = 256 half of pda_ials_gram_scaled_f32, which hands that width over to it (it lives beside the d = 256 kernels of pda_ialspp_gram_f32);
 * callers use pda_ials_gram_scaled_f32. */
int pda_ialspp_gram256_scaled_f32(const float* Z, const float* scale_row, size_t n_rows, float* G, float* workspace, size_t workspace_floats,
                                  void* stream);

/* pda_ials_half_sweep_f32 with alpha_row f32 [n_rows] (each finite and >= 0: an input, validated once by the caller on the host like lam_row)
 * in place of alpha0: A_r = alpha_row[r] G + sum z z^T + lam_row[r] I.  Every other argument, the layout, the launches and dbg_normal are those
 * of pda_ials_half_sweep_f32; one more 4-byte load per solved row.  X_out is not alpha_row. */
int pda_ials_half_sweep_rowalpha_f32(const int64_t* indptr, const int32_t* indices, size_t n_rows, size_t nnz, const int64_t* work, size_t n_work,
                                     const int64_t* long_rows, size_t n_long, size_t n_slots, const float* Z, size_t n_z, const float* G, int d,
                                     const float* alpha_row, const float* lam_row, float* X_out, int32_t* fail_count, float* dbg_normal,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* pda_ialspp_block_pass_f32 with alpha_row f32 [n_rows] (each finite and >= 0) in place of alpha0: H takes alpha_row[r] G[pi, pi] and g takes
 * alpha_row[r] G[pi, :] x_r.  Every other argument, the layout, the launches and dbg are those of pda_ialspp_block_pass_f32.  Neither X nor e
 * is alpha_row. */
int pda_ialspp_block_pass_rowalpha_f32(const int64_t* indptr, const int32_t* indices, const int64_t* pair_perm, size_t n_rows, size_t nnz,
                                       const int64_t* work, size_t n_work, const int64_t* long_rows, size_t n_long, size_t n_slots,
                                       const float* Z, size_t n_z, const float* G, int d, int k, int p0, const float* alpha_row,
                                       const float* lam_row, float* X, float* e, int32_t* fail_count, float* dbg, float* slots,
                                       size_t slot_floats, float* delta_ws, size_t delta_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PDA_HIP_IALS_ITEMW_H */
