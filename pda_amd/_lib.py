"""ctypes binding of libpda_hip.so (the C ABI declared in include/pda_hip.h, pda_hip_experimental.h, pda_hip_temp_pop.h, pda_hip_pc.h, pda_hip_det.h,
pda_hip_deep.h, pda_hip_xquad.h, pda_hip_dice.h, pda_hip_ips.h, pda_hip_macr.h, pda_hip_gcn.h, pda_hip_exposure.h, pda_hip_ssm.h,
pda_hip_inbatch.h, pda_hip_dns.h, pda_hip_ials.h, pda_hip_fullsm.h, pda_hip_rank.h, pda_hip_pcc.h, pda_hip_dau.h, pda_hip_negpop.h, pda_hip_ialspp.h, pda_hip_calib.h, pda_hip_warp.h and pda_hip_ials_itemw.h).

There is NO CPU fallback: if the shared object is missing or a symbol is absent this module raises.
Device pointers come from torch ROCm tensors (``tensor.data_ptr()``); the launch stream is torch's
current HIP stream, so torch.cuda.Event / torch.cuda.graph see every kernel.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PDA_HIP_LIB") or os.path.join(_HERE, "csrc", "libpda_hip.so")   # PDA_HIP_LIB: an A/B build of the same library (tools/)

# Constants mirrored from include/pda_hip.h
ABI_VERSION = 2
HEAD_RAW, HEAD_POP = 0, 1
HIST_BY_BLOCK_ROW, HIST_BY_USER_ID = 0, 1
UPD_NONE, UPD_SGD_FUSED, UPD_DENSE_GRAD = 0, 1, 2
UPD_ANY_ORDER = 0x100
UPD_USERS_DISTINCT = 0x200
ADAM_REPLAY_FAST = 0x10
MAX_K = 64
TOPK_CAP = 60

_vp, _i, _f, _u64, _sz = C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_size_t

class ScorePlan(C.Structure):
    """struct pda_score_plan of include/pda_hip.h (pda_score_topk_plan)."""
    _fields_ = [("path", _i), ("sweep_mode", _i), ("n_splits", _i), ("early_stop", _i), ("order", _i), ("prep_with_pop", _i),
                ("workspace_bytes", _sz), ("keys_rows", _sz)]


class SampleJob(C.Structure):
    """struct pda_sample_job of include/pda_hip.h (arguments of pda_sample_triplets_dev, for pda_bpr_step_sample_f32)."""
    _fields_ = [("users", _vp), ("gen_users", _i), ("user_pool", _vp), ("n_pool", _i), ("B", _i),
                ("train_indptr", _vp), ("train_indices", _vp), ("train_slots", _vp),
                ("neg_lo", _i), ("neg_hi", _i), ("pop_matrix", _vp), ("n_slots", _i), ("seed", _u64),
                ("step_dev", _vp), ("step_next", _vp),
                ("pos", _vp), ("neg", _vp), ("pos_pop", _vp), ("neg_pop", _vp)]


# name -> (restype, argtypes); exactly the declarations of include/pda_hip.h
SIGNATURES = {
    "pda_abi_version": (_i, []),
    "pda_error_string": (C.c_char_p, [_i]),
    "pda_score_topk_auto_splits": (_i, [_i, _i]),
    "pda_score_topk_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "pda_item_prep_bytes": (_sz, [_i, _i]),
    "pda_item_prep_f32": (_i, [_vp, _i, _i, _vp, _vp]),
    "pda_score_topk_workspace_bytes": (_sz, [_i]),
    "pda_score_topk4_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "pda_score_topk_prepped_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "pda_item_prep_ordered_bytes": (_sz, [_i, _i]),
    "pda_item_prep_ordered_f32": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "pda_item_prep_ordered_check": (_i, [_vp, _i, _i, _vp]),
    "pda_hist_reorder": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "pda_score_topk_ordered_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "pda_item_prep_bf16_bytes": (_sz, [_i, _i]),
    "pda_item_prep_bf16": (_i, [_vp, _i, _i, _vp, _vp]),
    "pda_score_topk_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "pda_item_prep_ordered_bf16_bytes": (_sz, [_i, _i]),
    "pda_item_prep_ordered_bf16": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "pda_score_topk_ordered_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "pda_item_prep4_bytes": (_sz, [_i, _i]),
    "pda_item_prep4_f32": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "pda_item_prep4_bf16": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "pda_item_prep7_f32": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "pda_item_prep7_bf16": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "pda_item_prep4_check": (_i, [_vp, _i, _i, _vp]),
    "pda_score_topk4_auto_splits": (_i, [_i, _i, _i]),
    "pda_score_topk4_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "pda_score_topk4_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "pda_peak_mfma_flops_per_launch": (C.c_double, [_i]),
    "pda_peak_mfma_bf16": (_i, [_vp, _i, _vp]),
    "pda_peak_mfma_bf16_const": (_i, [_vp, _i, _vp]),
    "pda_peak_mfma_lds_flops_per_launch": (C.c_double, [_i]),
    "pda_peak_mfma_lds_bf16": (_i, [_vp, _sz, _vp, _i, _vp]),
    "pda_peak_copy": (_i, [_vp, _vp, _sz, _vp]),
    "pda_topk_kth_value": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "pda_topk_remap_items": (_i, [_vp, _sz, _vp, _i, _vp]),
    "pda_topk_seed_refine": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "pda_topk_seed_bounds": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "pda_topk_seed_counts": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    "pda_topk_seed_pick": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "pda_score_topk4_phase_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "pda_score_topk4_phase_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "pda_score_topk4_phase_image_offsets": (_i, [_i, _i, _i, _i, _vp]),
    "pda_score_topk4_phase_user_image": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "pda_score_topk4_phase_mask_table": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "pda_score_topk4_phase_mask_rows": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp, _vp]),
    "pda_score_topk4_phase_mask_offsets": (_i, [_i, _i, _i, _i, _vp]),
    "pda_score_topk7_phase_user_image": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "pda_score_topk4_phase_bloom_rows": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp]),
    "pda_score_topk7_phase_bloom_rows": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "pda_score_topk4_phase_masked_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "pda_score_topk4_phase_masked_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "pda_score_topk_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "pda_score_topk_huge_splits": (_i, [_i, _i, _i]),
    "pda_score_topk7_workspace_bytes": (_sz, [_i, _i, _i]),
    "pda_score_topk7_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "pda_score_topk7_bf16": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "pda_topk_merge": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "pda_bpr_step_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pda_triplet_plan_bytes": (_sz, [_i]),
    "pda_bpr_step_plan_scratch_bytes": (_sz, [_i, _i]),
    "pda_triplet_plan": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "pda_triplet_plan_large_workspace_bytes": (_sz, [_i]),
    "pda_triplet_plan_large": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "pda_bpr_step_plan_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _vp, _vp, _i, _vp, _vp]),
    "pda_bpr_step_plan_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _vp, _vp, _vp, _vp]),
    "pda_sgd_apply_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "pda_bpr_step_shard_f32": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _f, _vp, _i, _vp, _vp, _vp]),
    "pda_apply_user_grads_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp]),
    "pda_bpr_step_bf16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pda_refresh_rows_bf16": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "pda_group_triplets_by_pos": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "pda_sort_triplets_by_pos": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "pda_adam_dense_sweep_f32": (_i, [_vp, _vp, _vp, _vp, _sz, _f, _f, _f, _f, _vp]),
    "pda_adam_dense_sweep2_f32": (_i, [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _sz, _f, _f, _f, _f, _vp]),
    "pda_adam_mark_rows": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "pda_adam_dense_sweep3_f32": (_i, [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _i, _f, _f, _f, _f, _vp]),
    "pda_score_dense_f32": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp]),
    "pda_adam_dense_sweep4_f32": (_i, [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _i, _i, _f, _f, _f, _f, _i, _vp]),
    "pda_adam_step_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _i, _f, _f, _f, _f,
                               _i, _i, _vp, _vp]),
    "pda_adam_rows_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _f, _vp]),
    "pda_adam_lazy_f32": (_i, [_i] + [_vp] * 13 + [_i, _i, _i, _vp, _f, _f, _f, _vp]),
    "pda_adam_lazy_dev_f32": (_i, [_i] + [_vp] * 13 + [_i, _i, _vp, _vp, _vp, _i, _f, _f, _f, _vp]),
    "pda_adam_lazy_sync_f32": (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _vp, _f, _f, _f, _vp]),
    "pda_adam_lazy_sync_fast_f32": (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _vp, _f, _f, _f, _vp]),
    "pda_metrics": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "pda_sample_triplets_dev": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pda_sample_batches_dev": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "pda_group_triplets_by_pos_batches": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "pda_counter_add": (_i, [_vp, _u64, _vp]),
    "pda_bpr_step_sample_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _i, _vp, _vp, _vp]),
    "pda_bpr_train_steps_f32": (_i, [_vp, _vp, _i, _f, _f, _f, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "pda_sample_triplets": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _u64, _u64, _vp, _vp, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_temp_pop.h (BPRMF(t)-pop, `--train temp_pop`)
HEAD_BIAS = 2
TEMP_POP_SIGNATURES = {
    "pda_temp_pop_step_f32": (_i, [_vp] * 8 + [_i, _i, _i, _f, _f] + [_vp] * 6 + [_i, _vp, _vp]),
    "pda_temp_pop_sweep_f32": (_i, [_vp] * 5 + [_sz] + [_vp] * 5 + [_sz] + [_vp] * 8 + [_i, _i, _i, _f, _f, _f, _f, _vp]),
    "pda_temp_pop_adam_step_f32": (_i, [_vp] * 5 + [_sz] + [_vp] * 5 + [_sz] + [_vp] * 12 + [_i, _i, _i, _f, _f, _i, _f, _f, _f, _f, _vp, _vp]),
    "pda_temp_pop_score_workspace_bytes": (_sz, [_i]),
    "pda_temp_pop_score_topk_f32": (_i, [_vp] * 6 + [_i, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_pc.h (BPR-PC)
HEAD_PC = 3
PC_MAX_K = 50
_d = C.c_double
PC_SIGNATURES = {
    "pda_pc_moments_workspace_bytes": (_sz, [_i, _i]),
    "pda_pc_item_moments_f32": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "pda_pc_user_stats_f32": (_i, [_vp] * 5 + [_i, _i, _i, _vp, _vp, _i, _d, _vp, _vp, _vp, _vp]),
    "pda_pc_score_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "pda_pc_score_topk_f32": (_i, [_vp] * 5 + [_i, _i, _i, _vp, _vp, _i, _d, _d, _i, _i, _vp, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_det.h (the bit-reproducible path, `--deterministic 1`)
DET_SIGNATURES = {
    "pda_bpr_grad_plan_scratch_bytes": (_sz, [_i, _i]),
    "pda_bpr_grad_plan_f32": (_i, [_vp] * 7 + [_i, _i, _f, _f] + [_vp] * 6 + [_i, _vp, _vp]),
    "pda_adam_step_plan_f32": (_i, [_vp] * 5 + [_sz] + [_vp] * 5 + [_sz] + [_vp] * 5 + [_i, _i, _f, _f, _i, _f, _f, _f, _f, _i, _vp, _vp, _vp, _vp]),
    "pda_metrics_ordered_workspace_bytes": (_sz, [_i, _i]),
    "pda_metrics_ordered": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_deep.h (deep lists: exact top-K up to 1 024, `--topk_max`)
DEEP_MAX_K = 1024
DEEP_MERGE_MAX_KEYS = 8192
DEEP_SIGNATURES = {
    "pda_deep_topk_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "pda_deep_topk_f32": (_i, [_vp] * 4 + [_i, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "pda_deep_topk_bf16": (_i, [_vp] * 4 + [_i, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "pda_metrics_deep_workspace_bytes": (_sz, [_i, _i]),
    "pda_metrics_deep": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "pda_deep_merge": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_xquad.h (xQuAD re-ranking of candidate lists, `python -m pda_amd.xquad`)
XQUAD_MAX_K = 64
XQUAD_MAX_N = 1024
XQUAD_BINARY, XQUAD_SMOOTH = 0, 1
XQUAD_SIGNATURES = {
    "pda_xquad_rerank": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _i, _d, _i, _i, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_dice.h (DICE, `--train dice`)
DICE_DIS_L1, DICE_DIS_L2 = 0, 1
DICE_SIGNATURES = {
    "pda_dice_rows_ws_words": (_sz, [_i]),
    "pda_dice_step_f32": (_i, [_vp, _vp, _sz, _sz] + [_vp] * 4 + [_i, _i, _f, _f, _f, _f] + [_vp] * 4 + [_i, _vp, _vp, _vp]),
    "pda_dice_dis_f32": (_i, [_vp, _vp, _sz, _sz, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "pda_dice_adam_step_f32": (_i, [_vp] * 5 + [_sz] + [_vp] * 5 + [_sz] + [_vp] * 4 + [_i, _i, _f, _f, _i, _f, _f, _f, _i, _f, _f, _f, _f, _i,
                                    _vp, _vp, _vp]),
    "pda_dice_sample": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _f, _u64, _u64, _vp, _vp, _vp, _vp]),
    "pda_dice_sample_dev": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_ips.h (IPS, IPS-C, IPS-CN: `--train ips`)
IPS_SIGNATURES = {
    "pda_ips_weight_sum": (_i, [_vp, _sz, _sz, _vp, _vp, _vp, _i, _vp, _vp]),
    "pda_ips_step_f32": (_i, [_vp, _vp, _sz, _sz] + [_vp] * 5 + [_i, _i, _f, _f] + [_vp] * 4 + [_i, _i, _vp, _vp]),
    "pda_ips_adam_step_f32": (_i, [_vp] * 5 + [_sz] + [_vp] * 5 + [_sz] + [_vp] * 5 + [_i, _i, _f, _f, _i, _f, _f, _f, _f, _i, _i, _vp, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_macr.h (MACR: `--train macr`)
MACR_SIGNATURES = {
    "pda_macr_step_f32": (_i, [_vp] * 4 + [_sz, _sz] + [_vp] * 3 + [_i, _i, _f, _f, _f, _f] + [_vp] * 5 + [_i, _i, _vp, _vp]),
    "pda_macr_adam_step_f32": (_i, [_vp] * 5 + [_sz] + [_vp] * 5 + [_sz] + [_vp] * 8 + [_i, _i, _f, _f, _f, _f, _i, _f, _f, _f, _f, _i, _i, _vp, _vp]),
    "pda_macr_item_prep_f32": (_i, [_vp, _vp, _sz, _i, _vp, _vp, _vp]),
    "pda_macr_item_bias_f32": (_i, [_vp, _f, _vp, _sz, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_gcn.h (the LightGCN backbone: `--model lightgcn`)
GCN_CHUNK = 512
GCN_SIGNATURES = {
    "pda_gcn_spmm_workspace_bytes": (_sz, [_sz, _i]),
    "pda_gcn_spmm_f32": (_i, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _i, _vp, _vp, _vp, _vp, _f, _vp, _sz, _vp]),
    "pda_gcn_reg_f32": (_i, [_vp, _vp, _sz, _sz, _vp, _vp, _vp, _i, _i, _f, _f, _vp, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_exposure.h (item exposure of the lists: `--bias_report 1`)
EXPOSURE_MAX_KS = 8
EXPOSURE_MAX_COLS = 1024
EXPOSURE_SIGNATURES = {
    "pda_list_exposure": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "pda_list_exposure_plain": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_ssm.h (the sampled-softmax loss: `--train ssm`)
SSM_MAX_NEGS = 256
SSM_SIGNATURES = {
    "pda_ssm_step_f32": (_i, [_vp, _vp, _sz, _sz] + [_vp] * 3 + [_i, _i, _i, _f, _i, _f, _f] + [_vp] * 4 + [_i, _i, _vp, _vp]),
    "pda_ssm_adam_step_f32": (_i, [_vp] * 5 + [_sz] + [_vp] * 5 + [_sz] + [_vp] * 3 + [_i, _i, _i, _f, _i, _f, _f, _i, _f, _f, _f, _f, _i, _i, _vp, _vp]),
    "pda_ssm_sample": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _i, _i, _u64, _u64, _vp, _vp, _vp]),
    "pda_ssm_sample_dev": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _i, _i, _u64, _vp, _vp, _vp, _vp, _vp]),
    "pda_ssm_normalize_rows_f32": (_i, [_vp, _sz, _i, _vp, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_inbatch.h (the in-batch softmax: `--train ssm --ssm_source batch`)
INBATCH_MAX_B = 16384
INBATCH_ROW_TILE = 32
INBATCH_COL_TILE = 32
INBATCH_SIGNATURES = {
    "pda_inbatch_col_splits": (_i, [_i]),
    "pda_inbatch_workspace_bytes": (_sz, [_i, _i]),
    "pda_inbatch_mask": (_i, [_vp, _vp, _i, _vp, _vp, _sz, _sz, _vp, _vp]),
    "pda_inbatch_step_f32": (_i, [_vp, _vp, _sz, _sz, _vp, _vp, _i, _i, _f, _i, _vp, _vp, _f, _f] + [_vp] * 4 + [_i, _i, _vp, _sz, _vp, _vp]),
    "pda_inbatch_adam_step_f32": (_i, [_vp] * 5 + [_sz] + [_vp] * 5 + [_sz] + [_vp, _vp, _i, _i, _f, _i, _vp, _vp, _f, _f, _i, _f, _f, _f, _f, _i, _i,
                                       _vp, _sz, _vp, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_dns.h (dynamic hard-negative sampling: `--neg_sampler dns`)
DNS_MAX_CANDIDATES = 256
_dns_head = [_vp, _vp, _sz, _sz, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _u64]
DNS_SIGNATURES = {
    "pda_dns_sample_f32": (_i, _dns_head + [_u64] + [_vp] * 8),
    "pda_dns_sample_f32_dev": (_i, _dns_head + [_vp, _vp] + [_vp] * 8),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_ials.h (the iALS baseline: `--train ials`)
IALS_CHUNK = 4096
IALS_GRAM_ROWS = 256
IALS_SIGNATURES = {
    "pda_ials_workspace_bytes": (_sz, [_sz, _i]),
    "pda_ials_gram_f32": (_i, [_vp, _sz, _i, _vp, _vp, _sz, _vp]),
    "pda_ials_half_sweep_f32": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _vp, _i, _f, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "pda_ials_loss_f32": (_i, [_vp, _vp, _sz, _sz, _vp, _vp, _sz, _vp, _i, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_fullsm.h (the full-catalogue softmax: `--train ssm --ssm_source all`)
FULLSM_MAX_B = 16384
FULLSM_ROW_TILE = 32
FULLSM_COL_TILE = 32
FULLSM_SIGNATURES = {
    "pda_fullsm_col_splits": (_i, [_sz, _i]),
    "pda_fullsm_workspace_bytes": (_sz, [_i, _sz, _i]),
    "pda_fullsm_step_f32": (_i, [_vp, _vp, _sz, _sz, _vp, _vp, _i, _i, _f, _i, _vp, _vp, _f, _f] + [_vp] * 4 + [_i, _i, _vp, _sz, _vp, _vp, _vp]),
    "pda_fullsm_adam_step_f32": (_i, [_vp] * 5 + [_sz] + [_vp] * 5 + [_sz] + [_vp, _vp, _i, _i, _f, _i, _vp, _vp, _f, _f, _i, _f, _f, _f, _f, _i, _i,
                                      _vp, _sz, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_rank.h (exact ranks of held-out items: `--rank_report 1`)
RANK_TCHUNK = 32
_rank_head = [_vp] * 4 + [_i, _i, _i, _i, _vp, _vp, _i]
RANK_SIGNATURES = {
    "pda_rank_keys_f32": (_i, _rank_head + [_vp, _vp, _i, _vp, _vp]),
    "pda_rank_keys_bf16": (_i, _rank_head + [_vp, _vp, _i, _vp, _vp]),
    "pda_rank_count_f32": (_i, _rank_head + [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "pda_rank_count_bf16": (_i, _rank_head + [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_pcc.h (the popularity-correlation regulariser: `--train pcc`)
PCC_ON_POS, PCC_ON_MARGIN = 0, 1
PCC_STAT_WORDS = 8
PCC_SIGNATURES = {
    "pda_pcc_stats_f32": (_i, [_vp, _vp, _sz, _sz] + [_vp] * 4 + [_i, _i, _i, _vp, _vp, _vp]),
    "pda_pcc_step_f32": (_i, [_vp, _vp, _sz, _sz] + [_vp] * 6 + [_i, _i, _f, _i, _f, _f] + [_vp] * 4 + [_i, _i, _vp, _vp, _vp]),
    "pda_pcc_adam_step_f32": (_i, [_vp] * 5 + [_sz] + [_vp] * 5 + [_sz] + [_vp] * 6 + [_i, _i, _f, _i, _f, _f, _i, _f, _f, _f, _f, _i, _i, _vp, _vp,
                                   _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_dau.h (the DirectAU loss: `--train dau`)
DAU_MAX_B = 16384
DAU_MAX_T = 20.0
DAU_TILE = 32
DAU_SAME_KEEP, DAU_SAME_DROP = 0, 1
DAU_STAT_WORDS = 4
DAU_SIGNATURES = {
    "pda_dau_col_splits": (_i, [_i]),
    "pda_dau_workspace_bytes": (_sz, [_i, _i]),
    "pda_dau_step_f32": (_i, [_vp, _vp, _sz, _sz, _vp, _vp, _i, _i, _f, _f, _i, _f, _f] + [_vp] * 4 + [_i, _i, _vp, _sz, _vp, _vp, _vp]),
    "pda_dau_adam_step_f32": (_i, [_vp] * 5 + [_sz] + [_vp] * 5 + [_sz] + [_vp, _vp, _i, _i, _f, _f, _i, _f, _f, _i, _f, _f, _f, _f, _i, _i, _vp, _sz,
                                   _vp, _vp, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_negpop.h (popularity-weighted negatives: `--neg_sampler pop`)
_negpop_head = [_vp, _i, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _u64]
NEGPOP_SIGNATURES = {
    "pda_negpop_sample_triplets": (_i, _negpop_head + [_u64] + [_vp] * 5),
    "pda_negpop_sample_triplets_dev": (_i, _negpop_head + [_vp, _vp] + [_vp] * 5),
    "pda_negpop_sample_batches_dev": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _u64, _vp, _vp] + [_vp] * 5),
    "pda_negpop_ssm_sample": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _i, _i, _vp, _u64, _u64, _vp, _vp, _vp]),
    "pda_negpop_ssm_sample_dev": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _i, _i, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "pda_ssm_step_logq_f32": (_i, [_vp, _vp, _sz, _sz] + [_vp] * 4 + [_i, _i, _i, _f, _i, _f, _f] + [_vp] * 4 + [_i, _i, _vp, _vp]),
    "pda_ssm_adam_step_logq_f32": (_i, [_vp] * 5 + [_sz] + [_vp] * 5 + [_sz] + [_vp] * 4 + [_i, _i, _i, _f, _i, _f, _f, _i, _f, _f, _f, _f, _i, _i, _vp,
                                        _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_ialspp.h (iALS++: `--train ials --ials_solver block`)
IALSPP_SIGNATURES = {
    "pda_ialspp_predict_f32": (_i, [_vp, _vp, _sz, _sz, _vp, _vp, _sz, _i, _vp, _vp]),
    "pda_ialspp_block_pass_f32": (_i, [_vp, _vp, _vp, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                                       _vp, _sz, _vp]),
    "pda_ialspp_gram_f32": (_i, [_vp, _sz, _i, _vp, _vp, _sz, _vp]),
    "pda_ialspp_loss_f32": (_i, [_vp, _vp, _sz, _sz, _vp, _vp, _sz, _vp, _i, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_ials_itemw.h (item-weighted iALS: `--train ials --ials_item_power`)
IALS_ITEMW_SIGNATURES = {
    "pda_ials_gram_scaled_f32": (_i, [_vp, _vp, _sz, _i, _vp, _vp, _sz, _vp]),
    "pda_ialspp_gram256_scaled_f32": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _vp]),
    "pda_ials_half_sweep_rowalpha_f32": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "pda_ialspp_block_pass_rowalpha_f32": (_i, [_vp, _vp, _vp, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                _sz, _vp, _sz, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_calib.h (calibrated-popularity re-ranking, `python -m pda_amd.calib`)
CALIB_MAX_G = 8
CALIB_MAX_K = 64
CALIB_MAX_N = 1024
CALIB_MAX_KS = 8
CALIB_JS, CALIB_KL = 0, 1
CALIB_SIGNATURES = {
    "pda_calib_profile": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp]),
    "pda_calib_list_counts": (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "pda_calib_rerank": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _d, _i, _d, _i, _vp, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); exactly the declarations of include/pda_hip_warp.h (the WARP loss: `--train warp`)
WARP_MAX_TRIALS = 256
_warp_head = [_vp, _vp, _sz, _sz, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _u64]
WARP_SIGNATURES = {
    "pda_warp_sample_f32": (_i, _warp_head + [_u64] + [_vp] * 11),
    "pda_warp_sample_f32_dev": (_i, _warp_head + [_vp, _vp] + [_vp] * 11),
    "pda_warp_step_f32": (_i, [_vp, _vp, _sz, _sz] + [_vp] * 4 + [_f, _i, _i, _f, _f] + [_vp] * 4 + [_i, _i, _vp, _vp]),
    "pda_warp_adam_step_f32": (_i, [_vp] * 5 + [_sz] + [_vp] * 5 + [_sz] + [_vp] * 4 + [_f, _i, _i, _f, _f, _i, _f, _f, _f, _f, _i, _i, _vp, _vp]),
}

_lib = None


class PdaHipError(RuntimeError):
    pass


def load():
    """Load (once) and type every entry point.  Raises if the library or a symbol is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PdaHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C pda_amd/csrc`.  pda_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(SIGNATURES.items()) + list(TEMP_POP_SIGNATURES.items()) + list(PC_SIGNATURES.items()) + \
            list(DET_SIGNATURES.items()) + list(DEEP_SIGNATURES.items()) + list(XQUAD_SIGNATURES.items()) + list(DICE_SIGNATURES.items()) + \
            list(IPS_SIGNATURES.items()) + list(MACR_SIGNATURES.items()) + list(GCN_SIGNATURES.items()) + list(EXPOSURE_SIGNATURES.items()) + \
            list(SSM_SIGNATURES.items()) + list(INBATCH_SIGNATURES.items()) + list(DNS_SIGNATURES.items()) + list(IALS_SIGNATURES.items()) + \
            list(FULLSM_SIGNATURES.items()) + list(RANK_SIGNATURES.items()) + list(PCC_SIGNATURES.items()) + \
            list(DAU_SIGNATURES.items()) + list(NEGPOP_SIGNATURES.items()) + list(IALSPP_SIGNATURES.items()) + list(CALIB_SIGNATURES.items()) + \
            list(WARP_SIGNATURES.items()) + list(IALS_ITEMW_SIGNATURES.items()):
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise PdaHipError(f"libpda_hip.so does not export {name}") from e
        fn.restype, fn.argtypes = res, args
    got = lib.pda_abi_version()
    if got != ABI_VERSION:
        raise PdaHipError(f"libpda_hip.so ABI {got} != binding ABI {ABI_VERSION}")
    _lib = lib
    return lib


def check(code: int, what: str):
    if code != 0:
        msg = load().pda_error_string(code).decode()
        raise PdaHipError(f"{what}: {msg} ({code})")


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
