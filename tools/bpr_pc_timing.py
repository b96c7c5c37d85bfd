"""BPR-PC timings on one GPU (device events, warm-up), one JSON object on stdout:
  douban  Douban shape (47 890 x 26 047, d = 64, ~20 train items per user, by-user-id history): the item moments, the per-user statistics
          and the PC score call (sweep + finish) of one 2 048-user block, and of a whole evaluation set (every user) in 2 048-user blocks
  c3      one 262 144-user block at C3 shape (1 M x 200 k x 128, no history): moments, statistics, the PC score call, and the exact
          generation-1 bias-head kernel (score_topk_kernel<128, 2>, the temp_pop exact path) on the same shape for comparison
Kernel-level splits (sweep against finish) come from a rocprofv3 --kernel-trace --stats run of this tool (profiles/bpr_pc_score.txt).
Usage: python tools/bpr_pc_timing.py [--reps N] [--only douban|c3]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pda_amd import ops  # noqa: E402


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=("douban", "c3"), default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    out = {}
    alpha, beta, K = 0.1, 0.1, 50
    if a.only in (None, "douban"):
        nU, nI, d = 47890, 26047, 64
        U = torch.randn(nU, d, device=dev, generator=g) * 0.1
        I = torch.randn(nI, d, device=dev, generator=g) * 0.1
        pop = torch.randint(1, 500, (nI,), device=dev, generator=g).float()
        lens = torch.randint(10, 31, (nU,), device=dev, generator=g)
        indptr = torch.zeros(nU + 1, dtype=torch.int64, device=dev)
        indptr[1:] = torch.cumsum(lens, 0)
        idx = torch.sort(torch.randint(0, nI, (nU, 30), device=dev, generator=g).int(), dim=1).values
        keep = torch.arange(30, device=dev)[None, :] < lens[:, None]
        hist = ops.HistoryCSR(indptr, idx[keep].contiguous(), by_user=True)
        allu = torch.arange(nU, dtype=torch.int32, device=dev)
        mom = ops.pc_item_moments(I, pop)
        k = ops.pc_user_stats(U, I, allu, pop, beta, hist, mom)[2]
        blk = allu[:2048]
        out["douban_moments_ms"] = timed(lambda: ops.pc_item_moments(I, pop), a.reps)
        out["douban_stats_block_ms"] = timed(lambda: ops.pc_user_stats(U, I, blk, pop, beta, hist, mom), a.reps)
        out["douban_stats_all_ms"] = timed(lambda: ops.pc_user_stats(U, I, allu, pop, beta, hist, mom), a.reps)
        stats = {}
        out["douban_score_block_ms"] = timed(lambda: ops.recommend_topk_pc(U, I, blk, pop, k[:2048], alpha, beta, K, hist, stats=stats), a.reps)
        out["douban_score_block_fallback_rows"] = stats["pc_fallback_rows"]

        def eval_pass():
            for i in range(0, nU, 2048):
                ops.recommend_topk_pc(U, I, allu[i:i + 2048], pop, k[i:i + 2048], alpha, beta, K, hist)
        out["douban_score_all_blocks_2048_ms"] = timed(eval_pass, max(2, a.reps // 5), warm=1)
        del U, I, hist, k
    if a.only in (None, "c3"):
        nU, nI, d, nb = 1 << 20, 200000, 128, 262144
        U = torch.randn(nU, d, device=dev, generator=g) * 0.1
        I = torch.randn(nI, d, device=dev, generator=g) * 0.1
        pop = torch.randint(1, 5000, (nI,), device=dev, generator=g).float()
        users = torch.randperm(nU, device=dev, generator=g)[:nb].int()
        reps = max(2, a.reps // 5)
        mom = ops.pc_item_moments(I, pop)
        k = ops.pc_user_stats(U, I, users, pop, beta, None, mom)[2]
        out["c3_moments_ms"] = timed(lambda: ops.pc_item_moments(I, pop), reps, warm=1)
        out["c3_stats_ms"] = timed(lambda: ops.pc_user_stats(U, I, users, pop, beta, None, mom), reps, warm=1)
        stats = {}
        out["c3_score_ms"] = timed(lambda: ops.recommend_topk_pc(U, I, users, pop, k, alpha, beta, K, None, stats=stats), reps, warm=1)
        out["c3_score_fallback_rows"] = stats["pc_fallback_rows"]
        alpha_t = torch.rand(nb, device=dev, generator=g) + 0.5
        beta_t = torch.randn(nI, device=dev, generator=g) * 0.1
        os.environ["PDA_TEMP_POP_KERNEL"] = "exact"
        out["c3_exact_bias_head_ms"] = timed(lambda: ops.recommend_topk_bias(U, I, users, alpha_t, beta_t, K, None), reps, warm=1)
        del os.environ["PDA_TEMP_POP_KERNEL"]
        out["c3_score_vs_exact_bias"] = out["c3_score_ms"] / out["c3_exact_bias_head_ms"]
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
