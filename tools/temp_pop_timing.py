"""BPRMF(t)-pop timings on one GPU (device events, warm-up), one JSON object on stdout:
  step   the temp_pop step (pda_temp_pop_adam_step_f32) against pda_adam_step_f32 on the same U / I tables (Douban shape: 47 890 x 26 047,
         d = 64, B = 2 048, T = 10)
  score  one 262 144-user block at C3 shape (1 M x 200 k x 128) through the pre-filtered bias-head kernel, the exact one, and the raw head
         through generation 3 in natural order
  eval   a whole --test temp_pop evaluation pass at Douban shape: every one of the 47 890 users scored, masked (about 20 train items each)
         and ranked through the library's choice of bias kernel, in 2 048-user blocks (the reference's) and in one block
Usage: python tools/temp_pop_timing.py [--reps N] [--only step|score|eval]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pda_amd import ops  # noqa: E402


def timed(fn, reps, warm=3):
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", choices=("step", "score", "eval"), default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    out = {}
    nU, nI, d, B, T = 47890, 26047, 64, 2048, 10
    U = torch.randn(nU, d, device=dev, generator=g) * 0.1
    I = torch.randn(nI, d, device=dev, generator=g) * 0.1
    bu = torch.randn(nU, 1, device=dev, generator=g) * 0.1
    C = torch.randn(nI, T + 1, device=dev, generator=g) * 0.1
    users = torch.randperm(nU, device=dev, generator=g)[:B].int()
    pos = torch.randint(0, nI, (B,), device=dev, generator=g).int()
    neg = torch.randint(0, nI, (B,), device=dev, generator=g).int()
    temps = torch.randint(0, T, (B,), device=dev, generator=g).float()
    st = ops.TempPopState(U, I, bu, C)
    loss = torch.zeros(3, device=dev)
    k = [0]

    def tp():
        k[0] += 1
        ops.temp_pop_adam_step(U, I, bu, C, users, pos, neg, temps, st, regs=1e-2, reg_div=B, step=k[0], lr_t=1e-4, loss_acc=loss)
    U2, I2 = U.clone(), I.clone()
    z = torch.zeros_like
    mU, vU, gU, mI, vI, gI = z(U2), z(U2), z(U2), z(I2), z(I2), z(I2)
    tagU, tagI = ops.adam_row_tags(nU, nI, dev)
    j = [0]

    def pd():
        j[0] += 1
        ops.adam_step(U2, mU, vU, gU, tagU, I2, mI, vI, gI, tagI, users, pos, neg, regs=1e-2, reg_div=B, step=j[0], lr_t=1e-4, loss_acc=loss)
    if a.only in (None, "step"):
        out["step_temp_pop_ms"] = timed(tp, a.reps)
        out["step_adam_pd_ms"] = timed(pd, a.reps)
        out["step_ratio"] = out["step_temp_pop_ms"] / out["step_adam_pd_ms"]
    if a.only in (None, "eval"):
        from pda_amd.model_api import BPRMFTempPop  # noqa: F401  (the evaluation path of the trainer: alpha per 2 048 users, beta per item)
        lens = torch.randint(10, 31, (nU,), device=dev, generator=g)
        indptr = torch.zeros(nU + 1, dtype=torch.int64, device=dev)
        indptr[1:] = torch.cumsum(lens, 0)
        idx = torch.sort(torch.randint(0, nI, (nU, 30), device=dev, generator=g).int(), dim=1).values
        keep = torch.arange(30, device=dev)[None, :] < lens[:, None]
        hist = ops.HistoryCSR(indptr, idx[keep].contiguous(), by_user=True)
        allu = torch.arange(nU, dtype=torch.int32, device=dev)
        beta = (C[:, T - 1] + C[:, T]).contiguous()
        first = torch.div(torch.arange(nU, device=dev), 2048, rounding_mode="floor") * 2048
        alpha = (bu.view(-1)[first] + 1.0).contiguous()

        def eval_pass(block):
            for i in range(0, nU, block):
                ops.recommend_topk_bias(U, I, allu[i:i + block], alpha[i:i + block].contiguous(), beta, 50, hist)
        out["eval_pass_blocks_2048_ms"] = timed(lambda: eval_pass(2048), max(3, a.reps // 10), warm=1)
        out["eval_pass_one_block_ms"] = timed(lambda: eval_pass(nU), max(3, a.reps // 10), warm=1)
    del U, I, U2, I2, st, mU, vU, gU, mI, vI, gI
    if a.only not in (None, "score"):
        print(json.dumps(out))
        return

    nU, nI, d, nb = 1 << 20, 200000, 128, 262144
    U = torch.randn(nU, d, device=dev, generator=g) * 0.1
    I = torch.randn(nI, d, device=dev, generator=g) * 0.1
    users = torch.randperm(nU, device=dev, generator=g)[:nb].int()
    alpha = torch.rand(nb, device=dev, generator=g) + 0.5
    beta = torch.randn(nI, device=dev, generator=g) * 0.1
    os.environ["PDA_TEMP_POP_KERNEL"] = "prefiltered"
    out["score_prefiltered_bias_ms"] = timed(lambda: ops.recommend_topk_bias(U, I, users, alpha, beta, 50, None), max(3, a.reps // 10), warm=1)
    os.environ["PDA_TEMP_POP_KERNEL"] = "exact"
    out["score_exact_bias_ms"] = timed(lambda: ops.recommend_topk_bias(U, I, users, alpha, beta, 50, None), max(3, a.reps // 10), warm=1)
    del os.environ["PDA_TEMP_POP_KERNEL"]
    os.environ["PDA_SCORE_KERNEL"] = "v3"
    out["score_raw_gen3_natural_ms"] = timed(lambda: ops.topk_merge(ops.score_topk_keys(U, I, users, 50, ops.HEAD_RAW, None, None, prune=False), users), max(3, a.reps // 10), warm=1)
    out["prefiltered_vs_raw_gen3"] = out["score_prefiltered_bias_ms"] / out["score_raw_gen3_natural_ms"]
    out["exact_vs_prefiltered"] = out["score_exact_bias_ms"] / out["score_prefiltered_bias_ms"]
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
