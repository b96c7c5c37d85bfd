"""DICE timings on one GPU (device events around HIP-graph replays, warm-up), one JSON object on stdout:
  step     pda_dice_adam_step_f32 (--embed_size 64: rows of 128 floats) against pda_adam_step_f32 at d = 128 on tables of the same bytes
           (C2 shape: 50 000 x 20 000), 2 048 triplets per step
  sampler  pda_dice_sample_dev (PNSM) against pda_sample_triplets_dev on the same train CSR (C2 shape, 150 train items per user on average,
           Zipf item popularity), 2 048 triplets per batch
Each pair is captured in two HIP graphs of --steps launches and replayed in --runs alternating runs inside this process; the figures are
microseconds per step (per batch): the median over the runs and their range.  The DICE graph alternates two step tags, so that every replayed
step finds the other tag on its rows and lists them again (a replay with one tag would skip the L_dis pass).
Usage: python tools/dice_timing.py [--runs 5] [--steps 20] [--replays 400] [--only step|sampler]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pda_amd import ops  # noqa: E402


def capture(fn):
    """fn() enqueues the launches: -> a graph of them (captured on a side stream, after one direct run that loads the code objects)."""
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            fn()
    torch.cuda.synchronize()
    return g


def replay_us(g, replays, steps, warm=3):
    for _ in range(warm):
        g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (replays * steps)


def alternate(a, b, runs, replays, steps):
    ta, tb = [], []
    for _ in range(runs):
        ta.append(replay_us(a, replays, steps))
        tb.append(replay_us(b, replays, steps))
    return ta, tb


def summary(name, xs, out):
    out[name + "_us"] = statistics.median(xs)
    out[name + "_range_us"] = [min(xs), max(xs)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="launches per captured graph (even)")
    ap.add_argument("--replays", type=int, default=400)
    ap.add_argument("--only", choices=("step", "sampler"), default=None)
    a = ap.parse_args()
    if a.steps % 2:
        raise SystemExit("--steps must be even (two step tags, two counter slots)")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    nU, nI, d, B = 50_000, 20_000, 64, 2048
    out = {"shape": [nU, nI], "B": B, "dice_embed_size": d, "bpr_embed_size": 2 * d, "runs": a.runs, "steps_per_graph": a.steps, "replays": a.replays}

    # one train CSR for both halves: Zipf popularity, 100 .. 200 sorted items per user
    w = 1.0 / torch.arange(1, nI + 1, device=dev, dtype=torch.float32)
    L = 200
    items = torch.multinomial(w, nU * L, replacement=True, generator=gen).view(nU, L).int()
    lens = torch.randint(100, L + 1, (nU,), device=dev, generator=gen)
    keep = torch.arange(L, device=dev)[None, :] < lens[:, None]
    rows = torch.where(keep, items, torch.full_like(items, nI))        # (dropped slots sort behind the kept ones)
    rows = torch.sort(rows, dim=1).values
    indices = rows[keep].contiguous()
    indptr = torch.zeros(nU + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(lens, 0)
    dp = ops.DicePop(indices, nI)
    margin = torch.tensor([40.0], dtype=torch.float32, device=dev)

    if a.only in (None, "step"):
        # a PNSM batch (popular positives, as in training) for both steps
        users, pos, neg, mask = ops.dice_sample(indptr, indices, dp, B, margin=40.0, seed=2020, step=1, n_pool=nU)
        out["mask_share"] = float(mask.float().mean())
        U = torch.randn(nU, 2 * d, device=dev, generator=gen) * 0.1
        I = torch.randn(nI, 2 * d, device=dev, generator=gen) * 0.1
        st = ops.DiceState(U, I)
        st.ws(B)
        loss = torch.zeros(6, device=dev)

        def dice():
            for k in range(a.steps):
                ops.dice_adam_step(U, I, users, pos, neg, mask, st, w_int=0.1, w_con=0.1, dis_pen=0.01, regs=1e-2, reg_div=B, step=1 + (k & 1),
                                   lr_t=1e-4, loss_acc=loss)
        U2, I2 = U.clone(), I.clone()
        z = torch.zeros_like
        mU, vU, gU, mI, vI, gI = z(U2), z(U2), z(U2), z(I2), z(I2), z(I2)
        tagU, tagI = ops.adam_row_tags(nU, nI, dev)
        loss3 = torch.zeros(3, device=dev)

        def bpr():
            for k in range(a.steps):
                ops.adam_step(U2, mU, vU, gU, tagU, I2, mI, vI, gI, tagI, users, pos, neg, regs=1e-2, reg_div=B, step=1 + (k & 1), lr_t=1e-4,
                              loss_acc=loss3)
        gd, gb = capture(dice), capture(bpr)
        td, tb = alternate(gd, gb, a.runs, a.replays, a.steps)
        summary("step_dice", td, out)
        summary("step_bpr", tb, out)
        out["step_ratio"] = out["step_dice_us"] / out["step_bpr_us"]
        out["step_ratio_range"] = [min(x / y for x, y in zip(td, tb)), max(x / y for x, y in zip(td, tb))]
        out["distinct_rows"] = st.rows_ws[:2].tolist()
        del gd, gb

    if a.only in (None, "sampler"):
        mk = lambda dt: torch.empty(B, dtype=dt, device=dev)      # noqa: E731
        od = (mk(torch.int32), mk(torch.int32), mk(torch.int32), mk(torch.uint8))
        ob = (mk(torch.int32), mk(torch.int32), mk(torch.int32), None, None)
        cd = torch.tensor([1, 0], dtype=torch.int64, device=dev)
        cb = torch.tensor([1, 0], dtype=torch.int64, device=dev)

        def pnsm():
            for k in range(a.steps):
                ops.dice_sample_into(od, indptr, indices, dp, margin_dev=margin, seed=2020, step_dev=cd, parity=k & 1, n_pool=nU)

        def plain():
            for k in range(a.steps):
                ops.sample_triplets_into(ob, indptr, indices, seed=2020, step_dev=cb, parity=k & 1, n_pool=nU, neg_range=(0, nI))
        gp, gq = capture(pnsm), capture(plain)
        tp, tq = alternate(gp, gq, a.runs, a.replays, a.steps)
        summary("sample_pnsm", tp, out)
        summary("sample_plain", tq, out)
        out["sample_ratio"] = out["sample_pnsm_us"] / out["sample_plain_us"]
        out["sample_ratio_range"] = [min(x / y for x, y in zip(tp, tq)), max(x / y for x, y in zip(tp, tq))]
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
