"""MACR timings on one GPU (device events, warm-up), one JSON object on stdout, on the C2 tables (50 000 x 20 000 x 64), 2 048 triplets per step
with Zipf positives:
  step   pda_macr_adam_step_f32 against pda_adam_step_f32, the plain BPR step, on the same tables and the same batch: each captured in a HIP
         graph of --steps launches and replayed in --runs alternating runs inside this process; microseconds per step, the median over the runs,
         their range, and the ratio run by run.
  eval   one evaluation pass over the grid of c for all users against one bias-head sweep over the same users: macr_item_prep +
         pda_item_prep_f32 of J + 21 x (the bias launch + the sweep: c = 0 and linspace(-1, 1, 20)), against recommend_topk_bias once.  Direct
         launches between device events (a sweep is milliseconds), the same alternating runs.
The outputs are compared first: the step's five loss terms and its gW against float64 torch autograd on the device (1e-5), and for 512 users the
values of a MACR list against torch.topk of fl(score_dense(U, J) + beta) (bit-equal); a mismatch ends the run before anything is timed.
Usage: python tools/macr_timing.py [--runs 5] [--steps 20] [--replays 400]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pda_amd import ops  # noqa: E402

ALPHA, BETA = 1e-3, 1e-3


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


def direct_ms(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def terms64(U, I, wi, wu, users, pos, neg, regs, B):
    """(loss, L_O, L_I, L_U, reg) and the gradients of the two branch vectors, float64 autograd on the device."""
    wi, wu = wi.double().view(-1).requires_grad_(), wu.double().view(-1).requires_grad_()
    u, p, n = U[users.long()].double(), I[pos.long()].double(), I[neg.long()].double()
    sp, sn, su = torch.sigmoid(p @ wi), torch.sigmoid(n @ wi), torch.sigmoid(u @ wu)
    bce = lambda s, z: (-torch.log(s + 1e-10) - torch.log(1 - z + 1e-10)).sum() / B      # noqa: E731
    lo = bce(torch.sigmoid((u * p).sum(1) * sp * su), torch.sigmoid((u * n).sum(1) * sn * su))
    li, lu = bce(sp, sn), bce(su, su)
    reg = regs * 0.5 * ((u ** 2).sum() + (p ** 2).sum() + (n ** 2).sum()) / B
    loss = lo + ALPHA * li + BETA * lu + reg
    loss.backward()
    return torch.stack([loss, lo, li, lu, reg]).detach(), torch.stack([wi.grad, wu.grad])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="launches per captured graph (even)")
    ap.add_argument("--replays", type=int, default=400)
    a = ap.parse_args()
    if a.steps % 2:
        raise SystemExit("--steps must be even (two step tags)")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    nU, nI, d, B, regs, K = 50_000, 20_000, 64, 2048, 1e-2, 50
    out = {"shape": [nU, nI, d], "B": B, "runs": a.runs, "steps_per_graph": a.steps, "replays": a.replays}

    # a train CSR with Zipf popularity, 100 .. 200 sorted items per user: the batch's positives are popular items, as in training
    w = 1.0 / torch.arange(1, nI + 1, device=dev, dtype=torch.float32)
    L = 200
    items = torch.multinomial(w, nU * L, replacement=True, generator=gen).view(nU, L).int()
    lens = torch.randint(100, L + 1, (nU,), device=dev, generator=gen)
    keep = torch.arange(L, device=dev)[None, :] < lens[:, None]
    rows = torch.sort(torch.where(keep, items, torch.full_like(items, nI)), dim=1).values
    indices = rows[keep].contiguous()
    indptr = torch.zeros(nU + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(lens, 0)
    users, pos, neg = ops.sample_triplets(indptr, indices, B, seed=2020, step=1, n_pool=nU, neg_range=(0, nI))[:3]
    out["distinct_positives"] = int(torch.unique(pos).numel())
    U = torch.randn(nU, d, device=dev, generator=gen) * 0.1
    I = torch.randn(nI, d, device=dev, generator=gen) * 0.1
    wi = torch.randn(d, device=dev, generator=gen) * 1.5       # branch dots of about +-1.2: s from 0.1 to 0.9
    wu = torch.randn(d, device=dev, generator=gen) * 1.5
    hist = ops.HistoryCSR(indptr, indices, by_user=True)
    all_users = torch.arange(nU, dtype=torch.int32, device=dev)
    grid = [0.0] + [float(c) for c in torch.linspace(-1.0, 1.0, 20)]

    # ---- outputs first
    st = ops.MacrState(U, I)
    loss = torch.zeros(5, device=dev)
    ops.macr_grads(U, I, wi, wu, users, pos, neg, st, alpha=ALPHA, beta=BETA, regs=regs, reg_div=B, step=1, loss_acc=loss)
    t64, gW64 = terms64(U, I, wi, wu, users, pos, neg, regs, B)
    out["loss_err"] = float((loss.double() - t64).abs().max())
    out["gW_err"] = float((st.gW.double() - gW64).abs().max())
    prep = ops.macr_item_prep(I, wi)
    some = all_users[:512].contiguous()
    h = ops.score_dense(U, prep.J, some, ops.HEAD_RAW) + ops.macr_item_bias(prep.sig, 0.37)[None, :]
    rowsel = torch.repeat_interleave(torch.arange(512, device=dev), (indptr[1:513] - indptr[:512]))
    h[rowsel, indices[:int(indptr[512])].long()] = float("-inf")
    _, val = ops.recommend_topk_macr(U, I, wi, some, 0.37, K, hist, prep=prep)
    out["list_values_equal"] = bool(torch.equal(val, torch.topk(h, K, dim=1).values))
    if not (out["loss_err"] <= 1e-5 and out["gW_err"] <= 1e-5 and out["list_values_equal"]):
        out["error"] = "outputs differ: nothing timed"
        print(json.dumps(out))
        raise SystemExit(1)

    # ---- the step
    keepalive = []

    def stepper(name):
        Uc, Ic = U.clone(), I.clone()
        lo = torch.zeros(5, device=dev)
        if name == "bpr":
            z = torch.zeros_like
            s = (Uc, z(Uc), z(Uc), z(Uc), ops.adam_row_tags(nU, nI, dev)[0], Ic, z(Ic), z(Ic), z(Ic), ops.adam_row_tags(nU, nI, dev)[1])
            keepalive.append(s)

            def run():
                for k in range(a.steps):
                    ops.adam_step(*s, users, pos, neg, regs=regs, reg_div=B, step=1 + (k & 1), lr_t=1e-4, loss_acc=lo[:3])
        else:
            s, wic, wuc = ops.MacrState(Uc, Ic), wi.clone(), wu.clone()
            keepalive.append((s, Uc, Ic, wic, wuc))

            def run():
                for k in range(a.steps):
                    ops.macr_adam_step(Uc, Ic, wic, wuc, users, pos, neg, s, alpha=ALPHA, beta=BETA, regs=regs, reg_div=B, step=1 + (k & 1),
                                       lr_t=1e-4, loss_acc=lo)
        return run
    names = ["bpr", "macr"]
    graphs = {n: capture(stepper(n)) for n in names}
    times = {n: [] for n in names}
    for _ in range(a.runs):
        for n in names:
            times[n].append(replay_us(graphs[n], a.replays, a.steps))
    for n in names:
        out["step_%s_us" % n] = statistics.median(times[n])
        out["step_%s_range_us" % n] = [min(times[n]), max(times[n])]
    r = [x / y for x, y in zip(times["macr"], times["bpr"])]
    out["step_ratio"] = statistics.median(r)
    out["step_ratio_range"] = [min(r), max(r)]

    # ---- one evaluation pass
    ones, zeros = torch.ones(nU, device=dev), torch.zeros(nI, device=dev)

    def one_sweep():
        ops.mark_modified(I)                                   # (a trained table: its pda_item_prep_f32 is part of the sweep's evaluation, too)
        ops.recommend_topk_bias(U, I, all_users, ones, zeros, K, hist)

    def macr_pass():
        p = ops.macr_item_prep(I, wi, prep)                    # bumps J's version: its pda_item_prep_f32 runs in the first sweep
        for c in grid:
            ops.recommend_topk_macr(U, I, wi, all_users, c, K, hist, prep=p)
    one_sweep(), macr_pass()
    ev = {"sweep": [], "macr_pass": []}
    for _ in range(a.runs):
        ev["sweep"].append(direct_ms(one_sweep))
        ev["macr_pass"].append(direct_ms(macr_pass))
    out["eval_users"], out["eval_values_of_c"] = nU, len(grid)
    for n in ev:
        out["eval_%s_ms" % n] = statistics.median(ev[n])
        out["eval_%s_range_ms" % n] = [min(ev[n]), max(ev[n])]
    r = [x / y for x, y in zip(ev["macr_pass"], ev["sweep"])]
    out["eval_ratio"] = statistics.median(r)
    out["eval_ratio_range"] = [min(r), max(r)]
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
