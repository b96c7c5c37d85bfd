"""IPS timings on one GPU (device events around HIP-graph replays, warm-up), one JSON object on stdout:
  pda_ips_adam_step_f32 for IPS, IPS-C (clip 8) and IPS-CN (clip 8, self-normalised) against pda_adam_step_f32, the plain BPR step, on the C2
  tables (50 000 x 20 000 x 64), 2 048 triplets per step with Zipf positives, the same batch for all four.
The outputs are compared first: with every weight one the IPS step must give the gradients and the loss of the BPR step (1e-5), and every variant's loss must
equal its float64 value computed by torch on the device (1e-5 max(1, w_max)); a mismatch ends the run before anything is timed.
The four steps are captured in four HIP graphs of --steps launches and replayed in --runs alternating runs inside this process; the figures
are microseconds per step: the median over the runs and their range, and each variant's ratio to the BPR step run by run.
Usage: python tools/ips_timing.py [--runs 5] [--steps 20] [--replays 400]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pda_amd import ops  # noqa: E402

VARIANTS = {"ips": (0.0, False), "ips_c": (8.0, False), "ips_cn": (8.0, True)}


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


class Tables:
    def __init__(self, U, I):
        z = torch.zeros_like
        self.U, self.I = U.clone(), I.clone()
        self.mU, self.vU, self.gU, self.mI, self.vI, self.gI = z(U), z(U), z(U), z(I), z(I), z(I)
        self.tagU, self.tagI = ops.adam_row_tags(U.shape[0], I.shape[0], U.device)
        self.wsum = torch.zeros(1, dtype=torch.float32, device=U.device)
        self.loss = torch.zeros(3, device=U.device)

    def state(self):
        return (self.U, self.mU, self.vU, self.gU, self.tagU, self.I, self.mI, self.vI, self.gI, self.tagI)


def loss64(U, I, users, pos, neg, ipw, norm, regs, B):
    u, p, n = U[users.long()].double(), I[pos.long()].double(), I[neg.long()].double()
    w = ipw[pos.long()].double()
    ls = torch.log(torch.sigmoid((u * p).sum(1) - (u * n).sum(1)) + 1e-10)
    mf = -(w * ls).sum() / (w.sum() if norm else B)
    reg = regs * 0.5 * ((u ** 2).sum() + (p ** 2).sum() + (n ** 2).sum()) / B
    return torch.stack([mf + reg, mf, reg])


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
    nU, nI, d, B, regs = 50_000, 20_000, 64, 2048, 1e-2
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
    weights = {k: ops.IpsWeights(indices, nI, clip=c).ipw for k, (c, _) in VARIANTS.items()}
    out["batch_w_max"] = {k: float(weights[k][pos.long()].max()) for k in VARIANTS}

    # ---- outputs first
    one, ref = Tables(U, I), Tables(U, I)
    ops.ips_grads(one.U, one.I, users, pos, neg, torch.ones(nI, device=dev), one.gU, one.gI, one.tagU, one.tagI, regs=regs, reg_div=B, step=1,
                  loss_acc=one.loss)
    ops.bpr_step(ref.U, ref.I, users, pos, neg, regs=regs, reg_div=B, mode=ops.UPD_DENSE_GRAD, gU=ref.gU, gI=ref.gI, loss_acc=ref.loss)
    out["unit_weights_max_diff"] = max(float((one.gU - ref.gU).abs().max()), float((one.gI - ref.gI).abs().max()), float((one.loss - ref.loss).abs().max()))
    ok = out["unit_weights_max_diff"] <= 1e-5
    out["loss_err"] = {}
    for k, (_, norm) in VARIANTS.items():
        t = Tables(U, I)
        ops.ips_grads(t.U, t.I, users, pos, neg, weights[k], t.gU, t.gI, t.tagU, t.tagI, wsum=t.wsum if norm else None, regs=regs, reg_div=B, step=1,
                      loss_acc=t.loss)
        err = float((t.loss.double() - loss64(U, I, users, pos, neg, weights[k], norm, regs, B)).abs().max())
        out["loss_err"][k] = err
        ok = ok and err <= 1e-5 * (1.0 if norm else max(1.0, out["batch_w_max"][k]))
    if not ok:
        out["error"] = "outputs differ: nothing timed"
        print(json.dumps(out))
        raise SystemExit(1)

    # ---- then the time
    graphs, keepalive = {}, []

    def stepper(name):
        t = Tables(U, I)
        keepalive.append(t)
        if name == "bpr":
            def run():
                for k in range(a.steps):
                    ops.adam_step(*t.state(), users, pos, neg, regs=regs, reg_div=B, step=1 + (k & 1), lr_t=1e-4, loss_acc=t.loss)
        else:
            norm = VARIANTS[name][1]

            def run():
                for k in range(a.steps):
                    ops.ips_adam_step(*t.state(), users, pos, neg, weights[name], wsum=t.wsum if norm else None, regs=regs, reg_div=B,
                                      step=1 + (k & 1), lr_t=1e-4, loss_acc=t.loss)
        return run
    names = ["bpr"] + list(VARIANTS)
    for n in names:
        graphs[n] = capture(stepper(n))
    times = {n: [] for n in names}
    for _ in range(a.runs):
        for n in names:
            times[n].append(replay_us(graphs[n], a.replays, a.steps))
    for n in names:
        out["step_%s_us" % n] = statistics.median(times[n])
        out["step_%s_range_us" % n] = [min(times[n]), max(times[n])]
    for n in VARIANTS:
        r = [x / y for x, y in zip(times[n], times["bpr"])]
        out["ratio_%s" % n] = statistics.median(r)
        out["ratio_%s_range" % n] = [min(r), max(r)]
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
