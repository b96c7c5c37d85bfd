"""Timings of the bit-reproducible training path (`--deterministic 1`, include/pda_hip_det.h) on one GPU; one JSON object on stdout.

  steps    per shape -- c2 (50 000 x 20 000, d = 64), c1 (the Douban shape, 47 890 x 26 047, d = 64), c3 (1 M x 200 k, d = 128, streaming sweep) --
           B = 2 048 triplets per step, 64 batches from the device sampler, their plans computed ahead:
             adam_step       pda_adam_step_f32 (float atomics; PDA_UPD_ANY_ORDER | PDA_UPD_USERS_DISTINCT, as the trainer calls it)
             adam_step_plan  pda_adam_step_plan_f32 (planned gradient + the same sweep: three launches)
             sgd_fused       pda_bpr_step_f32(PDA_UPD_SGD_FUSED)          } the project's own yardstick for what a fixed
             sgd_plan        pda_bpr_step_plan_f32(exact = 1)             } summation order may cost
           every variant on its own copy of the tables, 64 steps captured into a HIP graph; device events around `--steps` (>= 200) warmed steps,
           the variants alternated, three repetitions: median and (min, max) in us per step.
  metrics  pda_metrics against pda_metrics_ordered on 262 144 x 50 lists, the same way.
  default_path_differs   for the record: elements of (U, I, mU, vU, mI, vI) that differ between two runs of three default adam_step calls on the
           B = 2 048 Zipf batches of tests/test_gpu_deterministic.py (50 000 x 20 000, d = 64), and the same count for adam_step_plan (0).
Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/adam_plan_timing.py --only c2 --reps 1` run
(profiles/adam_plan_step.txt).
Usage: python tools/adam_plan_timing.py [--only c2|c1|c3|metrics|differs] [--steps N] [--reps R]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pda_amd import ops, synthetic  # noqa: E402

B, REGS, LR, NB = 2048, 1e-2, 1e-2, 64


class StepGraph:
    """A captured graph together with the tensors its kernels point into: the graph holds raw addresses, and torch.cuda.graph empties the allocator's
    cache before every capture, so a buffer that died with its closure would be unmapped under the graphs captured before."""

    def __init__(self, graph, *alive):
        self.graph, self.alive = graph, alive

    def replay(self):
        self.graph.replay()


def graph_of(body, *alive):
    """64 steps of `body(i)` as one HIP graph (warmed on a side stream first); `alive`: every tensor the steps touch."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for i in range(3):
            body(i)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(NB):
            body(i)
    g.replay()
    torch.cuda.synchronize()
    return StepGraph(g, body, *alive)


def alternate(graphs, steps, reps, per_replay=NB):
    """name -> (median, min, max) us per step; device events around ceil(steps / 64) replays, the variants in turn, `reps` times."""
    n = max(1, -(-steps // per_replay))
    got = {k: [] for k in graphs}
    for _ in range(reps):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            got[k].append(e0.elapsed_time(e1) * 1e3 / (n * per_replay))
    return {k: {"us": statistics.median(v), "min": min(v), "max": max(v)} for k, v in got.items()}


def steps_on(name, dev, steps, reps):
    W = synthetic.make_workload(name, dev)
    batches = [ops.sample_triplets(W.hist_indptr, W.hist_indices, B, seed=2020, step=s, n_pool=W.n_users, train_slots=W.hist_slots,
                                   neg_range=(0, W.n_items), pop_matrix=W.pop_train) for s in range(NB)]
    plans = [ops.triplet_plan(b[0], b[1], b[2])[0].clone() for b in batches]
    loss = torch.zeros(3, device=dev)
    graphs = {}

    def adam(planned):
        U, I = W.U.clone(), W.I.clone()
        st = [torch.zeros_like(t) for t in (U, U, U, I, I, I)]
        tags = ops.adam_row_tags(W.n_users, W.n_items, dev)
        keep = {}

        def body(i):
            t = i % NB + 1
            kw = dict(regs=REGS, reg_div=B, step=t, lr_t=ops.adam_lr_t(LR, t + 100), loss_acc=loss)
            if planned:
                keep["scratch"] = ops.adam_step_plan(U, st[0], st[1], st[2], tags[0], I, st[3], st[4], st[5], tags[1], *batches[i % NB],
                                                     plan=plans[i % NB], scratch=keep.get("scratch"), **kw)
            else:
                ops.adam_step(U, st[0], st[1], st[2], tags[0], I, st[3], st[4], st[5], tags[1], *batches[i % NB], users_distinct=True, **kw)
        return graph_of(body, U, I, st, tags, keep)

    def sgd(planned):
        U, I = W.U.clone(), W.I.clone()
        keep = {}

        def body(i):
            if planned:
                keep["scratch"] = ops.bpr_step_plan(U, I, *batches[i % NB], regs=REGS, reg_div=B, lr=LR, plan=plans[i % NB],
                                                    scratch=keep.get("scratch"), exact=True, loss_acc=loss)
            else:
                ops.bpr_step(U, I, *batches[i % NB], regs=REGS, reg_div=B, lr=LR, mode=ops.UPD_SGD_FUSED, loss_acc=loss, users_distinct=True)
        return graph_of(body, U, I, keep)

    graphs["adam_step"], graphs["adam_step_plan"] = adam(False), adam(True)
    graphs["sgd_fused"], graphs["sgd_plan"] = sgd(False), sgd(True)
    r = alternate(graphs, steps, reps)
    del graphs
    r["adam_plan_over_atomic"] = r["adam_step_plan"]["us"] / r["adam_step"]["us"]
    r["adam_plan_minus_atomic_us"] = r["adam_step_plan"]["us"] - r["adam_step"]["us"]
    r["sgd_plan_minus_fused_us"] = r["sgd_plan"]["us"] - r["sgd_fused"]["us"]
    r["tables"] = "%d x %d, d = %d" % (W.n_users, W.n_items, W.d)
    return r


def metrics_on(dev, steps, reps):
    g = torch.Generator(device=dev).manual_seed(3)
    n, K = 262144, 50
    topk = torch.argsort(torch.rand(n, 64, device=dev, generator=g), dim=1)[:, :K].int().contiguous()
    lens = torch.randint(1, 11, (n,), device=dev, generator=g)
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(lens, 0)
    idx = torch.randint(0, 64, (int(indptr[-1]),), device=dev, generator=g).int()
    ks = torch.tensor([20, 50], dtype=torch.int32, device=dev)
    sums = torch.zeros(4, 2, dtype=torch.float64, device=dev)
    alive = (topk, indptr, idx, ks, sums)
    graphs = {"metrics_sums": graph_of(lambda i: ops.metrics_sums(topk, indptr, idx, ks, sums), *alive),
              "metrics_sums_ordered": graph_of(lambda i: ops.metrics_sums_ordered(topk, indptr, idx, ks, sums), *alive)}
    return alternate(graphs, steps, reps)


def zipf_batch(seed, nU, nI, n):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(nI)
    w = 1.0 / np.arange(1, nI + 1)
    pos = perm[rng.choice(nI, n, p=w / w.sum())].astype(np.int32)
    neg = rng.integers(0, nI, n).astype(np.int32)
    users = rng.permutation(nU)[:n].astype(np.int32)
    rng = np.random.default_rng(1000 + seed)
    return users, pos, neg, (rng.uniform(0, 1, n) ** 0.22).astype(np.float32), (rng.uniform(0, 1, n) ** 0.22).astype(np.float32)


def differs(dev):
    nU, nI, d = 50000, 20000, 64
    rng = np.random.default_rng(5 + B)
    U0 = torch.from_numpy((rng.standard_normal((nU, d)) * 0.1).astype(np.float32)).to(dev)
    I0 = torch.from_numpy((rng.standard_normal((nI, d)) * 0.1).astype(np.float32)).to(dev)
    batches = [[torch.from_numpy(x).to(dev) for x in zipf_batch(seed, nU, nI, B)] for seed in (31, 32, 33)]
    plans = [ops.triplet_plan(b[0], b[1], b[2])[0].clone() for b in batches]

    def run(planned):
        U, I = U0.clone(), I0.clone()
        st = [torch.zeros_like(t) for t in (U, U, U, I, I, I)]
        tags = ops.adam_row_tags(nU, nI, dev)
        for t, b in enumerate(batches, 1):
            kw = dict(regs=REGS, reg_div=B, step=t, lr_t=ops.adam_lr_t(LR, t))
            if planned:
                ops.adam_step_plan(U, st[0], st[1], st[2], tags[0], I, st[3], st[4], st[5], tags[1], *b, plan=plans[t - 1], **kw)
            else:
                ops.adam_step(U, st[0], st[1], st[2], tags[0], I, st[3], st[4], st[5], tags[1], *b, users_distinct=True, **kw)
        torch.cuda.synchronize()
        return [U, I, st[0], st[1], st[3], st[4]]

    out = {"elements": 6 * (nU + nI) * d}
    for planned in (False, True):
        a = run(planned)
        worst, abs_worst = 0, 0.0
        for _ in range(4):
            b = run(planned)
            n = sum(int((x.view(torch.int32) != y.view(torch.int32)).sum()) for x, y in zip(a, b))
            worst = max(worst, n)
            abs_worst = max(abs_worst, max(float((x - y).abs().max()) for x, y in zip(a, b)))
        out["adam_step_plan" if planned else "adam_step"] = {"differing_elements_max_of_4_reruns": worst, "largest_difference": abs_worst}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("c2", "c1", "c3", "metrics", "differs"), default=None)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    for name in ("c2", "c1", "c3"):
        if a.only in (None, name):
            out[name] = steps_on(name, dev, a.steps, a.reps)
            torch.cuda.empty_cache()
    if a.only in (None, "metrics"):
        out["metrics_262144x50"] = metrics_on(dev, a.steps, a.reps)
    if a.only in (None, "differs"):
        out["default_path_differs"] = differs(dev)
    out["steps_per_measurement"], out["reps"] = max(1, -(-a.steps // NB)) * NB, a.reps
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
