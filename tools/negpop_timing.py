"""Popularity-weighted negative sampling timings on one GPU (device events around HIP-graph replays, warm-up), one JSON object on stdout:
  the triplet call pda_negpop_sample_triplets_dev at beta in {0, 0.75, 1} against pda_sample_triplets_dev measured in the same run;
  the look-ahead call pda_negpop_sample_batches_dev (32 batches a launch) per batch, against pda_sample_batches_dev;
  the [B, N] block pda_negpop_ssm_sample_dev at N in {16, 64, 256} against pda_ssm_sample_dev;
  the mean and the largest number of tries per negative, from the restatement tests/negpop_ref.py on the batch of step 1;
  the sampled-softmax Adam step (N = 64, d = 64) with and without logq;
on the train graphs of the C2 shape (50 000 x 20 000) and of the Douban shape (47 890 x 26 047) of pda_amd/synthetic.py, 2 048 rows per batch.
The samplers never read the embedding tables: their figures do not depend on d.
Every shape runs in a child process of its own under its own time limit (--child_timeout seconds); the first child that fails ends the tool
and nothing more is started on the GPU.  Inside a child every call is first compared with its by-value twin; a mismatch ends the child before
anything is timed.  Then every variant is captured in a HIP graph of --steps launches (an even number: the two-slot step counter is back where
it was) and replayed in --runs alternating runs; the figures are microseconds per call: the median over the runs and their range.
Usage: python tools/negpop_timing.py [--runs 5] [--steps 20] [--replays 100] [--shapes c2,c1]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = 2048
BETAS = (0.0, 0.75, 1.0)
AHEAD = 32


def capture(fn):
    """fn() enqueues the launches: -> a graph of them (captured on a side stream, after one direct run that loads the code objects)."""
    import torch
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            fn()
    torch.cuda.synchronize()
    return g


def replay_us(g, replays, per_replay, warm=3):
    import torch
    for _ in range(warm):
        g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (replays * per_replay)


def alternate(graphs, runs, replays, per_replay):
    """{name: graph} -> {name: [median, min, max]} us per call over `runs` runs that take the variants in turn."""
    seen = {k: [] for k in graphs}
    for _ in range(runs):
        for k, g in graphs.items():
            seen[k].append(replay_us(g, replays, per_replay[k] if isinstance(per_replay, dict) else per_replay))
    return {k: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)] for k, v in seen.items()}


def child(a, shape):
    import numpy as np
    import torch
    from pda_amd import ops, synthetic
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import negpop_ref as nr

    dev = torch.device("cuda:0")
    w = synthetic.make_workload(shape, device=dev, d=64)
    nU, nI = w.n_users, w.n_items
    ip, ix, sl, pop = w.hist_indptr, w.hist_indices, w.hist_slots, w.pop_train
    out = {"shape": shape, "n_users": nU, "n_items": nI, "train_pairs": int(w.n_train), "B": B}
    tables = {b: ops.NegPopTable(ix, nI, b, (0, nI), dev) for b in BETAS}
    out["table"] = {str(b): dict(zip(("max_q", "entropy", "uniform_entropy"), (round(x, 6) for x in t.stats()))) for b, t in tables.items()}
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)                # noqa: E731
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)              # noqa: E731
    steps = a.steps + (a.steps & 1)
    kw = dict(seed=2020, n_pool=nU, train_slots=sl, pop_matrix=pop)

    # -- the restatement's tries, and the calls against their by-value twins before anything is timed
    hp, hx, hs, hpop = ip.cpu().numpy(), ix.cpu().numpy(), sl.cpu().numpy(), pop.cpu().numpy()
    out["tries"] = {}
    for b, t in tables.items():
        want = nr.sample(2020, 1, B, hp, hx, t.thr, t.alias, slots=hs, n_pool=nU, pop_matrix=hpop)
        got = ops.negpop_sample_triplets(t, ip, ix, B, step=1, **kw)
        for g, k in zip(got, ("users", "pos", "neg", "pos_pop", "neg_pop")):
            if not np.array_equal(g.cpu().numpy().view(np.int32), want[k].view(np.int32)):
                raise SystemExit("beta %g: %s differs from the restatement" % (b, k))
        out["tries"][str(b)] = {"mean": round(float(1 + want["rejections"].mean()), 3), "max": int(1 + want["rejections"].max())}
    uni = ops.sample_triplets(ip, ix, B, step=1, neg_range=(0, nI), **kw)
    if not all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(uni, ops.negpop_sample_triplets(tables[0.0], ip, ix, B, step=1, **kw))):
        raise SystemExit("beta 0 is not the uniform sampler")

    # -- the triplet call
    ctr = torch.tensor([1, 0], dtype=torch.int64, device=dev)
    buf = (i32(B), i32(B), i32(B), f32(B), f32(B))

    def tri(table):
        def fn():
            for s in range(steps):
                if table is None:
                    ops.sample_triplets_into(buf, ip, ix, step_dev=ctr, parity=s & 1, neg_range=(0, nI), **kw)
                else:
                    ops.negpop_sample_triplets_into(buf, table, ip, ix, step_dev=ctr, parity=s & 1, **kw)
        return fn

    graphs = {"uniform": capture(tri(None))}
    graphs.update({"beta_%g" % b: capture(tri(t)) for b, t in tables.items()})
    out["triplets_us"] = alternate(graphs, a.runs, a.replays, steps)

    # -- the look-ahead call, per batch
    q = (i32(AHEAD, B), i32(AHEAD, B), i32(AHEAD, B), f32(AHEAD, B), f32(AHEAD, B))

    def ahead(table):
        def fn():
            for s in range(2):
                if table is None:
                    ops.sample_batches_into(q, ip, ix, step_dev=ctr, parity=s & 1, neg_range=(0, nI), **kw)
                else:
                    ops.negpop_sample_batches_into(q, table, ip, ix, step_dev=ctr, parity=s & 1, **kw)
        return fn

    graphs = {"uniform": capture(ahead(None))}
    graphs.update({"beta_%g" % b: capture(ahead(t)) for b, t in tables.items()})
    out["ahead_us_per_batch"] = alternate(graphs, a.runs, a.replays, 2 * AHEAD)

    # -- the [B, N] block
    out["block_us"] = {}
    bk = dict(seed=2020, n_pool=nU)
    for N in (16, 64, 256):
        blk = (i32(B), i32(B), i32(B, N))

        def block(table, blk=blk):
            def fn():
                for s in range(steps):
                    if table is None:
                        ops.ssm_sample_into(blk, ip, ix, step_dev=ctr, parity=s & 1, neg_range=(0, nI), **bk)
                    else:
                        ops.negpop_ssm_sample_into(blk, table, ip, ix, step_dev=ctr, parity=s & 1, **bk)
            return fn

        graphs = {"uniform": capture(block(None))}
        graphs.update({"beta_%g" % b: capture(block(t)) for b, t in tables.items()})
        out["block_us"][str(N)] = alternate(graphs, a.runs, a.replays, steps)

    # -- the sampled-softmax Adam step with and without logq (N = 64, d = 64, the negatives of beta = 0.75)
    N = 64
    t = tables[0.75]
    users, pos, negs = ops.negpop_ssm_sample(t, ip, ix, B, N, seed=2020, step=1, n_pool=nU)
    logq = torch.from_numpy(t.logq).to(dev)
    z = torch.zeros_like
    st = dict(mU=z(w.U), vU=z(w.U), gU=z(w.U), mI=z(w.I), vI=z(w.I), gI=z(w.I))
    tagU, tagI = ops.adam_row_tags(nU, nI, dev)
    loss = f32(3)

    def step(lq):
        def fn():
            for k in range(steps):
                ops.ssm_adam_step(w.U, st["mU"], st["vU"], st["gU"], tagU, w.I, st["mI"], st["vI"], st["gI"], tagI, users, pos, negs, tau=0.1, norm=1,
                                  regs=1e-2, reg_div=B, step=1 + (k & 1), lr_t=1e-4, users_distinct=True, loss_acc=loss, logq=lq)
        return fn

    graphs = {"plain": capture(step(None)), "logq": capture(step(logq))}
    out["ssm_adam_step_us"] = alternate(graphs, a.runs, a.replays, steps)
    print(json.dumps(out))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--replays", type=int, default=100)
    p.add_argument("--shapes", default="c2,c1")
    p.add_argument("--child_timeout", type=int, default=240)
    p.add_argument("--child", default="")
    a = p.parse_args()
    if a.child:
        return child(a, a.child)
    results = []
    for shape in a.shapes.split(","):
        cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", shape, "--runs", str(a.runs),
               "--steps", str(a.steps), "--replays", str(a.replays)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(json.dumps({"failed": shape, "returncode": r.returncode, "stderr": r.stderr[-2000:], "done": results}))
            sys.exit(1)                 # nothing more is started on the GPU
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps({"results": results}))


if __name__ == "__main__":
    main()
