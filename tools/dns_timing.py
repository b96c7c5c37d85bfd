"""Dynamic hard-negative sampling timings on one GPU (device events around HIP-graph replays, warm-up), one JSON object on stdout:
  the sampler call pda_dns_sample_f32_dev at M in {1, 8, 16, 32, 128, 256} candidates per row, both heads, against pda_sample_triplets_dev;
  sampler + BPR Adam step (pda_dns_sample_f32_dev + pda_adam_step_f32) against the uniform pair (pda_sample_triplets_dev + pda_adam_step_f32);
  a torch restatement of the call's work (ops.ssm_sample_into, gather, bmm, topk, gather);
  the byte floor of the call: B M d 4 bytes of item rows, once, at GATHER_TBPS (uniformly random rows of a table that sits in the Infinity
  Cache), and the fraction of it the call reaches;
on the C2 tables (50 000 x 20 000 x d, d in {64, 128}), 2 048 rows per batch, the train CSR of tools/ssm_timing.py (Zipf, 100 .. 200 items a user).
Every d runs in a child process of its own under its own time limit (--child_timeout seconds); the first child that fails ends the tool and
nothing more is started on the GPU.  Inside a child the call is first compared with the torch restatement (the candidates bit for bit, the
picked score against torch's maximum); a mismatch ends the child before anything is timed.  Then every variant is captured in a HIP graph of
--steps launches and replayed in --runs alternating runs; the figures are microseconds per call: the median over the runs and their range.
Usage: python tools/dns_timing.py [--runs 5] [--steps 20] [--replays 100] [--cands 1,8,16,32,128,256] [--dims 64,128]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REGS = 1e-2
GATHER_TBPS = 8.6       # uniformly random whole rows served from the Infinity Cache, chip-wide (a 38 MB table; the C2 item table is 5 .. 10 MB)
N_SLOTS = 10


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


def replay_us(g, replays, steps, warm=3):
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
    return e0.elapsed_time(e1) * 1e3 / (replays * steps)


def child(a, d):
    import torch
    from pda_amd import ops

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    nU, nI, B = 50_000, 20_000, 2048
    cands = [int(x) for x in a.cands.split(",")]
    out = {"d": d, "shape": [nU, nI, d], "B": B, "gather_TBps": GATHER_TBPS}
    w = 1.0 / torch.arange(1, nI + 1, device=dev, dtype=torch.float32)
    L = 200
    items = torch.multinomial(w, nU * L, replacement=True, generator=gen).view(nU, L).int()
    lens = torch.randint(100, L + 1, (nU,), device=dev, generator=gen)
    keep = torch.arange(L, device=dev)[None, :] < lens[:, None]
    rows = torch.sort(torch.where(keep, items, torch.full_like(items, nI)), dim=1).values
    indices = rows[keep].contiguous()
    indptr = torch.zeros(nU + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(lens, 0)
    slots = torch.randint(0, N_SLOTS, (indices.numel(),), device=dev, generator=gen).int()
    pop = (torch.rand(nI, N_SLOTS, device=dev, generator=gen) * 0.95 + 0.05) ** 0.22
    U = torch.randn(nU, d, device=dev, generator=gen) * 0.1
    I = torch.randn(nI, d, device=dev, generator=gen) * 0.1
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)                # noqa: E731
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)              # noqa: E731
    common = dict(seed=2020, neg_range=(0, nI), n_pool=nU)

    def torch_pick(users, negs):
        s = torch.bmm(I[negs.long()], U[users.long()][:, :, None])[:, :, 0]      # [B, M]
        top = torch.topk(s, 1, dim=1)
        return torch.gather(negs, 1, top.indices), top.values

    # ---- outputs first: the candidates are pda_ssm_sample's, the pick's score is the row's maximum
    for M in (cands[0], cands[-1]):
        u, p, n, _, _, cand, score, col = ops.dns_sample(U, I, indptr, indices, B, n_cands=M, topn=1, step=1, want_cands=True, **common)
        us, ps, negs = ops.ssm_sample(indptr, indices, B, M, seed=2020, step=1, n_pool=nU, neg_range=(0, nI))
        tn, tv = torch_pick(us, negs)
        picked = score.gather(1, col.long()[:, None])
        ok = torch.equal(cand, negs) and torch.equal(u, us) and torch.equal(p, ps) and bool((picked >= score).all()) and \
            float((picked - tv).abs().max()) <= 1e-5
        if not ok:
            out["error"] = "outputs differ at M = %d: nothing timed" % M
            print(json.dumps(out))
            raise SystemExit(1)

    # ---- then the time
    graphs, keepalive = {}, []

    def counter():
        c = torch.tensor([1, 0], dtype=torch.int64, device=dev)
        keepalive.append(c)
        return c

    def uniform_call(with_pop):
        ctr, bufs = counter(), (i32(B), i32(B), i32(B), f32(B) if with_pop else None, f32(B) if with_pop else None)

        def run(k):
            ops.sample_triplets_into(bufs, indptr, indices, seed=2020, step_dev=ctr, parity=k & 1, n_pool=nU, neg_range=(0, nI),
                                     train_slots=slots if with_pop else None, pop_matrix=pop if with_pop else None)
        return run, bufs

    def dns_call(M, head, tables=None):
        with_pop = head == ops.HEAD_POP
        ctr, bufs = counter(), (i32(B), i32(B), i32(B), f32(B) if with_pop else None, f32(B) if with_pop else None)

        def run(k):
            Ut, It = tables() if tables else (U, I)
            ops.dns_sample_into(bufs, Ut, It, indptr, indices, n_cands=M, topn=1, head=head, step_dev=ctr, parity=k & 1,
                                train_slots=slots if with_pop else None, pop_matrix=pop if with_pop else None, **common)
        return run, bufs

    def torch_call(M):
        ctr, bufs = counter(), (i32(B), i32(B), i32(B, M))

        def run(k):
            ops.ssm_sample_into(bufs, indptr, indices, seed=2020, step_dev=ctr, neg_range=(0, nI), parity=k & 1, n_pool=nU)
            torch_pick(bufs[0], bufs[2])
        return run, bufs

    class Tables:
        def __init__(self):
            z = torch.zeros_like
            self.U, self.I = U.clone(), I.clone()
            self.mU, self.vU, self.gU, self.mI, self.vI, self.gI = z(U), z(U), z(U), z(I), z(I), z(I)
            self.tagU, self.tagI = ops.adam_row_tags(nU, nI, dev)
            self.loss = torch.zeros(3, device=dev)

        def state(self):
            return (self.U, self.mU, self.vU, self.gU, self.tagU, self.I, self.mI, self.vI, self.gI, self.tagI)

    def with_step(make):
        t = Tables()
        keepalive.append(t)
        call, bufs = make(lambda: (t.U, t.I))

        def run(k):
            call(k)
            ops.adam_step(*t.state(), bufs[0], bufs[1], bufs[2], regs=REGS, reg_div=B, step=1 + (k & 1), lr_t=1e-4, loss_acc=t.loss, users_distinct=True)
        return run

    def loop(run, steps):
        def fn():
            for k in range(steps):
                run(k)
        return fn

    names = {"uniform": uniform_call(False)[0], "uniform_pop": uniform_call(True)[0]}
    for M in cands:
        names["dns_raw_M%d" % M] = dns_call(M, ops.HEAD_RAW)[0]
        names["dns_pop_M%d" % M] = dns_call(M, ops.HEAD_POP)[0]
        names["torch_M%d" % M] = torch_call(M)[0]
    names["uniform+adam"] = with_step(lambda tables: uniform_call(False))
    for M in a.pair_cands:
        names["dns_raw_M%d+adam" % M] = with_step(lambda tables, M=M: dns_call(M, ops.HEAD_RAW, tables))
    steps_of = {n: (a.torch_steps if n.startswith("torch") else a.steps) for n in names}
    replays_of = {n: (max(5, a.replays // 5) if n.startswith("torch") else a.replays) for n in names}
    for n, run in names.items():
        graphs[n] = capture(loop(run, steps_of[n]))
    times = {n: [] for n in names}
    for _ in range(a.runs):
        for n in names:
            times[n].append(replay_us(graphs[n], replays_of[n], steps_of[n]))
    out["us"] = {n: {"median": statistics.median(t), "range": [min(t), max(t)]} for n, t in times.items()}
    out["floor"] = {}
    for M in cands:
        floor = B * M * d * 4 / (GATHER_TBPS * 1e12) * 1e6
        out["floor"]["M%d" % M] = {"floor_us": floor, "fraction_reached_raw": floor / statistics.median(times["dns_raw_M%d" % M]),
                                   "call_minus_uniform_us": statistics.median(times["dns_raw_M%d" % M]) - statistics.median(times["uniform"])}
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="launches per captured graph (even: the two-slot step counter)")
    ap.add_argument("--torch_steps", type=int, default=4, help="calls of the torch restatement per captured graph (even)")
    ap.add_argument("--replays", type=int, default=100)
    ap.add_argument("--cands", type=str, default="1,8,16,32,128,256")
    ap.add_argument("--pairs", type=str, default="16,32", help="M of the sampler + Adam step pairs")
    ap.add_argument("--dims", type=str, default="64,128")
    ap.add_argument("--child_timeout", type=int, default=240, help="seconds one d may take")
    ap.add_argument("--child", type=int, default=0, help="(internal) measure this d in this process")
    a = ap.parse_args()
    if a.steps % 2 or a.torch_steps % 2:
        raise SystemExit("--steps and --torch_steps must be even (the two-slot step counter, two step tags)")
    a.pair_cands = [int(x) for x in a.pairs.split(",") if x]
    if a.child:
        return child(a, a.child)
    out = {"runs": a.runs, "steps_per_graph": a.steps, "replays": a.replays, "per_d": []}
    for d in [int(x) for x in a.dims.split(",")]:
        cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", str(d), "--runs", str(a.runs), "--steps",
               str(a.steps), "--torch_steps", str(a.torch_steps), "--replays", str(a.replays), "--cands", a.cands, "--pairs", a.pairs]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if line:
            out["per_d"].append(json.loads(line[-1]))
        if r.returncode != 0 or not line:
            out["error"] = "d = %d ended with status %d: nothing more is started" % (d, r.returncode)
            out["stderr_tail"] = r.stderr[-1500:]
            print(json.dumps(out))
            raise SystemExit(1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
