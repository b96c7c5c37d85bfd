"""WARP timings on one GPU (device events around HIP-graph replays, warm-up), one JSON object on stdout:
  the draw call pda_warp_sample_f32_dev at T in {16, 64, 256} in three states of the tables -- untrained (Xavier: nearly every row closes on its
  first candidate), one where no row closes (a margin of -1e30: every row scores all T), and one in between, reached by training --train_steps
  WARP steps (T = 64, margin 1, harmonic weights) from the untrained tables -- with the mean trial count and the share of rows without a
  violator of every state, against, re-measured in the same run:
    pda_sample_triplets_dev (the uniform sampler), pda_dns_sample_f32_dev at M = T (the cost of scoring everything), and a torch restatement
    (ops.ssm_sample_into, gather, bmm, compare, argmax);
  the step plus sweep pda_warp_adam_step_f32 against pda_adam_step_f32 and pda_ips_adam_step_f32;
  sampler plus step (pda_warp_sample_f32_dev + pda_warp_adam_step_f32) against the uniform pair (pda_sample_triplets_dev + pda_adam_step_f32);
on the C2 tables (50 000 x 20 000 x d, d in {64, 128}), 2 048 rows per batch, the train CSR of tools/ssm_timing.py (Zipf, 100 .. 200 items a user).
Every d runs in a child process of its own under its own time limit (--child_timeout seconds); the first child that fails ends the tool and
nothing more is started on the GPU.  Inside a child the call is first compared with the torch restatement (candidates, trial counts); a
mismatch ends the child before anything is timed.  Then every variant is captured in a HIP graph of --steps launches and replayed in --runs
alternating runs; the figures are microseconds per call: the median over the runs and their range.
Usage: python tools/warp_timing.py [--runs 5] [--steps 20] [--replays 100] [--trials 16,64,256] [--dims 64,128]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dns_timing import capture, replay_us      # noqa: E402

REGS = 1e-2
NONE_CLOSES = -1e30


def child(a, d):
    import torch
    from pda_amd import ops

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    nU, nI, B = 50_000, 20_000, 2048
    trials = [int(x) for x in a.trials.split(",")]
    out = {"d": d, "shape": [nU, nI, d], "B": B}
    w = 1.0 / torch.arange(1, nI + 1, device=dev, dtype=torch.float32)
    L = 200
    items = torch.multinomial(w, nU * L, replacement=True, generator=gen).view(nU, L).int()
    lens = torch.randint(100, L + 1, (nU,), device=dev, generator=gen)
    keep = torch.arange(L, device=dev)[None, :] < lens[:, None]
    rows = torch.sort(torch.where(keep, items, torch.full_like(items, nI)), dim=1).values
    indices = rows[keep].contiguous()
    indptr = torch.zeros(nU + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(lens, 0)
    counts = torch.bincount(indices.long(), minlength=nI).cpu().numpy()

    def xavier(n):
        bound = (6.0 / (n + d)) ** 0.5
        return (torch.rand(n, d, device=dev, generator=gen) * 2 - 1) * bound

    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)                # noqa: E731
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)              # noqa: E731
    common = dict(seed=2020, neg_range=(0, nI), n_pool=nU)
    wt = {T: ops.WarpWeights.build(nI, T, "harmonic", dev) for T in set(trials) | {64}}

    class Tables:
        def __init__(self, U, I):
            z = torch.zeros_like
            self.U, self.I = U.clone(), I.clone()
            self.mU, self.vU, self.gU, self.mI, self.vI, self.gI = z(U), z(U), z(U), z(I), z(I), z(I)
            self.tagU, self.tagI = ops.adam_row_tags(nU, nI, dev)
            self.loss = torch.zeros(3, device=dev)

        def state(self):
            return (self.U, self.mU, self.vU, self.gU, self.tagU, self.I, self.mI, self.vI, self.gI, self.tagI)

    U0, I0 = xavier(nU), xavier(nI)
    # ---- the state in between: --train_steps WARP steps from the untrained tables
    tr = Tables(U0, I0)
    for t in range(1, a.train_steps + 1):
        u, p, n, coef = ops.warp_sample(tr.U, tr.I, indptr, indices, B, max_trials=64, margin=1.0, wtab=wt[64].wtab, step=t, **common)[:4]
        ops.warp_adam_step(*tr.state(), u, p, n, coef, margin=1.0, regs=REGS, reg_div=B, step=t, lr_t=ops.adam_lr_t(a.train_lr, t), users_distinct=True)
    torch.cuda.synchronize()
    states = {"untrained": (U0, I0, 1.0), "trained": (tr.U, tr.I, 1.0), "none_closes": (U0, I0, NONE_CLOSES)}

    # ---- outputs first: the candidates are pda_ssm_sample's, the trial count is the torch restatement's (rows it decides by more than 1e-4)
    def torch_first(users, pos, negs, Ut, It, margin):
        ue = Ut[users.long()]
        s = torch.bmm(It[negs.long()], ue[:, :, None])[:, :, 0]                    # [B, T]
        x = (ue * It[pos.long()]).sum(1, keepdim=True) - s
        viol = (margin - x) > 0
        return torch.where(viol.any(1), viol.int().argmax(1) + 1, torch.zeros_like(viol[:, 0], dtype=torch.long)), margin - x

    out["states"] = {}
    for name, (Ut, It, margin) in states.items():
        for T in trials:
            stat = torch.zeros(2, dtype=torch.int64, device=dev)
            u, p, n, coef, tri, _, _, cand, score, ps = ops.warp_sample(Ut, It, indptr, indices, B, max_trials=T, margin=margin, wtab=wt[T].wtab, step=1,
                                                                        want_cands=True, stat=stat, **common)
            us, pp, negs = ops.ssm_sample(indptr, indices, B, T, seed=2020, step=1, n_pool=nU, neg_range=(0, nI))
            N, h = torch_first(us, pp, negs, Ut, It, margin)
            sure = (h.abs() > 1e-4).all(1)
            ok = torch.equal(u, us) and torch.equal(p, pp) and torch.equal(tri.long()[sure], N[sure]) and bool(sure.float().mean() > 0.9)
            kept = cand >= 0
            ok = ok and torch.equal(cand[kept], negs[kept])
            if not ok:
                out["error"] = "outputs differ in state %s at T = %d: nothing timed" % (name, T)
                print(json.dumps(out))
                raise SystemExit(1)
            total, none = stat.tolist()
            out["states"]["%s_T%d" % (name, T)] = {"mean_trials": total / max(B - none, 1), "share_none": none / B}

    # ---- then the time
    graphs, keepalive = {}, []

    def counter():
        c = torch.tensor([1, 0], dtype=torch.int64, device=dev)
        keepalive.append(c)
        return c

    def uniform_call():
        ctr, bufs = counter(), (i32(B), i32(B), i32(B), None, None)

        def run(k):
            ops.sample_triplets_into(bufs, indptr, indices, seed=2020, step_dev=ctr, parity=k & 1, n_pool=nU, neg_range=(0, nI))
        return run, bufs

    def dns_call(M, Ut, It):
        ctr, bufs = counter(), (i32(B), i32(B), i32(B), None, None)

        def run(k):
            ops.dns_sample_into(bufs, Ut, It, indptr, indices, n_cands=M, topn=1, head=ops.HEAD_RAW, step_dev=ctr, parity=k & 1, **common)
        return run, bufs

    def warp_call(T, margin, tables):
        ctr, bufs = counter(), (i32(B), i32(B), i32(B), f32(B), i32(B), None, None)

        def run(k):
            Ut, It = tables()
            ops.warp_sample_into(bufs, Ut, It, indptr, indices, max_trials=T, margin=margin, wtab=wt[T].wtab, step_dev=ctr, parity=k & 1, **common)
        return run, bufs

    def torch_call(T, Ut, It, margin):
        ctr, bufs = counter(), (i32(B), i32(B), i32(B, T))

        def run(k):
            ops.ssm_sample_into(bufs, indptr, indices, seed=2020, step_dev=ctr, neg_range=(0, nI), parity=k & 1, n_pool=nU)
            N, _ = torch_first(bufs[0], bufs[1], bufs[2], Ut, It, margin)
            torch.gather(bufs[2], 1, (N - 1).clamp_min(0)[:, None])
        return run, bufs

    ipw = ops.IpsWeights.from_counts(counts, 0.0, dev).ipw

    def with_step(make, kind):
        t = Tables(U0, I0)
        keepalive.append(t)
        call, bufs = make(lambda: (t.U, t.I))

        def run(k):
            call(k)
            kw = dict(regs=REGS, reg_div=B, step=1 + (k & 1), lr_t=1e-4, loss_acc=t.loss, users_distinct=True)
            if kind == "warp":
                ops.warp_adam_step(*t.state(), bufs[0], bufs[1], bufs[2], bufs[3], margin=1.0, **kw)
            elif kind == "ips":
                ops.ips_adam_step(*t.state(), bufs[0], bufs[1], bufs[2], ipw, **kw)
            else:
                ops.adam_step(*t.state(), bufs[0], bufs[1], bufs[2], **kw)
        return run

    def step_only(kind):
        """The step plus sweep on one fixed batch (drawn once by the WARP call on the untrained tables, T = 64)."""
        bufs = tuple(t.clone() for t in ops.warp_sample(U0, I0, indptr, indices, B, max_trials=64, margin=1.0, wtab=wt[64].wtab, step=1, **common)[:4])
        return with_step(lambda tables: ((lambda k: None), bufs), kind)

    def loop(run, steps):
        def fn():
            for k in range(steps):
                run(k)
        return fn

    names = {"uniform": uniform_call()[0]}
    for T in trials:
        for name, (Ut, It, margin) in states.items():
            names["warp_%s_T%d" % (name, T)] = warp_call(T, margin, lambda Ut=Ut, It=It: (Ut, It))[0]
        names["dns_M%d" % T] = dns_call(T, U0, I0)[0]
        names["torch_untrained_T%d" % T] = torch_call(T, U0, I0, 1.0)[0]
    for kind in ("bpr", "ips", "warp"):
        names["step+sweep_%s" % kind] = step_only(kind)
    names["uniform+adam"] = with_step(lambda tables: uniform_call(), "bpr")
    for T in a.pair_trials:
        names["warp_T%d+warp_adam" % T] = with_step(lambda tables, T=T: warp_call(T, 1.0, tables), "warp")
    steps_of = {n: (a.torch_steps if n.startswith("torch") else a.steps) for n in names}
    replays_of = {n: (max(5, a.replays // 5) if n.startswith("torch") else a.replays) for n in names}
    for n, run in names.items():
        graphs[n] = capture(loop(run, steps_of[n]))
    times = {n: [] for n in names}
    for _ in range(a.runs):
        for n in names:
            times[n].append(replay_us(graphs[n], replays_of[n], steps_of[n]))
    med = {n: statistics.median(t) for n, t in times.items()}
    out["us"] = {n: {"median": med[n], "range": [min(t), max(t)]} for n, t in times.items()}
    out["ratios"] = {}
    for T in trials:
        out["ratios"]["T%d" % T] = {"untrained_over_dns": med["warp_untrained_T%d" % T] / med["dns_M%d" % T],
                                    "untrained_over_uniform": med["warp_untrained_T%d" % T] / med["uniform"],
                                    "trained_over_dns": med["warp_trained_T%d" % T] / med["dns_M%d" % T],
                                    "none_closes_over_dns": med["warp_none_closes_T%d" % T] / med["dns_M%d" % T],
                                    "untrained_over_torch": med["warp_untrained_T%d" % T] / med["torch_untrained_T%d" % T]}
    out["ratios"]["step+sweep_warp_over_bpr"] = med["step+sweep_warp"] / med["step+sweep_bpr"]
    out["ratios"]["step+sweep_warp_over_ips"] = med["step+sweep_warp"] / med["step+sweep_ips"]
    for T in a.pair_trials:
        out["ratios"]["pair_T%d_over_uniform_pair" % T] = med["warp_T%d+warp_adam" % T] / med["uniform+adam"]
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="launches per captured graph (even: the two-slot step counter)")
    ap.add_argument("--torch_steps", type=int, default=4, help="calls of the torch restatement per captured graph (even)")
    ap.add_argument("--replays", type=int, default=100)
    ap.add_argument("--trials", type=str, default="16,64,256")
    ap.add_argument("--pairs", type=str, default="64", help="T of the sampler + step pairs")
    ap.add_argument("--dims", type=str, default="64,128")
    ap.add_argument("--train_steps", type=int, default=300, help="WARP steps that lead to the state in between")
    ap.add_argument("--train_lr", type=float, default=1e-2)
    ap.add_argument("--child_timeout", type=int, default=240, help="seconds one d may take")
    ap.add_argument("--child", type=int, default=0, help="(internal) measure this d in this process")
    a = ap.parse_args()
    if a.steps % 2 or a.torch_steps % 2:
        raise SystemExit("--steps and --torch_steps must be even (the two-slot step counter, two step tags)")
    a.pair_trials = [int(x) for x in a.pairs.split(",") if x]
    if a.child:
        return child(a, a.child)
    out = {"runs": a.runs, "steps_per_graph": a.steps, "replays": a.replays, "train_steps": a.train_steps, "per_d": []}
    for d in [int(x) for x in a.dims.split(",")]:
        cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", str(d), "--runs", str(a.runs), "--steps",
               str(a.steps), "--torch_steps", str(a.torch_steps), "--replays", str(a.replays), "--trials", a.trials, "--pairs", a.pairs,
               "--train_steps", str(a.train_steps), "--train_lr", str(a.train_lr)]
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
