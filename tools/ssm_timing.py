"""Sampled-softmax timings on one GPU (device events around HIP-graph replays, warm-up), one JSON object on stdout:
  pda_ssm_adam_step_f32 at N in {1, 16, 64, 256} negatives per row, norm 0 and 1, against pda_adam_step_f32 (the plain BPR step) and against a torch
  restatement of the same step (gather, bmm, logsumexp, autograd into dense gradients, pda_adam_dense_sweep2_f32), on the C2 tables
  (50 000 x 20 000 x 64), 2 048 rows per step with Zipf positives and uniform negatives outside the user's history (pda_ssm_sample).
Every N runs in a child process of its own under its own time limit (--child_timeout seconds); the first child that fails ends the tool, and
nothing more is started on the GPU.  Inside a child the outputs are compared first -- the loss of both norms against its float64 value computed by
torch on the device (1e-5 max(1, 1 / tau)) and the gradients against the torch restatement's; a mismatch ends the child before anything is timed --
then the steps are captured in HIP graphs of --steps launches and replayed in --runs alternating runs; the figures are microseconds per step:
the median over the runs and their range, and each variant's ratio to the BPR step run by run.
The share of the step the negatives' float atomics take is NOT measured by switching them off (that would need a kernel variant): the table has
the step at N against the step at N = 1 instead, which bounds it from above (the difference also holds the N - 1 further gathers, dots and exps).
Usage: python tools/ssm_timing.py [--runs 5] [--steps 20] [--replays 200] [--negs 1,16,64,256]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAU, REGS = 0.1, 1e-2


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


def child(a, N):
    import torch
    from pda_amd import ops

    class Tables:
        def __init__(self, U, I):
            z = torch.zeros_like
            self.U, self.I = U.clone(), I.clone()
            self.mU, self.vU, self.gU, self.mI, self.vI, self.gI = z(U), z(U), z(U), z(I), z(I), z(I)
            self.tagU, self.tagI = ops.adam_row_tags(U.shape[0], I.shape[0], U.device)
            self.loss = torch.zeros(3, device=U.device)

        def state(self):
            return (self.U, self.mU, self.vU, self.gU, self.tagU, self.I, self.mI, self.vI, self.gI, self.tagI)

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    nU, nI, d, B = 50_000, 20_000, 64, 2048
    out = {"N": N, "shape": [nU, nI, d], "B": B, "tau": TAU}
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
    users, pos, negs = ops.ssm_sample(indptr, indices, B, N, seed=2020, step=1, n_pool=nU, neg_range=(0, nI))
    neg0 = negs[:, 0].contiguous()
    out["distinct_positives"], out["distinct_negatives"] = int(torch.unique(pos).numel()), int(torch.unique(negs).numel())
    U = torch.randn(nU, d, device=dev, generator=gen) * 0.1
    I = torch.randn(nI, d, device=dev, generator=gen) * 0.1
    ids = torch.cat([pos[:, None], negs], dim=1).long()
    ul = users.long()

    def torch_loss(Ut, It, norm, dtype):
        u, it = Ut[ul].to(dtype), It[ids].to(dtype)                       # [B, d], [B, N + 1, d]
        uq, iq = u, it
        if norm:
            uq = u / torch.linalg.vector_norm(u, dim=-1, keepdim=True).clamp_min(1e-12)
            iq = it / torch.linalg.vector_norm(it, dim=-1, keepdim=True).clamp_min(1e-12)
        s = torch.bmm(iq, uq[:, :, None])[:, :, 0] / TAU
        mf = (torch.logsumexp(s, dim=1) - s[:, 0]).sum() / B
        reg = REGS * 0.5 * ((u ** 2).sum() + (it ** 2).sum()) / B
        return mf, reg

    # ---- outputs first
    tol = 1e-5 * max(1.0, 1.0 / TAU)
    out["loss_err"], out["grad_diff_to_torch"] = {}, {}
    ok = True
    for norm in (0, 1):
        t = Tables(U, I)
        ops.ssm_step(t.U, t.I, users, pos, negs, t.gU, t.gI, t.tagU, t.tagI, tau=TAU, norm=norm, regs=REGS, reg_div=B, step=1, loss_acc=t.loss,
                     users_distinct=True)
        mf, reg = torch_loss(U, I, norm, torch.float64)
        err = float((t.loss.double() - torch.stack([mf + reg, mf, reg])).abs().max())
        Ut, It = U.clone().requires_grad_(True), I.clone().requires_grad_(True)
        mf, reg = torch_loss(Ut, It, norm, torch.float32)
        gU, gI = torch.autograd.grad(mf + reg, (Ut, It))
        diff = max(float((t.gU - gU).abs().max()), float((t.gI - gI).abs().max()))
        out["loss_err"]["norm%d" % norm], out["grad_diff_to_torch"]["norm%d" % norm] = err, diff
        ok = ok and err <= tol and diff <= 2 * tol
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
                    ops.adam_step(*t.state(), users, pos, neg0, regs=REGS, reg_div=B, step=1 + (k & 1), lr_t=1e-4, loss_acc=t.loss, users_distinct=True)
        elif name.startswith("ssm"):
            norm = int(name[-1])

            def run():
                for k in range(a.steps):
                    ops.ssm_adam_step(*t.state(), users, pos, negs, tau=TAU, norm=norm, regs=REGS, reg_div=B, step=1 + (k & 1), lr_t=1e-4,
                                      loss_acc=t.loss, users_distinct=True)
        else:
            norm = int(name[-1])
            Ut, It = t.U.requires_grad_(True), t.I.requires_grad_(True)

            def run():
                for k in range(a.torch_steps):
                    mf, reg = torch_loss(Ut, It, norm, torch.float32)
                    gU, gI = torch.autograd.grad(mf + reg, (Ut, It))
                    with torch.no_grad():
                        ops.adam_dense_sweep2(Ut.detach(), t.mU, t.vU, gU.contiguous(), It.detach(), t.mI, t.vI, gI.contiguous(), 1e-4)
        return run
    names = ["bpr", "ssm_norm0", "ssm_norm1", "torch_norm0", "torch_norm1"]
    steps_of = {n: (a.torch_steps if n.startswith("torch") else a.steps) for n in names}
    replays_of = {n: (max(5, a.replays // 10) if n.startswith("torch") else a.replays) for n in names}
    for n in names:
        graphs[n] = capture(stepper(n))
    times = {n: [] for n in names}
    for _ in range(a.runs):
        for n in names:
            times[n].append(replay_us(graphs[n], replays_of[n], steps_of[n]))
    for n in names:
        out["step_%s_us" % n] = statistics.median(times[n])
        out["step_%s_range_us" % n] = [min(times[n]), max(times[n])]
    for n in names[1:]:
        r = [x / y for x, y in zip(times[n], times["bpr"])]
        out["ratio_%s_to_bpr" % n] = statistics.median(r)
        out["ratio_%s_to_bpr_range" % n] = [min(r), max(r)]
    for norm in (0, 1):
        r = [x / y for x, y in zip(times["torch_norm%d" % norm], times["ssm_norm%d" % norm])]
        out["torch_over_ssm_norm%d" % norm] = statistics.median(r)
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="launches per captured graph (even)")
    ap.add_argument("--torch_steps", type=int, default=4, help="steps of the torch restatement per captured graph")
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--negs", type=str, default="1,16,64,256")
    ap.add_argument("--child_timeout", type=int, default=240, help="seconds one N may take")
    ap.add_argument("--child", type=int, default=0, help="(internal) measure this N in this process")
    a = ap.parse_args()
    if a.steps % 2:
        raise SystemExit("--steps must be even (two step tags)")
    if a.child:
        return child(a, a.child)
    out = {"runs": a.runs, "steps_per_graph": a.steps, "replays": a.replays, "per_N": []}
    for N in [int(x) for x in a.negs.split(",")]:
        cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", str(N), "--runs", str(a.runs), "--steps",
               str(a.steps), "--torch_steps", str(a.torch_steps), "--replays", str(a.replays)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not line:
            out["error"] = "N = %d ended with status %d: nothing more is started" % (N, r.returncode)
            out["stderr_tail"] = r.stderr[-1500:]
            if line:
                out["per_N"].append(json.loads(line[-1]))
            print(json.dumps(out))
            raise SystemExit(1)
        out["per_N"].append(json.loads(line[-1]))
    base = {p["N"]: p for p in out["per_N"]}
    if 1 in base:       # the step at N against the step at N = 1: an upper bound of what the negatives' atomics take
        for p in out["per_N"]:
            for norm in (0, 1):
                k = "step_ssm_norm%d_us" % norm
                p["share_above_N1_norm%d" % norm] = 1.0 - base[1][k] / p[k]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
