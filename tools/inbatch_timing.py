"""In-batch softmax timings on one GPU (device events around HIP-graph replays, warm-up), one JSON object on stdout:
  pda_inbatch_adam_step_f32 with the train mask and logq (the mask launch included), the same without the mask launch (the mask built once),
  pda_ssm_adam_step_f32 at N = 64 and N = 256 sampled negatives, pda_adam_step_f32 (the plain BPR step) and a torch restatement of the in-batch
  step (gather, mm, masked logsumexp, autograd into dense gradients, pda_adam_dense_sweep2_f32), all with norm = 1 at tau = 0.1, on the C2
  tables (50 000 x 20 000 x d) with Zipf positives.  Shapes: B = 2 048 at d = 64 (with the sampled steps), B = 1 024 and 4 096 at d = 64, and
  B = 2 048 at d = 128.
Every shape runs in a child process of its own under its own time limit (--child_timeout seconds); the first child that fails ends the tool, and
nothing more is started on the GPU.  Inside a child the outputs are compared first -- the loss against its float64 value computed by torch on
the device (1e-5 max(1, 1 / tau)) and the gradients against the torch restatement's; a mismatch ends the child before anything is timed -- then
the steps are captured in HIP graphs of --steps launches and replayed in --runs alternating runs; the figures are microseconds per step: the
median over the runs and their range.
NOT measured: the passes of the step one by one (a kernel trace would run them again, outside the graphs), and the step without logq.
Usage: python tools/inbatch_timing.py [--runs 5] [--steps 20] [--replays 200] [--shapes 2048x64,1024x64,4096x64,2048x128]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.ssm_timing import capture, replay_us  # noqa: E402

TAU, REGS, NORM = 0.1, 1e-2, 1


def child(a, B, d):
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
    nU, nI = 50_000, 20_000
    with_ssm = (B, d) == (2048, 64)
    out = {"B": B, "d": d, "shape": [nU, nI, d], "tau": TAU, "norm": NORM, "col_splits": ops.inbatch_col_splits(B)}
    # a train CSR with Zipf popularity, 100 .. 200 sorted items per user (tools/ssm_timing.py): the batch's positives are popular items
    w = 1.0 / torch.arange(1, nI + 1, device=dev, dtype=torch.float32)
    L = 200
    items = torch.multinomial(w, nU * L, replacement=True, generator=gen).view(nU, L).int()
    lens = torch.randint(100, L + 1, (nU,), device=dev, generator=gen)
    keep = torch.arange(L, device=dev)[None, :] < lens[:, None]
    rows = torch.sort(torch.where(keep, items, torch.full_like(items, nI)), dim=1).values
    indices = rows[keep].contiguous()
    indptr = torch.zeros(nU + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(lens, 0)
    users, pos, negs256 = ops.ssm_sample(indptr, indices, B, 256, seed=2020, step=1, n_pool=nU, neg_range=(0, nI))
    negs = {64: negs256[:, :64].contiguous(), 256: negs256}
    neg0 = negs256[:, 0].contiguous()
    U = torch.randn(nU, d, device=dev, generator=gen) * 0.1
    I = torch.randn(nI, d, device=dev, generator=gen) * 0.1
    logq = torch.from_numpy(ops.inbatch_logq(indptr, indices, nI)).to(dev)
    mask = ops.inbatch_mask(users, pos, indptr, indices, nU, nI)
    ws = ops.inbatch_workspace(B, d, dev)
    ul, pl = users.long(), pos.long()
    bits = ((mask[:, :, None] >> torch.arange(32, device=dev, dtype=torch.int32)) & 1).reshape(B, -1)[:, :B].bool()
    eye = torch.eye(B, dtype=torch.bool, device=dev)
    excluded = (bits | (pl[:, None] == pl[None, :])) & ~eye
    out["distinct_positives"], out["excluded_share"] = int(torch.unique(pos).numel()), float(excluded.float().sum() / (B * (B - 1)))

    def torch_loss(Ut, It, dtype):
        u, it = Ut[ul].to(dtype), It[pl].to(dtype)
        uq = u / torch.linalg.vector_norm(u, dim=-1, keepdim=True).clamp_min(1e-12)
        iq = it / torch.linalg.vector_norm(it, dim=-1, keepdim=True).clamp_min(1e-12)
        s = torch.mm(uq, iq.T) / TAU - logq[pl].to(dtype)[None, :]
        mf = (torch.logsumexp(s.masked_fill(excluded, float("-inf")), dim=1) - torch.diagonal(s)).sum() / B
        reg = REGS * 0.5 * ((u ** 2).sum() + (it ** 2).sum()) / B
        return mf, reg

    # ---- outputs first
    tol = 1e-5 * max(1.0, 1.0 / TAU)
    t = Tables(U, I)
    ops.inbatch_step(t.U, t.I, users, pos, t.gU, t.gI, t.tagU, t.tagI, ws, tau=TAU, norm=NORM, regs=REGS, reg_div=B, step=1, logq=logq, mask=mask,
                     loss_acc=t.loss, users_distinct=True)
    mf, reg = torch_loss(U, I, torch.float64)
    out["loss_err"] = float((t.loss.double() - torch.stack([mf + reg, mf, reg])).abs().max())
    Ut, It = U.clone().requires_grad_(True), I.clone().requires_grad_(True)
    mf, reg = torch_loss(Ut, It, torch.float32)
    gU, gI = torch.autograd.grad(mf + reg, (Ut, It))
    out["grad_diff_to_torch"] = max(float((t.gU - gU).abs().max()), float((t.gI - gI).abs().max()))
    if not (out["loss_err"] <= tol and out["grad_diff_to_torch"] <= 2 * tol):
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
            nn = negs[int(name[4:])]

            def run():
                for k in range(a.steps):
                    ops.ssm_adam_step(*t.state(), users, pos, nn, tau=TAU, norm=NORM, regs=REGS, reg_div=B, step=1 + (k & 1), lr_t=1e-4,
                                      loss_acc=t.loss, users_distinct=True)
        elif name.startswith("inbatch"):
            mine = torch.empty_like(mask)
            mine.copy_(mask)

            def run():
                for k in range(a.steps):
                    if name == "inbatch":
                        ops.inbatch_mask(users, pos, indptr, indices, nU, nI, out=mine)
                    ops.inbatch_adam_step(*t.state(), users, pos, ws, tau=TAU, norm=NORM, regs=REGS, reg_div=B, step=1 + (k & 1), lr_t=1e-4, logq=logq,
                                          mask=mine, loss_acc=t.loss, users_distinct=True)
        else:
            Ut, It = t.U.requires_grad_(True), t.I.requires_grad_(True)

            def run():
                for k in range(a.torch_steps):
                    mf, reg = torch_loss(Ut, It, torch.float32)
                    gU, gI = torch.autograd.grad(mf + reg, (Ut, It))
                    with torch.no_grad():
                        ops.adam_dense_sweep2(Ut.detach(), t.mU, t.vU, gU.contiguous(), It.detach(), t.mI, t.vI, gI.contiguous(), 1e-4)
        return run
    names = ["bpr", "inbatch", "inbatch_mask_built_once"] + (["ssm_64", "ssm_256"] if with_ssm else []) + ["torch"]
    steps_of = {n: (a.torch_steps if n == "torch" else a.steps) for n in names}
    replays_of = {n: (max(5, a.replays // 10) if n == "torch" else a.replays) for n in names}
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
    if with_ssm:
        r = [x / y for x, y in zip(times["inbatch"], times["ssm_256"])]
        out["inbatch_over_ssm_256"] = statistics.median(r)
        out["inbatch_over_ssm_256_range"] = [min(r), max(r)]
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="launches per captured graph (even)")
    ap.add_argument("--torch_steps", type=int, default=4, help="steps of the torch restatement per captured graph")
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--shapes", type=str, default="2048x64,1024x64,4096x64,2048x128")
    ap.add_argument("--child_timeout", type=int, default=240, help="seconds one shape may take")
    ap.add_argument("--child", type=str, default="", help="(internal) measure this BxD in this process")
    a = ap.parse_args()
    if a.steps % 2:
        raise SystemExit("--steps must be even (two step tags)")
    if a.child:
        B, d = (int(x) for x in a.child.split("x"))
        return child(a, B, d)
    out = {"runs": a.runs, "steps_per_graph": a.steps, "replays": a.replays, "per_shape": []}
    for shape in a.shapes.split(","):
        cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", shape, "--runs", str(a.runs), "--steps",
               str(a.steps), "--torch_steps", str(a.torch_steps), "--replays", str(a.replays)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if line:
            out["per_shape"].append(json.loads(line[-1]))
        if r.returncode != 0 or not line:
            out["error"] = "shape %s ended with status %d: nothing more is started" % (shape, r.returncode)
            out["stderr_tail"] = r.stderr[-1500:]
            print(json.dumps(out))
            raise SystemExit(1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
