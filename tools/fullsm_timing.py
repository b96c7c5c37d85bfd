"""Full-catalogue softmax timings on one GPU (device events around HIP-graph replays, warm-up), one JSON object on stdout:
  pda_fullsm_step_f32 (the gradients alone), pda_fullsm_adam_step_f32 (with the dense sweep), pda_inbatch_adam_step_f32 (mask launch and logq
  included), pda_ssm_adam_step_f32 at N = 64 and N = 256 sampled negatives, pda_adam_step_f32 (the plain BPR step) and a torch restatement of
  the full softmax (U[users] @ I.T, masked logsumexp, autograd into dense gradients, pda_adam_dense_sweep2_f32), all with norm = 1 at tau = 0.1
  and the train mask on, B = 2 048, on the C2 tables (50 000 x 20 000 x d, d = 64 and 128) and on one larger catalogue (200 000 items, d = 128),
  with Zipf positives.  Peak device memory of the step and of the torch restatement beside the times.
The step is set against two floors computed from the shapes: its three matrix products (logits, C I^, C^T U^: 3 x 2 B n_items d FLOP; the
kernels EXECUTE five, the logits are recomputed in each gradient pass) at 155 TFLOP/s, the rate v_mfma_f32_32x32x2_f32 holds back to back on
this chip, and the bytes it has to move through HBM at 8 TB/s.
Every shape runs in a child process of its own under its own time limit (--child_timeout seconds); the first child that fails ends the tool, and
nothing more is started on the GPU.  Inside a child the outputs are compared first -- the loss against its float64 value computed by torch on
the device (1e-5 max(1, 1 / tau)) and the gradients against the torch restatement's; a mismatch ends the child before anything is timed -- then
the steps are captured in HIP graphs of --steps launches and replayed in --runs alternating runs; the figures are microseconds per step: the
median over the runs and their range.
NOT measured: the passes of the step one by one (a kernel trace would run them again, outside the graphs), a whole epoch, real data.
Usage: python tools/fullsm_timing.py [--runs 5] [--steps 10] [--replays 40] [--shapes 2048x20000x64,2048x20000x128,2048x200000x128]"""
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
MFMA_F32_FLOPS, HBM_BYTES_PER_S = 155e12, 8e12


def child(a, B, nI, d):
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
    nU = 50_000
    out = {"B": B, "d": d, "shape": [nU, nI, d], "tau": TAU, "norm": NORM, "col_splits": ops.fullsm_col_splits(nI, B)}
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
    ul, pl = users.long(), pos.long()
    n_row = (indptr[ul + 1] - indptr[ul])
    flat_r = torch.repeat_interleave(torch.arange(B, device=dev), n_row)
    flat_c = indices[(torch.arange(int(n_row.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(n_row, 0) - n_row, n_row)
                      + torch.repeat_interleave(indptr[ul], n_row))].long()
    excluded = torch.zeros((B, nI), dtype=torch.bool, device=dev)
    excluded[flat_r, flat_c] = True
    excluded[torch.arange(B, device=dev), pl] = False
    out["distinct_positives"], out["excluded_share"] = int(torch.unique(pos).numel()), float(excluded.float().mean())
    ws = ops.fullsm_workspace(B, nI, d, dev)
    out["workspace_bytes"] = ws.numel()

    def torch_loss(Ut, It, dtype):
        u, it = Ut[ul].to(dtype), It.to(dtype)
        uq = u / torch.linalg.vector_norm(u, dim=-1, keepdim=True).clamp_min(1e-12)
        iq = it / torch.linalg.vector_norm(it, dim=-1, keepdim=True).clamp_min(1e-12)
        s = torch.mm(uq, iq.T) / TAU
        mf = (torch.logsumexp(s.masked_fill(excluded, float("-inf")), dim=1) - s[torch.arange(B, device=dev), pl]).sum() / B
        reg = REGS * 0.5 * ((u ** 2).sum() + (it[pl] ** 2).sum()) / B
        return mf, reg

    # ---- outputs first
    tol = 1e-5 * max(1.0, 1.0 / TAU)
    t = Tables(U, I)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ops.fullsm_step(t.U, t.I, users, pos, t.gU, t.gI, t.tagU, t.tagI, ws, tau=TAU, norm=NORM, regs=REGS, reg_div=B, step=1, train_indptr=indptr,
                    train_indices=indices, loss_acc=t.loss, users_distinct=True)
    torch.cuda.synchronize()
    out["step_peak_extra_bytes"] = int(torch.cuda.max_memory_allocated() - base)          # (the workspace was allocated before: nothing more)
    mf, reg = torch_loss(U, I, torch.float64)
    out["loss_err"] = float((t.loss.double() - torch.stack([mf + reg, mf, reg])).abs().max())
    del mf, reg
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    Ut, It = U.clone().requires_grad_(True), I.clone().requires_grad_(True)
    mf, reg = torch_loss(Ut, It, torch.float32)
    gU, gI = torch.autograd.grad(mf + reg, (Ut, It))
    torch.cuda.synchronize()
    out["torch_peak_extra_bytes"] = int(torch.cuda.max_memory_allocated() - base)
    out["grad_diff_to_torch"] = max(float((t.gU - gU).abs().max()), float((t.gI - gI).abs().max()))
    del Ut, It, gU, gI, mf, reg
    if not (out["loss_err"] <= tol and out["grad_diff_to_torch"] <= 2 * tol):
        out["error"] = "outputs differ: nothing timed"
        print(json.dumps(out))
        raise SystemExit(1)

    # ---- then the time
    graphs, keepalive = {}, []
    logq = torch.from_numpy(ops.inbatch_logq(indptr, indices, nI)).to(dev)
    ws_in = ops.inbatch_workspace(B, d, dev)

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
        elif name == "inbatch":
            mine = torch.empty((B, ops.inbatch_mask_words(B)), dtype=torch.int32, device=dev)

            def run():
                for k in range(a.steps):
                    ops.inbatch_mask(users, pos, indptr, indices, nU, nI, out=mine)
                    ops.inbatch_adam_step(*t.state(), users, pos, ws_in, tau=TAU, norm=NORM, regs=REGS, reg_div=B, step=1 + (k & 1), lr_t=1e-4,
                                          logq=logq, mask=mine, loss_acc=t.loss, users_distinct=True)
        elif name == "fullsm":
            def run():
                for k in range(a.steps):
                    ops.fullsm_adam_step(*t.state(), users, pos, ws, tau=TAU, norm=NORM, regs=REGS, reg_div=B, step=1 + (k & 1), lr_t=1e-4,
                                         train_indptr=indptr, train_indices=indices, loss_acc=t.loss, users_distinct=True)
        elif name == "fullsm_grad_only":
            def run():
                for k in range(a.steps):
                    ops.fullsm_step(t.U, t.I, users, pos, t.gU, t.gI, t.tagU, t.tagI, ws, tau=TAU, norm=NORM, regs=REGS, reg_div=B, step=1 + (k & 1),
                                    train_indptr=indptr, train_indices=indices, loss_acc=t.loss, users_distinct=True, check_ids=False)
        else:
            Ut, It = t.U.requires_grad_(True), t.I.requires_grad_(True)

            def run():
                for k in range(a.torch_steps):
                    mf, reg = torch_loss(Ut, It, torch.float32)
                    gU, gI = torch.autograd.grad(mf + reg, (Ut, It))
                    with torch.no_grad():
                        ops.adam_dense_sweep2(Ut.detach(), t.mU, t.vU, gU.contiguous(), It.detach(), t.mI, t.vI, gI.contiguous(), 1e-4)
        return run
    names = ["bpr", "fullsm", "fullsm_grad_only", "inbatch", "ssm_64", "ssm_256", "torch"]
    steps_of = {n: (a.torch_steps if n == "torch" else a.steps) for n in names}
    for n in names:
        graphs[n] = capture(stepper(n))
    times = {n: [] for n in names}
    for _ in range(a.runs):
        for n in names:
            times[n].append(replay_us(graphs[n], a.replays, steps_of[n]))
    for n in names:
        out["step_%s_us" % n] = statistics.median(times[n])
        out["step_%s_range_us" % n] = [min(times[n]), max(times[n])]
    for n in ("bpr", "inbatch", "ssm_64", "ssm_256", "torch"):
        r = [x / y for x, y in zip(times["fullsm"], times[n])]
        out["fullsm_over_%s" % n] = statistics.median(r)
        out["fullsm_over_%s_range" % n] = [min(r), max(r)]
    # the floors, from the shapes
    prod = 2.0 * B * nI * d
    hbm = 4.0 * (3 * nI * d + 2 * nI * d + 3 * B * ((nI + 31) // 32) + 2 * B * d)      # I once per pass, gI read and written, the bits, U rows and gU
    out["flop_needed"], out["flop_executed"] = 3 * prod, 5 * prod
    out["floor_matrix_us"] = 3 * prod / MFMA_F32_FLOPS * 1e6
    out["floor_matrix_executed_us"] = 5 * prod / MFMA_F32_FLOPS * 1e6
    out["floor_hbm_us"] = hbm / HBM_BYTES_PER_S * 1e6
    out["grad_only_over_matrix_floor"] = out["step_fullsm_grad_only_us"] / out["floor_matrix_us"]
    out["grad_only_tflops_executed"] = 5 * prod / out["step_fullsm_grad_only_us"] / 1e6
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="launches per captured graph (even)")
    ap.add_argument("--torch_steps", type=int, default=2, help="steps of the torch restatement per captured graph")
    ap.add_argument("--replays", type=int, default=40)
    ap.add_argument("--shapes", type=str, default="2048x20000x64,2048x20000x128,2048x200000x128", help="B x n_items x d")
    ap.add_argument("--child_timeout", type=int, default=240, help="seconds one shape may take")
    ap.add_argument("--child", type=str, default="", help="(internal) measure this BxNxD in this process")
    a = ap.parse_args()
    if a.steps % 2:
        raise SystemExit("--steps must be even (two step tags)")
    if a.child:
        B, nI, d = (int(x) for x in a.child.split("x"))
        return child(a, B, nI, d)
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
