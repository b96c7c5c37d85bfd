"""PCC timings on one GPU (device events around HIP-graph replays, warm-up), one JSON object per width on stdout:
  pda_pcc_adam_step_f32 (--pcc_on pos and margin) against two steps measured in the same process -- pda_adam_step_f32, the plain BPR step, and
  pda_ips_adam_step_f32 self-normalised (IPS-CN), the one other step with a batch statistic in front of its gradients -- and beside them
  pda_pcc_stats_f32 alone and a torch restatement of the step (gather, dots, centred float64 moments, autograd, pda_adam_dense_sweep2_f32; eager,
  not in a graph), on the C2 tables (50 000 x 20 000 x d), d in 64 and 128, 2 048 triplets per step with Zipf positives, the same batch for all.
The outputs are compared first: with gamma = 0 the PCC step must give the gradients and the loss of the BPR step (1e-5), and the loss and the
statistic at gamma = 1 must equal their float64 values computed by torch on the device (1e-5 max(1, 4 gamma / sqrt(Szz))); a mismatch ends the
run before anything is timed.
The steps are captured in HIP graphs of --steps launches and replayed in --runs alternating runs inside one process per width; the figures are
microseconds per step: the median over the runs and their range, and each variant's ratio to the BPR and to the IPS-CN step run by run.
Without --d the tool starts one child process per width, each under its own time limit, and starts nothing after a failure.
Usage: python tools/pcc_timing.py [--d 64] [--runs 5] [--steps 20] [--replays 400] [--limit 240]"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

WIDTHS = (64, 128)
GAMMA = 1.0


def capture(torch, fn):
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


def timed_us(torch, fn, reps, per, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * per)


def terms64(torch, U, I, users, pos, neg, pop, on, gamma, regs, B):
    """-> (float64 [3] loss, mf, reg; float64 [7] n_v, zbar, qbar, Szz, Sqq, Szq, r) on the device."""
    u, p, n = U[users.long()].double(), I[pos.long()].double(), I[neg.long()].double()
    sp, sn = (u * p).sum(1), (u * n).sum(1)
    z, q = (sp if on == "pos" else sp - sn), pop[pos.long()].double()
    dz, dq = z - z.mean(), q - q.mean()
    Szz, Sqq, Szq = (dz * dz).sum(), (dq * dq).sum(), (dz * dq).sum()
    r = Szq / torch.sqrt(Szz * Sqq)
    mf = -torch.log(torch.sigmoid(sp - sn) + 1e-10).sum() / B + gamma * r * r
    reg = regs * 0.5 * ((u ** 2).sum() + (p ** 2).sum() + (n ** 2).sum()) / B
    return torch.stack([mf + reg, mf, reg]), torch.stack([torch.tensor(float(B), dtype=torch.float64, device=U.device), z.mean(), q.mean(), Szz, Sqq, Szq, r])


def one_width(a):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pda_amd import ops

    class Tables:
        def __init__(self, U, I, B):
            z = torch.zeros_like
            self.U, self.I = U.clone(), I.clone()
            self.mU, self.vU, self.gU, self.mI, self.vI, self.gI = z(U), z(U), z(U), z(I), z(I), z(I)
            self.tagU, self.tagI = ops.adam_row_tags(U.shape[0], I.shape[0], U.device)
            self.wsum = torch.zeros(1, dtype=torch.float32, device=U.device)
            self.z_ws, self.stat = ops.pcc_workspace(B, U.device)
            self.loss, self.pcc = torch.zeros(3, device=U.device), torch.zeros(2, device=U.device)

        def state(self):
            return (self.U, self.mU, self.vU, self.gU, self.tagU, self.I, self.mI, self.vI, self.gI, self.tagI)

    if a.steps % 2:
        raise SystemExit("--steps must be even (two step tags)")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    nU, nI, d, B, regs = 50_000, 20_000, a.d, 2048, 1e-2
    out = {"shape": [nU, nI, d], "B": B, "gamma": GAMMA, "runs": a.runs, "steps_per_graph": a.steps, "replays": a.replays}

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
    counts = torch.bincount(indices.long(), minlength=nI).cpu().numpy()
    pop = ops.PccPop.from_counts(counts, "count", dev).pop
    ipw = ops.IpsWeights(indices, nI, clip=8.0).ipw

    # ---- outputs first
    one, ref = Tables(U, I, B), Tables(U, I, B)
    ops.pcc_grads(one.U, one.I, users, pos, neg, pop, one.gU, one.gI, one.tagU, one.tagI, gamma=0.0, regs=regs, reg_div=B, step=1, z_ws=one.z_ws,
                  stat=one.stat, loss_acc=one.loss)
    ops.bpr_step(ref.U, ref.I, users, pos, neg, regs=regs, reg_div=B, mode=ops.UPD_DENSE_GRAD, gU=ref.gU, gI=ref.gI, loss_acc=ref.loss)
    out["gamma_zero_max_diff"] = max(float((one.gU - ref.gU).abs().max()), float((one.gI - ref.gI).abs().max()), float((one.loss - ref.loss).abs().max()))
    ok = out["gamma_zero_max_diff"] <= 1e-5
    out["loss_err"], out["stat_rel_err"], out["r"], out["bound"] = {}, {}, {}, {}
    for on in ("pos", "margin"):
        t = Tables(U, I, B)
        ops.pcc_grads(t.U, t.I, users, pos, neg, pop, t.gU, t.gI, t.tagU, t.tagI, gamma=GAMMA, on=on, regs=regs, reg_div=B, step=1, z_ws=t.z_ws,
                      stat=t.stat, loss_acc=t.loss)
        want, st = terms64(torch, U, I, users, pos, neg, pop, on, GAMMA, regs, B)
        bound = 1e-5 * max(1.0, 4 * GAMMA / math.sqrt(float(st[3])))
        out["loss_err"][on] = float((t.loss.double() - want).abs().max())
        out["stat_rel_err"][on] = float(((t.stat[:7] - st).abs() / st.abs().clamp_min(1e-300)).max())
        out["r"][on], out["bound"][on] = float(t.stat[6]), bound
        ok = ok and out["loss_err"][on] <= bound and abs(float(t.stat[6]) - float(st[6])) <= 1e-5
    if not ok:
        out["error"] = "outputs differ: nothing timed"
        print(json.dumps(out))
        raise SystemExit(1)

    # ---- then the time
    graphs, keepalive = {}, []

    def stepper(name):
        t = Tables(U, I, B)
        keepalive.append(t)

        def run():
            for k in range(a.steps):
                kw = dict(regs=regs, reg_div=B, step=1 + (k & 1), lr_t=1e-4, loss_acc=t.loss)
                if name == "bpr":
                    ops.adam_step(*t.state(), users, pos, neg, **kw)
                elif name == "ips_cn":
                    ops.ips_adam_step(*t.state(), users, pos, neg, ipw, wsum=t.wsum, **kw)
                elif name == "stats":
                    ops.pcc_stats(t.U, t.I, users, pos, neg, pop, on="pos", z_ws=t.z_ws, stat=t.stat, check_ids=False)
                else:
                    ops.pcc_adam_step(*t.state(), users, pos, neg, pop, t.z_ws, t.stat, gamma=GAMMA, on=name[4:], pcc_acc=t.pcc, **kw)
        return run
    names = ["bpr", "ips_cn", "pcc_pos", "pcc_margin", "stats"]
    for n in names:
        graphs[n] = capture(torch, stepper(n))

    # the torch restatement: eager, one step per call
    tt = Tables(U, I, B)
    Up, Ip = tt.U.requires_grad_(True), tt.I.requires_grad_(True)
    ul, pl, nl = users.long(), pos.long(), neg.long()

    def torch_step():
        u, p, n = Up[ul], Ip[pl], Ip[nl]
        sp, sn = (u * p).sum(1), (u * n).sum(1)
        z, q = sp.double(), pop[pl].double()
        dz, dq = z - z.mean(), q - q.mean()
        r2 = (dz * dq).sum() ** 2 / ((dz * dz).sum() * (dq * dq).sum())
        loss = -torch.log(torch.sigmoid(sp - sn) + 1e-10).sum() / B + (GAMMA * r2).float() + regs * 0.5 * ((u ** 2).sum() + (p ** 2).sum() + (n ** 2).sum()) / B
        gU, gI = torch.autograd.grad(loss, (Up, Ip))
        with torch.no_grad():
            ops.adam_dense_sweep2(Up, tt.mU, tt.vU, gU.contiguous(), Ip, tt.mI, tt.vI, gI.contiguous(), 1e-4)
    times = {n: [] for n in names + ["torch"]}
    for _ in range(a.runs):
        for n in names:
            times[n].append(timed_us(torch, graphs[n].replay, a.replays, a.steps))
        times["torch"].append(timed_us(torch, torch_step, max(20, a.replays // 8), 1))
    for n in times:
        out["step_%s_us" % n] = statistics.median(times[n])
        out["step_%s_range_us" % n] = [min(times[n]), max(times[n])]
    for n in ("pcc_pos", "pcc_margin", "torch"):
        for base in ("bpr", "ips_cn"):
            r = [x / y for x, y in zip(times[n], times[base])]
            out["ratio_%s_to_%s" % (n, base)] = statistics.median(r)
            out["ratio_%s_to_%s_range" % (n, base)] = [min(r), max(r)]
    over = [x - y - s for x, y, s in zip(times["pcc_pos"], times["ips_cn"], times["stats"])]
    out["pcc_pos_minus_ips_cn_minus_stats_us"] = [min(over), statistics.median(over), max(over)]
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=0, help="one width in this process (64 | 128); 0: one child process per width")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="launches per captured graph (even)")
    ap.add_argument("--replays", type=int, default=400)
    ap.add_argument("--limit", type=int, default=240, help="seconds a width's process may take")
    a = ap.parse_args()
    if a.d:
        return one_width(a)
    for d in WIDTHS:           # (this process never opens the GPU)
        cmd = [sys.executable, os.path.abspath(__file__), "--d", str(d), "--runs", str(a.runs), "--steps", str(a.steps), "--replays", str(a.replays)]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print("d = %d ended with status %d: nothing more is started" % (d, rc), file=sys.stderr)
            raise SystemExit(rc)


if __name__ == "__main__":
    main()
