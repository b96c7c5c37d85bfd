"""DirectAU timings on one GPU (device events around HIP-graph replays, warm-up), one JSON object per (width, batch size) on stdout:
  pda_dau_adam_step_f32 against three steps measured in the same process -- pda_inbatch_adam_step_f32 (norm 1, logQ on, the train mask built
  once and NOT rebuilt per step), pda_adam_step_f32 (the plain BPR step) and a torch restatement (F.normalize, the two Gram products, exp,
  autograd, pda_adam_dense_sweep2_f32; eager, not in a graph) -- and beside them pda_dau_step_f32 alone (the four launches without the sweep), on
  the C2 tables (50 000 x 20 000 x d), d in 64 and 128, B in 1 024, 2 048 and 4 096 rows per step with Zipf positives, the same batch for all.
The outputs are compared first: the loss terms of the DirectAU step must equal their float64 values computed by torch on the device within
1e-5 max(1, 2 t gamma); a mismatch ends the run before anything is timed.
The steps are captured in HIP graphs of --steps launches and replayed in --runs alternating runs inside one process per width; the figures are
microseconds per step: the median over the runs and their range, and each variant's ratio to the DirectAU step run by run.
Without --d the tool starts one child process per width, each under its own time limit, and starts nothing after a failure.
The kernels of the step one by one (the tile pass alone, the share of the pack and the tail) come from a kernel trace taken in a run of its
own: `--trace` runs --replays eager DirectAU steps at one (d, B) and nothing else, for
    rocprofv3 --kernel-trace --output-format csv -d OUT -o dau -- python tools/dau_timing.py --trace --d 64 --B 2048
and `--summarise OUT/.../dau_kernel_trace.csv` prints the mean and median duration per kernel name of such a trace.
Usage: python tools/dau_timing.py [--d 64] [--B 2048] [--runs 5] [--steps 20] [--replays 200] [--limit 400]"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys

WIDTHS = (64, 128)
BATCHES = (1024, 2048, 4096)
T_, GAMMA, SAME, TAU = 2.0, 1.0, "keep", 0.1


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


def uniformity(torch, x, ids=None):
    """log of the mean of exp(-t |x_a - x_b|^2) over the pairs a < b of the unit rows x (same = keep), from the Gram product."""
    B = x.shape[0]
    d2 = (2.0 - 2.0 * (x @ x.T)).clamp_min(0.0)
    e = torch.exp(-T_ * d2)
    if ids is not None:                     # rows with the same id are the same row: distance 0
        e = torch.where(ids[:, None] == ids[None, :], torch.ones_like(e), e)
    return torch.log((e.sum() - torch.diagonal(e).sum()) / (B * (B - 1)))


def terms64(torch, U, I, users, pos, regs, B):
    """-> float64 [3] loss, mf, reg and float64 [3] align, uni_U, uni_I on the device."""
    F = torch.nn.functional
    u, p = U[users.long()].double(), I[pos.long()].double()
    uq, pq = F.normalize(u, dim=1, eps=1e-12), F.normalize(p, dim=1, eps=1e-12)
    align = ((uq - pq) ** 2).sum() / B
    uu, ui = uniformity(torch, uq, users), uniformity(torch, pq, pos)
    mf = align + GAMMA * (uu + ui) / 2
    reg = regs * 0.5 * ((u ** 2).sum() + (p ** 2).sum()) / B
    return torch.stack([mf + reg, mf, reg]), torch.stack([align, uu, ui])


def setup(a):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pda_amd import ops
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    nU, nI, d = 50_000, 20_000, a.d
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
    U = torch.randn(nU, d, device=dev, generator=gen) * 0.1
    I = torch.randn(nI, d, device=dev, generator=gen) * 0.1
    return torch, ops, dev, nU, nI, indptr, indices, U, I


class Tables:
    def __init__(self, torch, ops, U, I):
        z = torch.zeros_like
        self.U, self.I = U.clone(), I.clone()
        self.mU, self.vU, self.gU, self.mI, self.vI, self.gI = z(U), z(U), z(U), z(I), z(I), z(I)
        self.tagU, self.tagI = ops.adam_row_tags(U.shape[0], I.shape[0], U.device)
        self.loss, self.stat = torch.zeros(3, device=U.device), torch.zeros(4, device=U.device)

    def state(self):
        return (self.U, self.mU, self.vU, self.gU, self.tagU, self.I, self.mI, self.vI, self.gI, self.tagI)


def one_width(a):
    torch, ops, dev, nU, nI, indptr, indices, U, I = setup(a)
    if a.steps % 2:
        raise SystemExit("--steps must be even (two step tags)")
    regs, d = 1e-2, a.d
    logq = torch.from_numpy(ops.inbatch_logq(indptr, indices, nI)).to(dev)
    for B in ([a.B] if a.B else BATCHES):
        out = {"shape": [nU, nI, d], "B": B, "t": T_, "gamma": GAMMA, "same": SAME, "runs": a.runs, "steps_per_graph": a.steps, "replays": a.replays,
               "col_splits": ops.dau_col_splits(B), "inbatch_col_splits": ops.inbatch_col_splits(B)}
        users, pos, neg = ops.sample_triplets(indptr, indices, B, seed=2020, step=1, n_pool=nU, neg_range=(0, nI))[:3]
        out["distinct_positives"] = int(torch.unique(pos).numel())
        mask = ops.inbatch_mask(users, pos, indptr, indices, nU, nI)

        # ---- outputs first
        one = Tables(torch, ops, U, I)
        ws = ops.dau_workspace(B, d, dev)
        ops.dau_step(one.U, one.I, users, pos, one.gU, one.gI, one.tagU, one.tagI, ws, t=T_, gamma=GAMMA, same=SAME, regs=regs, reg_div=B, step=1,
                     stat=one.stat, loss_acc=one.loss)
        want, wstat = terms64(torch, U, I, users, pos, regs, B)
        bound = 1e-5 * max(1.0, 2 * T_ * GAMMA)
        out["loss_err"] = float((one.loss.double() - want).abs().max())
        out["stat_err"] = float((one.stat[:3].double() - wstat).abs().max())
        out["stat"], out["bound"] = [float(x) for x in one.stat[:3]], bound
        if not (out["loss_err"] <= bound and out["stat_err"] <= bound):
            out["error"] = "outputs differ: nothing timed"
            print(json.dumps(out))
            raise SystemExit(1)

        # ---- then the time
        graphs, keepalive = {}, []

        def stepper(name):
            t = Tables(torch, ops, U, I)
            wsd, wsi = ops.dau_workspace(B, d, dev), ops.inbatch_workspace(B, d, dev)
            keepalive.append((t, wsd, wsi))

            def run():
                for k in range(a.steps):
                    kw = dict(regs=regs, reg_div=B, step=1 + (k & 1), loss_acc=t.loss)
                    if name == "bpr":
                        ops.adam_step(*t.state(), users, pos, neg, lr_t=1e-4, **kw)
                    elif name == "inbatch":
                        ops.inbatch_adam_step(*t.state(), users, pos, wsi, tau=TAU, norm=1, lr_t=1e-4, logq=logq, mask=mask, **kw)
                    elif name == "dau":
                        ops.dau_adam_step(*t.state(), users, pos, wsd, t=T_, gamma=GAMMA, same=SAME, lr_t=1e-4, stat=t.stat, **kw)
                    else:               # the four launches of the step without the sweep (gU / gI keep accumulating: the time does not care)
                        ops.dau_step(t.U, t.I, users, pos, t.gU, t.gI, t.tagU, t.tagI, wsd, t=T_, gamma=GAMMA, same=SAME, stat=t.stat, check_ids=False,
                                     **kw)
            return run
        names = ["bpr", "inbatch", "dau", "dau_grads"]
        for n in names:
            graphs[n] = capture(torch, stepper(n))

        # the torch restatement: eager, one step per call
        tt = Tables(torch, ops, U, I)
        Up, Ip = tt.U.requires_grad_(True), tt.I.requires_grad_(True)
        ul, pl = users.long(), pos.long()
        F = torch.nn.functional

        def torch_step():
            u, p = Up[ul], Ip[pl]
            uq, pq = F.normalize(u, dim=1, eps=1e-12), F.normalize(p, dim=1, eps=1e-12)
            loss = ((uq - pq) ** 2).sum() / B + GAMMA * (uniformity(torch, uq) + uniformity(torch, pq)) / 2 + regs * 0.5 * ((u ** 2).sum() + (p ** 2).sum()) / B
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
        for n in ("bpr", "inbatch", "torch", "dau_grads"):
            r = [x / y for x, y in zip(times[n], times["dau"])]
            out["ratio_%s_to_dau" % n] = statistics.median(r)
            out["ratio_%s_to_dau_range" % n] = [min(r), max(r)]
        # the matrix work of the tile pass: two sides, B^2 pairs, d multiply-adds for the dots and d for E X: 8 B^2 d flop
        out["tile_pass_gflop"] = 8.0 * B * B * d / 1e9
        out["measured_on"] = torch.cuda.get_device_name(0)
        print(json.dumps(out), flush=True)
        del graphs, keepalive


def trace(a):
    """--replays eager DirectAU steps at one (d, B), and nothing else: the program of a kernel trace."""
    torch, ops, dev, nU, nI, indptr, indices, U, I = setup(a)
    B = a.B or 2048
    users, pos = ops.sample_triplets(indptr, indices, B, seed=2020, step=1, n_pool=nU, neg_range=(0, nI))[:2]
    t = Tables(torch, ops, U, I)
    ws = ops.dau_workspace(B, a.d, dev)
    for k in range(a.replays):
        ops.dau_adam_step(*t.state(), users, pos, ws, t=T_, gamma=GAMMA, same=SAME, regs=1e-2, reg_div=B, step=1 + (k & 1), lr_t=1e-4, stat=t.stat,
                          loss_acc=t.loss)
    torch.cuda.synchronize()
    print(json.dumps({"traced_steps": a.replays, "d": a.d, "B": B, "loss_sum": [float(x) for x in t.loss]}))


def summarise(path):
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name in sorted(rows, key=lambda n: -sum(rows[n])):
        v = rows[name]
        print("%-90s n=%5d  mean %8.2f us  median %8.2f us  total %10.1f us" % (name[:90], len(v), statistics.mean(v), statistics.median(v), sum(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=0, help="one width in this process (64 | 128); 0: one child process per width")
    ap.add_argument("--B", type=int, default=0, help="one batch size; 0: 1 024, 2 048 and 4 096")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="launches per captured graph (even)")
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--limit", type=int, default=400, help="seconds a width's process may take")
    ap.add_argument("--trace", action="store_true", help="run --replays eager DirectAU steps at (--d, --B) and nothing else")
    ap.add_argument("--summarise", default="", help="a kernel trace CSV: print the duration per kernel name")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    if a.trace:
        if not a.d:
            raise SystemExit("--trace needs --d")
        return trace(a)
    if a.d:
        return one_width(a)
    for d in WIDTHS:           # (this process never opens the GPU)
        cmd = [sys.executable, os.path.abspath(__file__), "--d", str(d), "--B", str(a.B), "--runs", str(a.runs), "--steps", str(a.steps), "--replays",
               str(a.replays)]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print("d = %d ended with status %d: nothing more is started" % (d, rc), file=sys.stderr)
            raise SystemExit(rc)


if __name__ == "__main__":
    main()
