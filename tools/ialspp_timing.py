"""iALS++ timings on one GPU (device events, warm-up), one JSON object on stdout, on the Douban-shaped graph of tools/ials_timing.py
(47 890 users x 26 047 items, about 6.9 M distinct pairs).  Everything is measured in ONE process, --runs alternating runs, the median and
the range of each; nothing is quoted across runs:
  block epoch at (d, k) in --cases         ops.ialspp_epoch: predict, 2 d / k Gram calls, d / k user and item passes, the objective
  exact epoch at d in --exact_dims         ops.ials_half_sweep x 2 + both Gram matrices + ops.ials_loss (IALSMF.train_epoch's launches)
  the parts of a block epoch               predict; one Gram call of each table; one user pass and one item pass (G given); one item pass over
                                           the cut rows alone (their three phases: a work list of the rows above PDA_IALS_CHUNK pairs); the loss
  convergence                              the float64 objective (torch, on the device) after 1, 5 and 10 epochs of both solvers from the SAME
                                           initial tables: a cheaper epoch that converges more slowly shows here
Every measurement runs under its own time limit (a watchdog ends the process with status 124; nothing is started after it).
Usage: python tools/ialspp_timing.py [--runs 5] [--reps 3] [--limit 120] [--cases 64:32,128:32,128:64,256:32,256:64] [--exact_dims 64,128]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from lightgcn_timing import limit, shaped_pairs, timed_ms  # noqa: E402
from pda_amd import ops  # noqa: E402


def objective64(g, X, Y, step=1 << 20):
    """L(X, Y) in float64 on the device: the observed pairs in slices, alpha0 tr(X^T X Y^T Y), both regularisers."""
    rows = torch.repeat_interleave(torch.arange(g.n_users, device=X.device), g.user.indptr[1:] - g.user.indptr[:-1])
    cols = g.user.indices.long()
    fit = torch.zeros((), dtype=torch.float64, device=X.device)
    for a in range(0, g.nnz, step):
        s = (X[rows[a:a + step]].double() * Y[cols[a:a + step]].double()).sum(1)
        fit += ((s - 1.0) ** 2).sum()
    Xd, Yd = X.double(), Y.double()
    fit += float(np.float32(g.alpha0)) * ((Xd.t() @ Xd) * (Yd.t() @ Yd)).sum()
    reg = (g.user.lam_row.double() * Xd.square().sum(1)).sum() + (g.item.lam_row.double() * Yd.square().sum(1)).sum()
    return float(fit + reg)


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds per measurement")
    ap.add_argument("--users", type=int, default=47890)
    ap.add_argument("--items", type=int, default=26047)
    ap.add_argument("--mean_hist", type=int, default=212)
    ap.add_argument("--cases", type=str, default="64:32,128:32,128:64,256:32,256:64")
    ap.add_argument("--exact_dims", type=str, default="64,128")
    ap.add_argument("--epochs", type=str, default="1,5,10")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nU, nI = a.users, a.items
    alpha0, lam, nu = 0.1, 0.05, 1.0
    u, it = shaped_pairs(nU, nI, a.mean_hist)
    g = ops.IalsGraph(u, it, nU, nI, dev, lam=lam, alpha0=alpha0, nu=nu)
    cases = [tuple(int(x) for x in c.split(":")) for c in a.cases.split(",")]
    exact_dims = [int(x) for x in a.exact_dims.split(",")]
    marks = [int(x) for x in a.epochs.split(",")]
    long_items = g.item.host["long_rows"][:, 0]
    out = {"shape": {"users": nU, "items": nI, "pairs": g.nnz, "chunk": ops.IALS_CHUNK, "alpha0": alpha0, "lambda": lam, "nu": nu,
                     "cut_items": g.item.all_rows.n_long, "item_slots": g.item.all_rows.n_slots, "cut_users": g.user.all_rows.n_long}}
    gen = torch.Generator(device=dev).manual_seed(2021)
    init = {}
    for d in sorted({d for d, _ in cases} | set(exact_dims)):
        init[d] = ((torch.rand((nU, d), device=dev, generator=gen) - 0.5) * 0.2, (torch.rand((nI, d), device=dev, generator=gen) - 0.5) * 0.2)

    def exact_epoch(X, Y):
        ops.ials_half_sweep(g, "user", Y, X)
        ops.ials_half_sweep(g, "item", X, Y)
        return ops.ials_loss(g, X, Y)

    what, state = {}, {}
    for d in exact_dims:
        state["exact", d] = tuple(t.clone() for t in init[d])
        what["exact_epoch_d%d" % d] = (lambda d=d: exact_epoch(*state["exact", d]))
    for d, k in cases:
        X, Y = state["block", d, k] = tuple(t.clone() for t in init[d])
        what["block_epoch_d%d_k%d" % (d, k)] = (lambda X=X, Y=Y, k=k: ops.ialspp_epoch(g, X, Y, k))
        b = ops.ialspp_buffers(g, d, k)
        GY, GX = ops.ialspp_gram(Y), ops.ialspp_gram(X)
        tag = "d%d_k%d" % (d, k)
        what["predict_" + tag] = (lambda X=X, Y=Y: ops.ialspp_predict(g, X, Y))
        what["gram_items_" + tag] = (lambda Y=Y, b=b: ops.ialspp_gram(Y, b["G"], b["gram_ws"]))
        what["gram_users_" + tag] = (lambda X=X, b=b: ops.ialspp_gram(X, b["G"], b["gram_ws"]))
        what["user_pass_" + tag] = (lambda X=X, Y=Y, k=k, GY=GY: ops.ialspp_block_pass(g, "user", Y, X, 0, k, G=GY))
        what["item_pass_" + tag] = (lambda X=X, Y=Y, k=k, GX=GX: ops.ialspp_block_pass(g, "item", X, Y, 0, k, G=GX))
        if len(long_items):
            lw = g.item.sub_list(long_items)
            what["item_cut_rows_alone_" + tag] = (lambda X=X, Y=Y, k=k, GX=GX, lw=lw: ops.ialspp_block_pass(g, "item", X, Y, 0, k, G=GX, work=lw))
        what["loss_" + tag] = (lambda X=X, Y=Y, GY=GY: ops.ialspp_loss(g, X, Y, G=GY))
    ms = {name: [] for name in what}
    for _ in range(a.runs):
        for name, fn in what.items():
            with limit(a.limit, name):
                ms[name].append(timed_ms(fn, a.reps))
    out["ms"] = {name: stats(v) for name, v in ms.items()}
    sys.stderr.write("timings done\n")
    # ---- convergence from the same initial tables
    conv = {}
    runs = [("exact_d%d" % d, d, None) for d in exact_dims] + [("block_d%d_k%d" % (d, k), d, k) for d, k in cases]
    for name, d, k in runs:
        X, Y = (t.clone() for t in init[d])
        with limit(a.limit, "objective " + name):
            trail = {"0": objective64(g, X, Y)}
            for ep in range(1, max(marks) + 1):
                if k is None:
                    exact_epoch(X, Y)
                else:
                    ops.ialspp_epoch(g, X, Y, k)
                if ep in marks:
                    trail[str(ep)] = objective64(g, X, Y)
        conv[name] = trail
    out["float64_objective_after_epochs"] = conv
    out["failed_pivots"] = {"block": int(ops.ialspp_buffers(g, cases[0][0])["fail"].item()),
                            "exact": sum(int(g.buffers(d)["fail"].item()) for d in exact_dims)}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
