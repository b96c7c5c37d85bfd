"""Item-weighted iALS (--ials_item_power, include/pda_hip_ials_itemw.h) against the unweighted model on one GPU (device events, warm-up), one
JSON object on stdout, on the Douban-shaped graph of tools/ials_timing.py (47 890 users x 26 047 items, about 6.9 M distinct pairs).
Everything is measured in ONE process, --runs alternating runs, the median and the range of each; nothing is quoted across runs:
  exact epoch at d in --exact_dims, weighted and unweighted     both Gram matrices, both half-sweeps, the objective (IALSMF.train_epoch's launches)
  block epoch at (d, k) in --cases, weighted and unweighted     ops.ialspp_epoch
  the Gram matrix of the item table, scaled and plain           pda_ials_gram_scaled_f32 against pda_ials_gram_f32 / pda_ialspp_gram_f32
  the item half-sweep / item pass, alpha_row and scalar         the entry points that read one more float per solved row
The two graphs hold the same pairs; the weighted one is built with item_power = --power.  Both models start from the same tables, and the
tables are reset before every measurement, so that no run solves the result of the one before.
Every measurement runs under its own time limit (a watchdog ends the process with status 124; nothing is started after it).
Usage: python tools/ials_itemw_timing.py [--runs 5] [--reps 3] [--limit 120] [--power 0.5] [--exact_dims 64,128] [--cases 128:32,256:32]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from lightgcn_timing import limit, shaped_pairs, timed_ms  # noqa: E402
from pda_amd import ops  # noqa: E402


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def overlap(a, b):
    return not (a["min"] > b["max"] or b["min"] > a["max"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds per measurement")
    ap.add_argument("--users", type=int, default=47890)
    ap.add_argument("--items", type=int, default=26047)
    ap.add_argument("--mean_hist", type=int, default=212)
    ap.add_argument("--power", type=float, default=0.5)
    ap.add_argument("--exact_dims", type=str, default="64,128")
    ap.add_argument("--cases", type=str, default="128:32,256:32")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nU, nI = a.users, a.items
    alpha0, lam, nu = 0.1, 0.05, 1.0
    u, it = shaped_pairs(nU, nI, a.mean_hist)
    graphs = {"plain": ops.IalsGraph(u, it, nU, nI, dev, lam=lam, alpha0=alpha0, nu=nu),
              "weighted": ops.IalsGraph(u, it, nU, nI, dev, lam=lam, alpha0=alpha0, nu=nu, item_power=a.power)}
    iw = graphs["weighted"].item_weights
    cases = [tuple(int(x) for x in c.split(":")) for c in a.cases.split(",")]
    exact_dims = [int(x) for x in a.exact_dims.split(",")]
    out = {"shape": {"users": nU, "items": nI, "pairs": graphs["plain"].nnz, "alpha0": alpha0, "lambda": lam, "nu": nu, "item_power": a.power,
                     "w_min": float(iw.w.min()), "w_max": float(iw.w.max()), "w_mean": float(iw.w.mean())}}
    gen = torch.Generator(device=dev).manual_seed(2021)
    init, work = {}, {}
    for d in sorted({d for d, _ in cases} | set(exact_dims)):
        init[d] = ((torch.rand((nU, d), device=dev, generator=gen) - 0.5) * 0.2, (torch.rand((nI, d), device=dev, generator=gen) - 0.5) * 0.2)
        work[d] = tuple(torch.empty_like(t) for t in init[d])

    def fresh(d):
        X, Y = work[d]
        X.copy_(init[d][0])
        Y.copy_(init[d][1])
        return X, Y

    def exact_epoch(g, d):
        X, Y = fresh(d)
        ops.ials_half_sweep(g, "user", Y, X)
        ops.ials_half_sweep(g, "item", X, Y)
        return ops.ials_loss(g, X, Y)

    def block_epoch(g, d, k):
        X, Y = fresh(d)
        return ops.ialspp_epoch(g, X, Y, k)

    def item_sweep(g, d, G):
        X, Y = fresh(d)
        return ops.ials_half_sweep(g, "item", X, Y, G=G)

    def item_pass(g, d, k, G):
        X, Y = fresh(d)
        return ops.ialspp_block_pass(g, "item", X, Y, 0, k, G=G)

    what = {}
    for d in exact_dims:
        GX = ops.ials_gram(init[d][0])
        for tag, g in graphs.items():
            b = g.buffers(d)
            what["exact_epoch_d%d_%s" % (d, tag)] = (lambda g=g, d=d: exact_epoch(g, d))
            what["item_sweep_d%d_%s" % (d, tag)] = (lambda g=g, d=d, GX=GX: item_sweep(g, d, GX))
            what["gram_items_d%d_%s" % (d, tag)] = (lambda g=g, d=d, b=b: ops.ials_gram(init[d][1], b["G"], b["ws"],
                                                                                         g.item_weights.scale if g.item_weights is not None else None))
    for d, k in cases:
        GX = ops.ialspp_gram(init[d][0])
        for tag, g in graphs.items():
            b = ops.ialspp_buffers(g, d, k)
            ops.ialspp_predict(g, *init[d])
            what["block_epoch_d%d_k%d_%s" % (d, k, tag)] = (lambda g=g, d=d, k=k: block_epoch(g, d, k))
            what["item_pass_d%d_k%d_%s" % (d, k, tag)] = (lambda g=g, d=d, k=k, GX=GX: item_pass(g, d, k, GX))
            what["gram_items_d%d_k%d_%s" % (d, k, tag)] = (lambda g=g, d=d, b=b: ops.ialspp_gram(init[d][1], b["G"], b["gram_ws"],
                                                                                                  g.item_weights.scale if g.item_weights is not None else None))
    ms = {name: [] for name in what}
    for _ in range(a.runs):
        for name, fn in what.items():
            with limit(a.limit, name):
                ms[name].append(timed_ms(fn, a.reps))
    out["ms"] = {name: stats(v) for name, v in ms.items()}
    out["weighted_over_plain"] = {}
    for name in what:
        if name.endswith("_plain"):
            base = name[:-len("_plain")]
            p, w = out["ms"][name], out["ms"][base + "_weighted"]
            out["weighted_over_plain"][base] = {"median_ratio": w["median"] / p["median"], "ranges_overlap": overlap(p, w)}
    out["failed_pivots"] = {tag: sum(int(g.buffers(d)["fail"].item()) for d in exact_dims) + int(ops.ialspp_buffers(g, cases[0][0])["fail"].item())
                            for tag, g in graphs.items()}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
