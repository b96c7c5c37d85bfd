"""Item exposure of the lists (pda_list_exposure, include/pda_hip_exposure.h), timings on one GPU: device events, a warm-up of every variant,
five alternating runs in one process, one JSON object on stdout.

Shape: one evaluation block, 262 144 lists x 50 columns over 200 000 items, Ks = [20, 50], ten targets per row (three of them from the row's own
list, so that there are hits).  Two list distributions:
  pda      the lists ops.recommend_topk ranks with the popularity head on the synthetic `c3` workload (Zipf popularity: concentrated)
  uniform  distinct ids per row, id = (a_r + j b_r) mod n_items with a_r, b_r uniform: no reuse inside a workgroup's slab, the LDS table's worst case
Variants, per distribution:
  exposure / exposure_no_targets   ops.list_exposure (the LDS table) with and without the hit counts
  plain / plain_no_targets         pda_list_exposure_plain: one global atomic per entry
  torch / torch_no_targets         the restatement a user has without the kernel: a bincount per bucket, a broadcast membership test for the hits
  read_lists                       one reduction over the lists (reads them once)
and, on `pda`, the block around it: recommend_topk (the call that produces the lists) and metrics_sums.  The outputs of the three routes are
compared before anything is timed.
Usage: python tools/exposure_timing.py [--runs 5] [--rows 262144]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pda_amd import ops, synthetic  # noqa: E402

N_ITEMS, K_COLS, KS, N_TGT = 200000, 50, [20, 50], 10


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(runs, fns):
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(runs):
        for k, f in fns.items():
            t[k].append(once(f))
    return t


def torch_route(topk, n_items, tgt=None):
    """The contract in torch for target rows of one length (tgt [n, T]): -> (shown, hit | None) int32 [len(KS), n_items]."""
    valid = (topk >= 0) & (topk < n_items)
    member = None if tgt is None else (topk[:, :, None] == tgt[:, None, :]).any(dim=2)
    shown = torch.zeros((len(KS), n_items), dtype=torch.int32, device=topk.device)
    hit = None if tgt is None else torch.zeros_like(shown)
    lo = 0
    for b, k in enumerate(KS):
        hi = min(k, topk.shape[1])
        ids, ok = topk[:, lo:hi], valid[:, lo:hi]
        shown[b] += torch.bincount(ids[ok].long(), minlength=n_items).int()
        if tgt is not None:
            hit[b] += torch.bincount(ids[ok & member[:, lo:hi]].long(), minlength=n_items).int()
        lo = hi
    return shown, hit


def targets_for(topk, g):
    """Ten targets per row, unsorted: three ids of the row's own list among seven random ones."""
    n = topk.shape[0]
    cols = torch.randint(0, topk.shape[1], (n, 3), device=topk.device, generator=g)
    own = torch.gather(topk, 1, cols).clamp(min=0)
    rnd = torch.randint(0, N_ITEMS, (n, N_TGT - 3), dtype=torch.int32, device=topk.device, generator=g)
    tgt = torch.cat([rnd[:, :4], own, rnd[:, 4:]], dim=1).contiguous()
    return tgt, torch.arange(n + 1, dtype=torch.int64, device=topk.device) * N_TGT


def measure(name, topk, g, runs, extra=None):
    tgt, tptr = targets_for(topk, g)
    flat = tgt.view(-1)
    s_k, h_k = ops.list_exposure(topk, KS, N_ITEMS, tptr, flat)
    s_p, h_p = ops.list_exposure(topk, KS, N_ITEMS, tptr, flat, plain=True)
    s_t, h_t = torch_route(topk, N_ITEMS, tgt)
    pt = {"lists": name, "rows": topk.shape[0], "columns": topk.shape[1], "items": N_ITEMS, "Ks": KS, "targets_per_row": N_TGT,
          "kernel_equals_torch": bool(torch.equal(s_k, s_t) and torch.equal(h_k, h_t)),
          "plain_equals_torch": bool(torch.equal(s_p, s_t) and torch.equal(h_p, h_t)),
          "distinct_items_shown": int((s_t.sum(dim=0) > 0).sum()), "hits": int(h_t.sum()),
          "entries_on_the_1000_most_shown_items": float(torch.sort(s_t.sum(dim=0), descending=True).values[:1000].sum()) / float(s_t.sum())}
    shown, hit = torch.zeros_like(s_k), torch.zeros_like(s_k)
    fns = {"exposure": lambda: ops.list_exposure(topk, KS, N_ITEMS, tptr, flat, shown, hit),
           "exposure_no_targets": lambda: ops.list_exposure(topk, KS, N_ITEMS, None, None, shown),
           "plain": lambda: ops.list_exposure(topk, KS, N_ITEMS, tptr, flat, shown, hit, plain=True),
           "plain_no_targets": lambda: ops.list_exposure(topk, KS, N_ITEMS, None, None, shown, plain=True),
           "torch": lambda: torch_route(topk, N_ITEMS, tgt),
           "torch_no_targets": lambda: torch_route(topk, N_ITEMS),
           "read_lists": lambda: topk.max()}
    fns.update(extra(tptr, flat) if extra else {})
    t = alternate(runs, fns)
    pt.update({k + "_ms": v for k, v in t.items()})
    for a, b in (("exposure", "torch"), ("exposure_no_targets", "torch_no_targets"), ("exposure", "plain"), ("exposure_no_targets", "plain_no_targets")):
        pt["%s_wholly_below_%s" % (a, b)] = max(t[a]) < min(t[b])
        pt["%s_over_%s_run_by_run" % (b, a)] = [y / x for x, y in zip(t[a], t[b])]
    return pt, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=262144)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    out = {}

    w = synthetic.make_workload("c3", dev)
    assert w.n_items == N_ITEMS
    users = torch.arange(a.rows, dtype=torch.int32, device=dev)
    hist = ops.HistoryCSR(w.hist_indptr, w.hist_indices, by_user=True)

    def rank():
        return ops.recommend_topk(w.U, w.I, users, K_COLS, ops.HEAD_POP, w.pop_last, hist)

    topk = rank()[0]
    ks_dev = torch.as_tensor(KS, dtype=torch.int32, device=dev)
    pt, t = measure("pda", topk, g, a.runs, extra=lambda tptr, flat: {"recommend_topk": rank,
                                                                      "metrics_sums": lambda: ops.metrics_sums(topk, tptr, flat, ks_dev)})
    block = [r + m + e for r, m, e in zip(t["recommend_topk"], t["metrics_sums"], t["exposure"])]
    pt["exposure_share_of_block_run_by_run"] = [e / b for e, b in zip(t["exposure"], block)]
    out["pda"] = pt
    del w, hist, topk

    start = torch.randint(0, N_ITEMS, (a.rows, 1), device=dev, generator=g)
    stride = torch.randint(1, N_ITEMS // K_COLS, (a.rows, 1), device=dev, generator=g)
    topk = ((start + stride * torch.arange(K_COLS, device=dev)[None, :]) % N_ITEMS).int().contiguous()
    out["uniform"] = measure("uniform", topk, g, a.runs)[0]
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
