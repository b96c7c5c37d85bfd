"""Exact ranks of held-out items (pda_rank_keys_*, pda_rank_count_*, include/pda_hip_rank.h), timings on one GPU: device events, a warm-up of
every variant, five alternating runs in one process, one JSON object on stdout.

Shapes (popularity head, the history mask of the synthetic workload, ten targets per row, unsorted):
  c3_d128       one evaluation block of 262 144 users x 200 000 items, d = 128
  c3_d64        the same block at d = 64
  c2            50 000 users x 20 000 items, d = 64
  c3_d128_long  the first shape with one row of 5 000 targets (157 chunks of PDA_RANK_TCHUNK for that row's workgroups)
Variants:
  rank_keys     the keys of the target entries
  rank_count    the counts above them and the lengths of the rankings
  deep_1024     ops.recommend_topk_deep at K = 1 024 on the same block: the sweep whose front end rank_count shares
  torch         the restatement a user has without the kernels: ops.score_dense over chunks of 2 048 users, the history mask, a gather of the
                target scores, comparison counts by (value, id) per target slot (slots only a few rows have are compared on those rows alone)
The ranks and lengths of the two routes are compared before anything is timed.
Usage: python tools/rank_timing.py [--runs 5] [--rows 262144] [--shapes c3_d128,c3_d64,c2,c3_d128_long]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pda_amd import ops, synthetic  # noqa: E402

N_TGT, LONG_ROW, CHUNK, DEEP_K = 10, 5000, 2048, 1024


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


def torch_route(U, I, pop, users, hist_indptr, hist_indices, tptr, tgt):
    """-> (rank int32 [n_entries], -1 = unranked; n_ranked int32 [n_users]).  hist by user id; targets a CSR by block row."""
    dev = U.device
    n_items = I.shape[0]
    ids = torch.arange(n_items, device=dev, dtype=torch.int32)[None, :]
    rank = torch.full((tgt.numel(),), -1, dtype=torch.int32, device=dev)
    n_ranked = torch.empty(users.numel(), dtype=torch.int32, device=dev)
    lens = tptr[1:] - tptr[:-1]
    for lo in range(0, users.numel(), CHUNK):
        ub = users[lo:lo + CHUNK]
        sc = ops.score_dense(U, I, ub, ops.HEAD_POP, pop)
        ul = ub.long()
        hb, he = hist_indptr[ul], hist_indptr[ul + 1]
        rows = torch.repeat_interleave(torch.arange(ub.numel(), device=dev), he - hb)
        span = torch.arange(rows.numel(), device=dev) - torch.repeat_interleave(torch.cumsum(he - hb, 0) - (he - hb), he - hb)
        sc[rows, hist_indices[hb[rows] + span].long()] = float("-inf")
        ok = sc > float("-inf")
        n_ranked[lo:lo + ub.numel()] = ok.sum(dim=1)
        ln, tb = lens[lo:lo + ub.numel()], tptr[lo:lo + ub.numel()]
        for s in range(int(ln.max())):
            has = torch.nonzero(ln > s).view(-1)
            e = tb[has] + s
            t_id = tgt[e]
            rows_s = sc if has.numel() == ub.numel() else sc[has]
            t_sc = rows_s.gather(1, t_id.long()[:, None])
            above = ((rows_s > t_sc) | ((rows_s == t_sc) & (ids < t_id[:, None]))).sum(dim=1)   # (-inf > anything is false: listed items never count)
            rank[e] = torch.where(t_sc.view(-1) > float("-inf"), above.int(), torch.full_like(above, -1).int())
    return rank, n_ranked


def measure(name, w, rows, runs, g, long_row=False):
    dev = w.U.device
    users = torch.arange(rows, dtype=torch.int32, device=dev)
    hist = ops.HistoryCSR(w.hist_indptr, w.hist_indices, by_user=True)
    lens = torch.full((rows,), N_TGT, dtype=torch.int64, device=dev)
    if long_row:
        lens[rows // 3] = LONG_ROW
    tptr = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=tptr[1:])
    tgt = torch.randint(0, w.n_items, (int(tptr[-1]),), dtype=torch.int32, device=dev, generator=g)
    max_row = int(lens.max())
    args = (w.U, w.I, users, tptr)
    kw = dict(head=ops.HEAD_POP, pop_shard=w.pop_last, hist=hist)

    keys = ops.rank_keys(*args, tgt, **kw)
    rank_k, n_k = ops.rank_targets(*args, tgt, max_row=max_row, **kw)
    rank_t, n_t = torch_route(w.U, w.I, w.pop_last, users, w.hist_indptr, w.hist_indices, tptr, tgt)
    pt = {"shape": name, "users": rows, "items": w.n_items, "d": w.U.shape[1], "targets": int(tgt.numel()), "longest_row": max_row,
          "kernels_equal_torch": bool(torch.equal(rank_k, rank_t) and torch.equal(n_k, n_t)),
          "unranked_targets": int((rank_k < 0).sum()), "median_rank": float(rank_k[rank_k >= 0].float().median())}
    above, n_ranked = torch.zeros_like(rank_k), torch.zeros_like(n_k)
    k_deep = min(DEEP_K, w.n_items)
    fns = {"rank_keys": lambda: ops.rank_keys(*args, tgt, out=keys, **kw),
           "rank_count": lambda: ops.rank_count(*args, keys, above=above, n_ranked=n_ranked, max_row=max_row, **kw),
           "deep_1024": lambda: ops.recommend_topk_deep(w.U, w.I, users, k_deep, ops.HEAD_POP, w.pop_last, hist),
           "torch": lambda: torch_route(w.U, w.I, w.pop_last, users, w.hist_indptr, w.hist_indices, tptr, tgt)}
    t = alternate(runs, fns)
    pt.update({k + "_ms": v for k, v in t.items()})
    both = [a + b for a, b in zip(t["rank_keys"], t["rank_count"])]
    pt["keys_plus_count_ms"] = both
    pt["keys_plus_count_wholly_below_torch"] = max(both) < min(t["torch"])
    pt["torch_over_keys_plus_count_run_by_run"] = [y / x for x, y in zip(both, t["torch"])]
    pt["rank_count_over_deep_1024_run_by_run"] = [x / y for x, y in zip(t["rank_count"], t["deep_1024"])]
    return pt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--shapes", default="c3_d128,c3_d64,c2,c3_d128_long")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    out = {}
    for name in a.shapes.split(","):
        if name == "c2":
            w = synthetic.make_workload("c2", dev)
            rows = w.n_users
        else:
            w = synthetic.make_workload("c3", dev, n_users=a.rows, d=64 if name == "c3_d64" else 128)
            rows = a.rows
        out[name] = measure(name, w, rows, a.runs, g, long_row=name.endswith("_long"))
        print(json.dumps({name: out[name]}), file=sys.stderr, flush=True)
        del w
        torch.cuda.empty_cache()
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
