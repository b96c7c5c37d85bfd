"""Deep lists on item shards, timings on one GPU (device events, a warm-up of every shape), one JSON object on stdout:
  merge  R = 8 lists of K in {100, 1000} random sorted keys for 65 536 rows.  Route A = ops.deep_merge (to keys, and to ids + values); route B =
         the torch route a user has without it: the lists concatenated per row, the sign bit flipped into int64 order, torch.sort(descending)
         [:, :K].  The outputs are compared first; five alternating runs, every run timed by itself; beside them the time the bytes of the
         merge take at 5.5 TB/s (a row reads R K 8 B and writes K 8 B per output form).
  shard  one emulated rank's share of config 3: 65 536 users x 25 000 items x 128, K = 1 000 -- ops.deep_shard_keys on the rank's shard, then
         ops.deep_merge of the eight shards' lists -- against ops.recommend_topk_deep on the 200 000 items for the same users (the only way to
         these lists without the merge).  The merged lists are compared with that call's first.
  one    a single merge at R = 8, K = 1 000 (for a rocprofv3 --kernel-trace --stats run of its own).
No collective runs here: RCCL itself stays unexecuted on one GPU.
Usage: python tools/deep_shard_timing.py [--only merge|shard|one] [--runs 5]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pda_amd import ops  # noqa: E402
from pda_amd.dist import shard_range  # noqa: E402

SIGN = -(1 << 63)
ACHIEVABLE_BYTES_PER_S = 5.5e12


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def random_lists(R, rows, K, dev, g):
    """int64 [R, rows, K]: positive 62-bit keys (distinct but for a chance of 1e-11 per row), every list sorted descending."""
    keys = torch.randint(1, 1 << 62, (R, rows, K), dtype=torch.int64, device=dev, generator=g)
    return torch.sort(keys, dim=2, descending=True).values.contiguous()


def torch_route(keys):
    R, rows, K = keys.shape
    flat = keys.permute(1, 0, 2).reshape(rows, R * K) ^ SIGN          # u64 order as int64 order
    return torch.sort(flat, dim=1, descending=True).values[:, :K] ^ SIGN


def alternate(runs, **fns):
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(runs):
        for k, f in fns.items():
            t[k].append(once(f)[0])
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("merge", "shard", "one"), default=None)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    out = {}
    R, rows = 8, 65536
    if a.only == "one":
        keys = random_lists(R, rows, 1000, dev, g)
        ops.deep_merge(keys)
        torch.cuda.synchronize()
        out["one_ms"] = once(lambda: ops.deep_merge(keys))[0]
    if a.only in (None, "merge"):
        pts = []
        for K in (100, 1000):
            keys = random_lists(R, rows, K, dev, g)
            mk, ref = ops.deep_merge(keys, want="keys"), torch_route(keys)
            idx, val = ops.deep_merge(keys)
            torch.cuda.synchronize()
            pt = {"R": R, "rows": rows, "K": K, "keys_equal": bool(torch.equal(mk, ref)),
                  "ids_match_keys": bool(torch.equal(idx.long() & 0xFFFFFFFF, 0xFFFFFFFF - (mk & 0xFFFFFFFF)))}
            del mk, ref, idx, val
            t = alternate(a.runs, merge_keys=lambda: ops.deep_merge(keys, want="keys"), merge_idx_val=lambda: ops.deep_merge(keys),
                          torch_sort=lambda: torch_route(keys))
            nbytes = rows * (R * K * 8 + K * 8)
            pt.update({k + "_ms": v for k, v in t.items()})
            pt.update(bytes=nbytes, bytes_derived_ms=nbytes / ACHIEVABLE_BYTES_PER_S * 1e3,
                      merge_wholly_below_torch=max(t["merge_keys"] + t["merge_idx_val"]) < min(t["torch_sort"]),
                      merge_over_bytes_derived=min(t["merge_idx_val"]) / (nbytes / ACHIEVABLE_BYTES_PER_S * 1e3))
            pts.append(pt)
            del keys
        out["merge"] = pts
    if a.only in (None, "shard"):
        nU, nb, nI, d, K = 1 << 20, 65536, 200000, 128, 1000
        U = torch.randn(nU, d, device=dev, generator=g) * 0.1
        I = torch.randn(nI, d, device=dev, generator=g) * 0.1
        users = torch.randperm(nU, device=dev, generator=g)[:nb].int()
        shards = [shard_range(nI, r, R) for r in range(R)]
        tabs = [I[lo:hi].contiguous() for lo, hi in shards]
        lists = torch.stack([ops.deep_shard_keys(U, tabs[r], users, K, ops.HEAD_RAW, None, None, shards[r][0]) for r in range(R)])
        idx, val = ops.deep_merge(lists, users)
        widx, wval = ops.recommend_topk_deep(U, I, users, K, ops.HEAD_RAW)
        torch.cuda.synchronize()
        pt = {"users": nb, "items": nI, "items_per_shard": shards[0][1] - shards[0][0], "d": d, "K": K, "R": R,
              "ids_equal": bool(torch.equal(idx, widx)), "values_equal": bool(torch.equal(val, wval))}
        del idx, val, widx, wval
        t = alternate(a.runs, shard_sweep=lambda: ops.deep_shard_keys(U, tabs[0], users, K, ops.HEAD_RAW, None, None, 0),
                      merge_of_eight=lambda: ops.deep_merge(lists, users),
                      whole_catalogue=lambda: ops.recommend_topk_deep(U, I, users, K, ops.HEAD_RAW))
        pt.update({k + "_ms": v for k, v in t.items()})
        pt.update(rank_share_ms=min(t["shard_sweep"]) + min(t["merge_of_eight"]), merge_over_sweep=min(t["merge_of_eight"]) / min(t["shard_sweep"]),
                  whole_over_rank_share=min(t["whole_catalogue"]) / (min(t["shard_sweep"]) + min(t["merge_of_eight"])))
        out["shard"] = pt
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
