"""Deep-list timings on one GPU (device events, a warm-up of every shape), one JSON object on stdout:
  compare  8 192 users x 200 000 items x 128, K in {100, 1000}, both heads, no history.  Route A = ops.recommend_topk_deep; route B = the only
           way to a list deeper than 54 without it: ops.score_dense + torch.topk(sorted=True) in 2 048-user chunks.  Five alternating runs
           of both routes per point, every run timed by itself; the outputs of the two routes are compared first (values bit for bit, ids
           wherever the row's values are distinct).
  big      one 262 144-user block x 200 000 items x 128, raw head: the deep call at K = 1 000 (chunked to its workspace budget) against the
           exact K = 50 kernel pda_score_topk_f32 (generation 1, the floor of an exact fp32 sweep) on the same block; workspace bytes.
  one      a single deep call at the compare shape, K = 1 000 (for a rocprofv3 --kernel-trace --stats run of its own).
Usage: python tools/deep_topk_timing.py [--only compare|big|one] [--runs 5]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pda_amd import ops  # noqa: E402


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def dense_route(U, I, users, K, head, pop, chunk=2048):
    idx = torch.empty((users.numel(), K), dtype=torch.int64, device=U.device)
    val = torch.empty((users.numel(), K), dtype=torch.float32, device=U.device)
    for lo in range(0, users.numel(), chunk):
        s = ops.score_dense(U, I, users[lo:lo + chunk], head, pop)
        v, i = torch.topk(s, K, dim=1, sorted=True)
        idx[lo:lo + chunk], val[lo:lo + chunk] = i, v
    return idx, val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("compare", "big", "one"), default=None)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    nI, d = 200000, 128
    I = torch.randn(nI, d, device=dev, generator=g) * 0.1
    pop = torch.rand(nI, device=dev, generator=g) ** 0.22 + 1e-3
    out = {"n_items": nI, "d": d}
    if a.only in (None, "compare", "one"):
        nU = 8192
        U = torch.randn(nU, d, device=dev, generator=g) * 0.1
        users = torch.randperm(nU, device=dev, generator=g).int()
        if a.only == "one":
            ops.recommend_topk_deep(U, I, users, 1000, ops.HEAD_RAW)
            torch.cuda.synchronize()
            out["one_ms"] = once(lambda: ops.recommend_topk_deep(U, I, users, 1000, ops.HEAD_RAW))[0]
        else:
            pts = []
            for head in (ops.HEAD_RAW, ops.HEAD_POP):
                for K in (100, 1000):
                    p = pop if head == ops.HEAD_POP else None
                    fa = lambda: ops.recommend_topk_deep(U, I, users, K, head, p)      # noqa: E731
                    fb = lambda: dense_route(U, I, users, K, head, p)                  # noqa: E731
                    (ia, va), (ib, vb) = fa(), fb()                                     # warm-up of both routes at this point, and the comparison
                    torch.cuda.synchronize()
                    distinct = (va[:, 1:] != va[:, :-1]).all(dim=1)
                    pt = {"head": head, "K": K, "values_equal": bool(torch.equal(va, vb)),
                          "ids_equal_on_rows_without_ties": bool(torch.equal(ia[distinct].long(), ib[distinct])),
                          "rows_with_ties": int((~distinct).sum())}
                    del ia, va, ib, vb
                    ta, tb = [], []
                    for _ in range(a.runs):
                        ta.append(once(fa)[0])
                        tb.append(once(fb)[0])
                    pt.update(deep_ms=ta, dense_topk_ms=tb, deep_range=[min(ta), max(ta)], dense_topk_range=[min(tb), max(tb)],
                              deep_wholly_below=max(ta) < min(tb), workspace_bytes=ops.deep_workspace_bytes(nU, nI, d, K))
                    pts.append(pt)
            out["compare_users"] = nU
            out["compare"] = pts
        del U, users
    if a.only in (None, "big"):
        nU, nb = 1 << 20, 262144
        U = torch.randn(nU, d, device=dev, generator=g) * 0.1
        users = torch.randperm(nU, device=dev, generator=g)[:nb].int()
        st = {}
        fd = lambda: ops.recommend_topk_deep(U, I, users, 1000, ops.HEAD_RAW, stats=st)                      # noqa: E731
        fe = lambda: ops.score_topk_keys(U, I, users, 50, ops.HEAD_RAW, impl="v1")                          # noqa: E731
        fd(), fe()
        torch.cuda.synchronize()
        td, te = [], []
        for _ in range(max(2, a.runs // 2)):
            td.append(once(fd)[0])
            te.append(once(fe)[0])
        out["big"] = {"users": nb, "deep_k1000_ms": td, "exact_k50_ms": te, "ratio": min(td) / min(te), "chunk_users": st["chunk_users"],
                      "workspace_bytes_per_chunk": st["workspace_bytes"], "workspace_bytes_whole_block": ops.deep_workspace_bytes(nb, nI, d, 1000)}
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
