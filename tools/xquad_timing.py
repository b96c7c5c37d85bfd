"""xQuAD re-ranking, timings on one GPU (device events, a warm-up of every shape), one JSON object on stdout:
  rerank  262 144 rows x N = 1 000 sorted synthetic candidates over 200 000 items (a fifth of them head), 32 history entries per row, K = 50,
          lambda = 0.5, both variants.  Route A = ops.xquad_rerank (one launch); route B = the torch restatement of the same K-step selection on
          the device, which is what a user has without it: [rows, N] tensors, an arg-max per step.  The outputs are compared first (the
          values are random normals: no ties, so torch's arg-max has no choice to make); five alternating runs, every run timed by itself;
          beside them the time 8 B x N per row (every candidate read once) and the outputs take at 5.5 TB/s.
  block   one xQuAD evaluation block: deep candidates (ops.recommend_topk_deep) at 65 536 users x 200 000 items x 128, K = 1 000, then the
          re-ranking of those lists: the re-ranking's share of the block.
  parts   the `rerank` shape with parts of the work taken away, five alternating runs, the fastest of each: no history; K = 1 (one merge step;
          the chunks stop after the first trip); half of the items head (both categories hold K members after one trip); no head item (the
          head never fills: every chunk of the row is read); and a copy of the two candidate arrays (what streaming them costs here).
  one     a single re-ranking per variant at the `rerank` shape (for a rocprofv3 --kernel-trace --stats run of its own).
Usage: python tools/xquad_timing.py [--only rerank|block|parts|one] [--runs 5] [--rows 262144]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pda_amd import ops  # noqa: E402

ACHIEVABLE_BYTES_PER_S = 5.5e12
N_ITEMS, N, K, LAM, HIST = 200000, 1000, 50, 0.5, 32


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def alternate(runs, **fns):
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(runs):
        for k, f in fns.items():
            t[k].append(once(f)[0])
    return t


def synthetic(rows, dev, g):
    idx = torch.randint(0, N_ITEMS, (rows, N), dtype=torch.int32, device=dev, generator=g)
    val = torch.sort(torch.randn((rows, N), device=dev, generator=g), dim=1, descending=True).values.contiguous()
    is_head = (torch.rand(N_ITEMS, device=dev, generator=g) < 0.2).to(torch.uint8)
    hist = torch.sort(torch.randint(0, N_ITEMS, (rows, HIST), dtype=torch.int32, device=dev, generator=g), dim=1).values.contiguous()
    indptr = torch.arange(rows + 1, dtype=torch.int64, device=dev) * HIST
    return idx, val, is_head, hist, ops.HistoryCSR(indptr, hist.view(-1), by_user=False)


def torch_route(idx, val, is_head, hist, lam, k, variant):
    """The contract of include/pda_hip_xquad.h in torch, for rows whose candidates are all valid: the same fp32 operations in the same order."""
    f32 = torch.float32
    L = torch.tensor(lam, dtype=f32, device=idx.device)
    W = torch.tensor(1.0 - lam, dtype=f32, device=idx.device)
    first = torch.ones_like(hist, dtype=torch.bool)
    first[:, 1:] = hist[:, 1:] != hist[:, :-1]
    H = first.sum(dim=1)
    H1 = (first & (is_head[hist.long()] != 0)).sum(dim=1)
    q = torch.stack([(H - H1).to(f32) / H.to(f32), H1.to(f32) / H.to(f32)], dim=1)
    q = torch.where(H[:, None] > 0, q, torch.zeros_like(q))
    lo = val[:, -1:]
    rng = val[:, :1] - lo
    p = torch.where((rng != 0) & torch.isfinite(rng), (val - lo) / rng, torch.zeros_like(val))
    wp = W * p
    cat = is_head[idx.long()] != 0
    avail = torch.ones_like(cat)
    n = torch.zeros((idx.shape[0], 2), dtype=torch.int64, device=idx.device)
    rows = torch.arange(idx.shape[0], device=idx.device)
    out_idx = torch.empty((idx.shape[0], k), dtype=torch.int32, device=idx.device)
    out_val = torch.empty((idx.shape[0], k), dtype=f32, device=idx.device)
    ninf = torch.tensor(float("-inf"), dtype=f32, device=idx.device)
    for t in range(k):
        if variant == "binary":
            cov = (n == 0).to(f32)
        elif t == 0:
            cov = torch.ones_like(q)
        else:
            cov = 1.0 - n.to(f32) / torch.full((), float(t), dtype=f32, device=idx.device)   # (a device tensor: a true division)
        bonus = L * (q * cov)
        x = wp + torch.where(cat, bonus[:, 1:2], bonus[:, 0:1])
        v, j = torch.where(avail, x, ninf).max(dim=1)
        out_idx[:, t] = idx[rows, j]
        out_val[:, t] = v
        avail[rows, j] = False
        n[rows, cat[rows, j].long()] += 1
    return out_idx, out_val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("rerank", "block", "parts", "one"), default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=262144)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    out = {}
    if a.only in (None, "rerank", "one"):
        idx, val, is_head, hist, h = synthetic(a.rows, dev, g)
        if a.only == "one":
            for variant in ("smooth", "binary"):
                ops.xquad_rerank(idx, val, is_head, LAM, K, variant, None, h)
                torch.cuda.synchronize()
                out["one_%s_ms" % variant] = once(lambda: ops.xquad_rerank(idx, val, is_head, LAM, K, variant, None, h))[0]
        else:
            pts = []
            for variant in ("smooth", "binary"):
                gi, gv = ops.xquad_rerank(idx, val, is_head, LAM, K, variant, None, h)
                ti, tv = torch_route(idx, val, is_head, hist, LAM, K, variant)
                torch.cuda.synchronize()
                pt = {"rows": a.rows, "N": N, "K": K, "items": N_ITEMS, "lambda": LAM, "variant": variant,
                      "ids_equal": bool(torch.equal(gi, ti)), "values_equal": bool(torch.equal(gv, tv)),
                      "rows_reordered": int((gi != idx[:, :K]).any(dim=1).sum())}
                del gi, gv, ti, tv
                t = alternate(a.runs, xquad_rerank=lambda: ops.xquad_rerank(idx, val, is_head, LAM, K, variant, None, h),
                              torch_steps=lambda: torch_route(idx, val, is_head, hist, LAM, K, variant))
                pt.update({k + "_ms": v for k, v in t.items()})
                all_bytes, out_bytes = a.rows * N * 8, a.rows * K * 8
                pt.update(candidate_bytes=all_bytes, output_bytes=out_bytes,
                          stream_all_derived_ms=(all_bytes + out_bytes) / ACHIEVABLE_BYTES_PER_S * 1e3,
                          rerank_over_stream_all=min(t["xquad_rerank"]) / ((all_bytes + out_bytes) / ACHIEVABLE_BYTES_PER_S * 1e3),
                          torch_over_rerank=min(t["torch_steps"]) / min(t["xquad_rerank"]),
                          rerank_wholly_below_torch=max(t["xquad_rerank"]) < min(t["torch_steps"]))
                pts.append(pt)
            out["rerank"] = pts
        del idx, val, is_head, hist, h
    if a.only == "parts":
        idx, val, is_head, hist, h = synthetic(a.rows, dev, g)
        no_head = torch.zeros_like(is_head)
        half = (torch.rand(N_ITEMS, device=dev, generator=g) < 0.5).to(torch.uint8)
        t = alternate(a.runs,
                      smooth=lambda: ops.xquad_rerank(idx, val, is_head, LAM, K, "smooth", None, h),
                      binary=lambda: ops.xquad_rerank(idx, val, is_head, LAM, K, "binary", None, h),
                      binary_no_history=lambda: ops.xquad_rerank(idx, val, is_head, LAM, K, "binary", None, None),
                      binary_k1=lambda: ops.xquad_rerank(idx, val, is_head, LAM, 1, "binary", None, h),
                      binary_k1_no_history=lambda: ops.xquad_rerank(idx, val, is_head, LAM, 1, "binary", None, None),
                      binary_half_head=lambda: ops.xquad_rerank(idx, val, half, LAM, K, "binary", None, h),
                      binary_no_head_reads_every_chunk=lambda: ops.xquad_rerank(idx, val, no_head, LAM, K, "binary", None, h),
                      copy_of_the_candidates=lambda: (idx.clone(), val.clone()))
        out["parts_min_ms"] = {k: min(v) for k, v in t.items()}
        del idx, val, is_head, hist, h
    if a.only in (None, "block"):
        nU, nb, d, Kc = 1 << 20, 65536, 128, 1000
        U = torch.randn(nU, d, device=dev, generator=g) * 0.1
        I = torch.randn(N_ITEMS, d, device=dev, generator=g) * 0.1
        users = torch.randperm(nU, device=dev, generator=g)[:nb].int()
        is_head = (torch.rand(N_ITEMS, device=dev, generator=g) < 0.2).to(torch.uint8)
        hist = torch.sort(torch.randint(0, N_ITEMS, (nb, HIST), dtype=torch.int32, device=dev, generator=g), dim=1).values.contiguous()
        h = ops.HistoryCSR(torch.arange(nb + 1, dtype=torch.int64, device=dev) * HIST, hist.view(-1), by_user=False)
        cidx, cval = ops.recommend_topk_deep(U, I, users, Kc, ops.HEAD_RAW, None, h)
        t = alternate(a.runs, candidates=lambda: ops.recommend_topk_deep(U, I, users, Kc, ops.HEAD_RAW, None, h),
                      rerank=lambda: ops.xquad_rerank(cidx, cval, is_head, LAM, K, "smooth", None, h))
        pt = {"users": nb, "items": N_ITEMS, "d": d, "candidates": Kc, "K": K}
        pt.update({k + "_ms": v for k, v in t.items()})
        pt.update(rerank_share_of_block=min(t["rerank"]) / (min(t["rerank"]) + min(t["candidates"])))
        out["block"] = pt
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
