"""Calibrated-popularity re-ranking, timings on one GPU (device events, a warm-up of every shape), one JSON object on stdout:
  rerank  262 144 rows x N = 1 000 sorted synthetic candidates over 200 000 items, 32 history entries per row, K = 50, lambda = 0.5; both
          divergences, G = 3 and G = 8 (groups drawn uniformly: every group is as likely as any other among the candidates).
          Route A = ops.calib_rerank (one launch, the profile from ops.calib_profile outside the timed part).  Route B = the torch restatement
          of the same K-step selection on the device, which is what a user has without it: [rows, N] tensors, G divergences in float64 per row
          and step, an arg-max per step.  Route C = ops.xquad_rerank at the same shape: the one-wave-per-row merge of two categories this
          project already had, as the yardstick of what such a merge costs without the double logarithms.
          The outputs of A and B are compared first (the values are random normals: no ties between candidates of one group; rows whose ids
          differ are counted, not hidden -- the device's log and torch's may round a divergence to different grid points); five alternating
          runs, every run timed by itself; beside them the time 8 B x N per row (every candidate read once) and the outputs take at 5.5 TB/s.
  parts   the G = 8 JS shape with parts of the work taken away, five alternating runs, the fastest of each: K = 1 (one step; the chunks still
          fill eight groups), lambda = 0 with an empty profile (no logarithm is evaluated), and G = 2.
Usage: python tools/calib_timing.py [--only rerank|parts] [--runs 5] [--rows 262144]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pda_amd import ops  # noqa: E402

ACHIEVABLE_BYTES_PER_S = 5.5e12
N_ITEMS, N, K, LAM, HIST, ALPHA = 200000, 1000, 50, 0.5, 32, 0.01


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
    hist = torch.sort(torch.randint(0, N_ITEMS, (rows, HIST), dtype=torch.int32, device=dev, generator=g), dim=1).values.contiguous()
    indptr = torch.arange(rows + 1, dtype=torch.int64, device=dev) * HIST
    return idx, val, ops.HistoryCSR(indptr, hist.view(-1), by_user=False)


def torch_route(idx, val, prof, item_group, G, lam, k, div, alpha):
    """The contract of include/pda_hip_calib.h in torch, for rows whose candidates are all valid: the same operations in the same order."""
    f32, f64 = torch.float32, torch.float64
    dev = idx.device
    L = torch.tensor(lam, dtype=f32, device=dev)
    W = torch.tensor(1.0 - lam, dtype=f32, device=dev)
    H = prof.sum(dim=1, keepdim=True)
    some = H > 0
    pi = torch.where(some, prof.to(f64) / H.clamp(min=1).to(f64), torch.zeros((), dtype=f64, device=dev))
    lo = val[:, -1:]
    rng = val[:, :1] - lo
    p = torch.where((rng != 0) & torch.isfinite(rng), (val - lo) / rng, torch.zeros_like(val))
    wp = W * p
    cat = item_group[idx.long()].long()
    avail = torch.ones_like(cat, dtype=torch.bool)
    n = torch.zeros((idx.shape[0], G), dtype=torch.int64, device=dev)
    rows = torch.arange(idx.shape[0], device=dev)
    eye = torch.eye(G, dtype=torch.int64, device=dev)
    out_idx = torch.empty((idx.shape[0], k), dtype=torch.int32, device=dev)
    out_val = torch.empty((idx.shape[0], k), dtype=f32, device=dev)
    out_div = torch.empty((idx.shape[0], k), dtype=f32, device=dev)
    ninf = torch.tensor(float("-inf"), dtype=f32, device=dev)
    zero, one = torch.zeros((), dtype=f64, device=dev), torch.ones((), dtype=f64, device=dev)
    for t in range(k):
        s = torch.zeros((idx.shape[0], G), dtype=f64, device=dev)                # [rows, c]
        tt = torch.full((), float(t + 1), dtype=f64, device=dev)
        for g in range(G):
            q = (n[:, g:g + 1] + eye[g][None, :]).to(f64) / tt
            pg = pi[:, g:g + 1]
            if div == "js":
                m = 0.5 * (pg + q)
                ta = torch.where(pg > 0, pg * torch.log2(torch.where(pg > 0, pg / m, one)), zero)
                tb = torch.where(q > 0, q * torch.log2(torch.where(q > 0, q / m, one)), zero)
                s = s + (ta + tb)
            else:
                qs = (1.0 - alpha) * q + alpha * pg
                s = s + torch.where(pg > 0, pg * torch.log(torch.where(pg > 0, pg / qs, one)), zero)
        D = torch.where(some, 0.5 * s if div == "js" else s, zero)
        d32 = torch.clamp(torch.round(D * 1048576.0), 0.0, 8388608.0).to(torch.int64).to(f32) * (2.0 ** -20)
        x = wp - torch.gather(L * d32, 1, cat)
        v, j = torch.where(avail, x, ninf).max(dim=1)
        cj = cat[rows, j]
        out_idx[:, t] = idx[rows, j]
        out_val[:, t] = v
        out_div[:, t] = d32[rows, cj]
        avail[rows, j] = False
        n[rows, cj] += 1
    return out_idx, out_val, out_div


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("rerank", "parts"), default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=262144)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    out = {}
    idx, val, h = synthetic(a.rows, dev, g)
    groups = {G: torch.randint(0, G, (N_ITEMS,), device=dev, generator=g).to(torch.uint8) for G in (2, 3, 8)}
    is_head = (torch.rand(N_ITEMS, device=dev, generator=g) < 0.2).to(torch.uint8)
    if a.only in (None, "rerank"):
        pts = []
        for G in (3, 8):
            prof = ops.calib_profile(groups[G], G, a.rows, None, h)
            for div in ("js", "kl"):
                gi, gv, gd = ops.calib_rerank(idx, val, prof, groups[G], G, LAM, K, div, ALPHA)
                ti, tv, td = torch_route(idx, val, prof, groups[G], G, LAM, K, div, ALPHA)
                torch.cuda.synchronize()
                same = (gi == ti).all(dim=1)
                pt = {"rows": a.rows, "N": N, "K": K, "items": N_ITEMS, "lambda": LAM, "G": G, "div": div,
                      "rows_with_other_ids": int((~same).sum()),
                      "values_equal_on_rows_with_equal_ids": bool(torch.equal(gv[same], tv[same]) and torch.equal(gd[same], td[same])),
                      "rows_reordered": int((gi != idx[:, :K]).any(dim=1).sum())}
                del gi, gv, gd, ti, tv, td, same
                t = alternate(a.runs, calib_rerank=lambda: ops.calib_rerank(idx, val, prof, groups[G], G, LAM, K, div, ALPHA),
                              torch_steps=lambda: torch_route(idx, val, prof, groups[G], G, LAM, K, div, ALPHA),
                              xquad_rerank=lambda: ops.xquad_rerank(idx, val, is_head, LAM, K, "smooth", None, h))
                pt.update({k + "_ms": v for k, v in t.items()})
                all_bytes, out_bytes = a.rows * N * 8, a.rows * K * 12
                pt.update(candidate_bytes=all_bytes, output_bytes=out_bytes,
                          stream_all_derived_ms=(all_bytes + out_bytes) / ACHIEVABLE_BYTES_PER_S * 1e3,
                          rerank_over_stream_all=min(t["calib_rerank"]) / ((all_bytes + out_bytes) / ACHIEVABLE_BYTES_PER_S * 1e3),
                          torch_over_rerank=min(t["torch_steps"]) / min(t["calib_rerank"]),
                          rerank_over_xquad=min(t["calib_rerank"]) / min(t["xquad_rerank"]),
                          rerank_wholly_below_torch=max(t["calib_rerank"]) < min(t["torch_steps"]))
                pts.append(pt)
        out["rerank"] = pts
    if a.only in (None, "parts"):
        prof8 = ops.calib_profile(groups[8], 8, a.rows, None, h)
        prof2 = ops.calib_profile(groups[2], 2, a.rows, None, h)
        none8 = torch.zeros_like(prof8)
        first_k = idx[:, :K].contiguous()
        t = alternate(a.runs,
                      js_g8=lambda: ops.calib_rerank(idx, val, prof8, groups[8], 8, LAM, K, "js", ALPHA),
                      js_g8_k1=lambda: ops.calib_rerank(idx, val, prof8, groups[8], 8, LAM, 1, "js", ALPHA),
                      js_g8_no_profile_lambda_0=lambda: ops.calib_rerank(idx, val, none8, groups[8], 8, 0.0, K, "js", ALPHA),
                      js_g2=lambda: ops.calib_rerank(idx, val, prof2, groups[2], 2, LAM, K, "js", ALPHA),
                      profile_g8=lambda: ops.calib_profile(groups[8], 8, a.rows, None, h),
                      list_counts_g8=lambda: ops.calib_list_counts(first_k, groups[8], 8, [20, 50]),
                      copy_of_the_candidates=lambda: (idx.clone(), val.clone()))
        out["parts_min_ms"] = {k: min(v) for k, v in t.items()}
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
