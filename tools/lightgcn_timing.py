"""LightGCN timings on one GPU (device events, warm-up), one JSON object on stdout, on a graph of the Douban shape of tools/cli_epoch.py
(47 890 users x 26 047 items, Zipf items, log-normal user lengths, about 6.9 M distinct pairs), d = 64, L = 3:
  product      one pda_gcn_spmm_f32 over the symmetric graph (both directions in one launch, plus the launch of the cut rows)
  propagation  ops.gcn_propagate: L products with the running sum fused
  step         LightGCN.train_step: propagate, the triplet gradient, the backward pass, the regulariser, the dense Adam sweep
  sparse_mm    torch.sparse.mm of the same CSR (int64 indices) with the same table
  mf_step      pda_adam_step_f32, the matrix-factorisation step, on tables of the same shape and the same batch
--runs alternating runs of all five in this process, the median and the range of each, and the ratio sparse_mm / product run by run.  Every
measurement runs under its own time limit: a watchdog ends the process (exit status 124) when one exceeds it, and nothing is started after it.
The product's output is compared with torch.sparse.mm first (1e-5 absolute; a mismatch ends the run before anything is timed).
Reported beside the times: the bytes the product moves by its shapes (nnz x (256-byte row + index + weight) + the rows written + the work
list) over its time, next to the gather rates MI355X is known for (5.5 - 5.8 TB/s for random whole rows from HBM, 8.6 TB/s from a 38 MB table
that stays in the Infinity Cache: the table here is 18.9 MB), and the most loaded and the median entry of the work list.
Usage: python tools/lightgcn_timing.py [--runs 5] [--reps 20] [--limit 60]"""
import argparse
import json
import os
import statistics
import sys
import threading

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pda_amd import ops  # noqa: E402


class limit:
    """A time limit around one measurement: past it the process ends with status 124 (a hung launch never returns to Python)."""

    def __init__(self, seconds, what):
        self.t = threading.Timer(seconds, lambda: (sys.stderr.write("time limit: %s\n" % what), sys.stderr.flush(), os._exit(124)))
        self.t.daemon = True

    def __enter__(self):
        self.t.start()

    def __exit__(self, *exc):
        self.t.cancel()


def shaped_pairs(n_users, n_items, mean_hist, seed=2020):
    """The pair recipe of tools/cli_epoch.write_shaped_dataset, without the files."""
    rng = np.random.default_rng(seed)
    sigma = 0.8
    lens = np.clip(np.exp(rng.standard_normal(n_users) * sigma + np.log(mean_hist) - 0.5 * sigma * sigma), 3, n_items // 2).astype(np.int64)
    u = np.repeat(np.arange(n_users, dtype=np.int64), lens)
    w = 1.0 / np.arange(1, n_items + 1)
    cdf = np.cumsum(w / w.sum())
    it = rng.permutation(n_items)[np.minimum(np.searchsorted(cdf, rng.random(u.size)), n_items - 1)]
    return u, it


def timed_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=float, default=60.0, help="seconds per measurement")
    ap.add_argument("--users", type=int, default=47890)
    ap.add_argument("--items", type=int, default=26047)
    ap.add_argument("--mean_hist", type=int, default=212)
    a = ap.parse_args()
    from pda_amd.model_api import LightGCN
    from pda_amd.parse import parse_args
    dev = torch.device("cuda:0")
    nU, nI, d, L, B = a.users, a.items, 64, 3, 1024
    N = nU + nI
    u, it = shaped_pairs(nU, nI, a.mean_hist)
    args = parse_args(["--model", "lightgcn", "--embed_size", str(d), "--batch_size", str(B), "--gcn_layers", str(L), "--verbose", "0"])
    with limit(a.limit, "graph build"):
        model = LightGCN(args, {"n_users": nU, "n_items": nI, "gcn_train_pairs": (u, it)}, device=dev)
    g = model.graph
    lens = (g.host["work"][:, 2] - g.host["work"][:, 1])
    nnz = int(g.indices.numel())
    out = {"shape": [nU, nI, d], "layers": L, "B": B, "pairs": g.n_edges, "nnz_symmetric": nnz, "work_entries": int(len(lens)),
           "cut_rows": int(g.long_rows.shape[0]), "chunk": ops.GCN_CHUNK, "entry_edges_max": int(lens.max()), "entry_edges_median": float(np.median(lens)),
           "row_edges_max": int(np.diff(g.host["indptr"]).max()), "runs": a.runs, "reps": a.reps}
    gen = torch.Generator(device=dev).manual_seed(1)
    X = model._E0
    Y = torch.empty_like(X)
    users = torch.randint(0, nU, (B,), device=dev, generator=gen, dtype=torch.int32)
    pos = torch.randint(0, nI, (B,), device=dev, generator=gen, dtype=torch.int32)
    neg = torch.randint(0, nI, (B,), device=dev, generator=gen, dtype=torch.int32)

    sp = None
    try:
        with limit(a.limit, "sparse build and check"):
            sp = torch.sparse_csr_tensor(g.indptr, g.indices.long(), g.w, size=(N, N))
            ref = torch.sparse.mm(sp, X)
            ops.gcn_spmm(g, X, Y=Y)
            out["product_vs_sparse_mm_max_err"] = float((Y - ref).abs().max())
            if not out["product_vs_sparse_mm_max_err"] <= 1e-5:
                out["error"] = "outputs differ: nothing timed"
                print(json.dumps(out))
                raise SystemExit(1)
    except RuntimeError as e:                                 # (a torch build without CSR x dense on this device)
        out["sparse_mm"] = "not measured: " + str(e).splitlines()[0][:200]
        sp = None

    U2, I2 = X[:nU].clone(), X[nU:].clone()
    z = torch.zeros_like
    tags = ops.adam_row_tags(nU, nI, dev)
    mf = (U2, z(U2), z(U2), z(U2), tags[0], I2, z(I2), z(I2), z(I2), tags[1])
    k = [0]

    def mf_step():
        k[0] += 1
        ops.adam_step(*mf, users, pos, neg, regs=1e-5, reg_div=B, step=1 + (k[0] & 1), lr_t=1e-4)
    jobs = {"product": lambda: ops.gcn_spmm(g, X, Y=Y), "propagation": lambda: ops.gcn_propagate(g, X[:nU], X[nU:], L),
            "step": lambda: model.train_step(users, pos, neg), "mf_step": mf_step}
    if sp is not None:
        jobs["sparse_mm"] = lambda: torch.sparse.mm(sp, X)
    times = {n: [] for n in jobs}
    for _ in range(a.runs):
        for n, fn in jobs.items():
            with limit(a.limit, n):
                times[n].append(timed_ms(fn, a.reps))
    for n in jobs:
        out[n + "_ms"] = statistics.median(times[n])
        out[n + "_range_ms"] = [min(times[n]), max(times[n])]
    if sp is not None:
        r = [s / p for s, p in zip(times["sparse_mm"], times["product"])]
        out["sparse_mm_over_product"] = statistics.median(r)
        out["sparse_mm_over_product_range"] = [min(r), max(r)]
        out["ranges_overlap"] = bool(min(times["sparse_mm"]) <= max(times["product"]))
    moved = nnz * (d * 4 + 8) + N * d * 4 + len(lens) * 32
    out["product_bytes"] = int(moved)
    out["product_TB_per_s"] = moved / (out["product_ms"] * 1e-3) / 1e12
    out["product_TB_per_s_range"] = [moved / (t * 1e-3) / 1e12 for t in (max(times["product"]), min(times["product"]))]
    out["guide_gather_TB_per_s"] = {"random rows from HBM": [5.5, 5.8], "38 MB table in the Infinity Cache": 8.6}
    out["table_MB"] = N * d * 4 / 1e6
    out["step_over_mf_step"] = out["step_ms"] / out["mf_step_ms"]
    out["measured_on"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
