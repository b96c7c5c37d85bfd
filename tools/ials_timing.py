"""iALS timings on one GPU (device events, warm-up), one JSON object on stdout, on a graph of the Douban shape of tools/cli_epoch.py
(47 890 users x 26 047 items, Zipf items, log-normal user lengths, about 6.9 M distinct pairs), d = 64 and 128:
  user_sweep    pda_ials_half_sweep_f32 over the user rows (the Gram matrix of the item table is computed once, outside)
  item_sweep    the same over the item rows: the Zipf side, where rows above PDA_IALS_CHUNK pairs are cut
  item_uncut    the item rows with the cut off (a work list with chunk = infinity): what the cut buys
  gram          pda_ials_gram_f32 of the item table
  epoch         both Gram matrices, both half-sweeps and the objective (IALSMF.train_epoch's launches)
  torch_user / torch_item   the torch restatement of a half-sweep: rows in blocks of falling length, a padded gather per block, bmm,
                torch.linalg.cholesky and cholesky_solve
--runs alternating runs of all of them in this process, each timed by itself; the median and the range of each.  Every measurement runs under
its own time limit: a watchdog ends the process (exit status 124) when one exceeds it, and nothing is started after it.
Before anything is timed, a sample of rows (the longest of each side among them) of the kernel's and of the torch restatement's result is held
to the a-priori bound of tests/ials_ref.py against the float64 solution; a miss ends the run.
Reported beside the times: the floor computed from the shapes -- the larger of (2 nnz d^2 + rows d^3 / 3) flops at the fp32 rate (157.3 TFLOPS)
and the gathered bytes nnz d 4 at the HBM bandwidth (8 TB/s) -- and which of the two binds.
Usage: python tools/ials_timing.py [--runs 5] [--reps 3] [--limit 120] [--dims 64,128]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ials_ref as ir  # noqa: E402
from lightgcn_timing import limit, shaped_pairs, timed_ms  # noqa: E402
from pda_amd import ops  # noqa: E402

F32_FLOPS, HBM_BYTES = 157.3e12, 8.0e12
NONFINITE = [0]         # rows for which torch's batched Cholesky path gave non-finite values (solved again by LU)


def torch_half_sweep(side, Z, G, alpha0, X_out, budget=1 << 27):
    """The restatement in torch: the rows by falling length in blocks whose padded gather holds at most `budget` floats."""
    d = Z.shape[1]
    lens = side.indptr[1:] - side.indptr[:-1]
    order = torch.argsort(lens, descending=True, stable=True)
    eye = torch.eye(d, device=Z.device)
    n, i = side.n_rows, 0
    lens_h = lens[order].cpu().tolist()
    while i < n:
        L = max(1, lens_h[i])
        nb = max(1, min(n - i, budget // (L * d)))
        rows = order[i:i + nb]
        ar = torch.arange(L, device=Z.device)[None, :]
        m = ar < lens[rows][:, None]
        idx = side.indices[(side.indptr[rows][:, None] + ar).clamp(max=max(0, side.nnz - 1))].long()
        Zg = Z[idx] * m[..., None]
        A = torch.bmm(Zg.transpose(1, 2), Zg) + alpha0 * G + side.lam_row[rows][:, None, None] * eye
        b = Zg.sum(1)
        x = torch.cholesky_solve(b[..., None], torch.linalg.cholesky(A))[..., 0]
        bad = ~torch.isfinite(x).all(1)
        if bad.any():       # (a batched Cholesky that returns non-finite rows on systems that are positive definite: those rows by LU, and counted)
            x[bad] = torch.linalg.solve(A[bad], b[bad])
            NONFINITE[0] += int(bad.sum())
        X_out[rows] = x
        i += nb
    return X_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds per measurement")
    ap.add_argument("--users", type=int, default=47890)
    ap.add_argument("--items", type=int, default=26047)
    ap.add_argument("--mean_hist", type=int, default=212)
    ap.add_argument("--dims", type=str, default="64,128")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nU, nI = a.users, a.items
    alpha0, lam, nu = 0.1, 0.05, 1.0
    u, it = shaped_pairs(nU, nI, a.mean_hist)
    g = ops.IalsGraph(u, it, nU, nI, dev, lam=lam, alpha0=alpha0, nu=nu)
    g_uncut = ops.IalsGraph(u, it, nU, nI, dev, lam=lam, alpha0=alpha0, nu=nu, chunk=1 << 40)
    out = {"shape": {"users": nU, "items": nI, "pairs": g.nnz, "chunk": ops.IALS_CHUNK, "alpha0": alpha0, "lambda": lam, "nu": nu,
                     "longest_user": int(g.user.host["deg"].max()), "longest_item": int(g.item.host["deg"].max()),
                     "cut_items": g.item.all_rows.n_long, "item_slots": g.item.all_rows.n_slots, "cut_users": g.user.all_rows.n_long}}
    gen = torch.Generator(device=dev).manual_seed(2021)
    for d in [int(x) for x in a.dims.split(",")]:
        X = (torch.rand((nU, d), device=dev, generator=gen) - 0.5) * 0.2
        Y = (torch.rand((nI, d), device=dev, generator=gen) - 0.5) * 0.2
        Xo, Yo, Xt, Yt = (torch.empty_like(t) for t in (X, Y, X, Y))
        GY, GX = ops.ials_gram(Y), ops.ials_gram(X)
        res = {}
        # ---- correctness first: a sample of rows of both results inside the a-priori bound
        NONFINITE[0] = 0
        with limit(a.limit, "check d=%d" % d):
            ops.ials_half_sweep(g, "user", Y, Xo, G=GY)
            ops.ials_half_sweep(g, "item", X, Yo, G=GX)
            Yu = torch.empty_like(Y)
            ops.ials_half_sweep(g_uncut, "item", X, Yu, G=GX)
            torch.cuda.synchronize()
            short = torch.from_numpy(g.item.host["deg"] <= ops.IALS_CHUNK).to(dev)      # rows the cut leaves whole: the same bits either way
            res["uncut_equals_cut_on_whole_rows"] = bool(torch.equal(Yu[short], Yo[short]))
            have_torch = True
            try:
                torch_half_sweep(g.user, Y, GY, alpha0, Xt)
                torch_half_sweep(g.item, X, GX, alpha0, Yt)
                torch.cuda.synchronize()
                res["torch_cholesky_nonfinite_rows_redone_by_lu"] = NONFINITE[0]
            except RuntimeError as e:               # (a torch build without a batched Cholesky on this device)
                have_torch, res["torch_error"] = False, str(e).splitlines()[0][:200]
        rs = np.random.default_rng(1)
        for name, side, Z, mine, theirs in (("user", g.user, Y, Xo, Xt), ("item", g.item, X, Yo, Yt)):
            rows = np.unique(np.concatenate([rs.integers(0, side.n_rows, 12), [int(side.host["deg"].argmax())]]))
            b = ir.row_bounds(side.host["indptr"], side.host["indices"], Z.cpu().numpy(), alpha0, side.host_lam_row, rows)
            allowed = b["bound"] * b["xnorm"]
            for tag, t in (("kernel", mine),) + ((("torch", theirs),) if have_torch else ()):
                err = np.linalg.norm(t[torch.from_numpy(rows).to(dev)].cpu().numpy().astype(np.float64) - b["x"], axis=1)
                res["%s_%s_observed_over_bound" % (name, tag)] = float(np.max(err / np.maximum(allowed, 1e-300)))
                if not (err <= allowed).all():
                    print(json.dumps({"error": "%s %s rows outside the bound at d=%d" % (name, tag, d), "partial": res}))
                    sys.exit(2)
        res["failed_pivots"] = int(g.buffers(d)["fail"].item()) + int(g_uncut.buffers(d)["fail"].item())

        def epoch():
            ops.ials_half_sweep(g, "user", Y, Xo)
            ops.ials_half_sweep(g, "item", Xo, Yo)
            ops.ials_loss(g, Xo, Yo)

        what = {"user_sweep": lambda: ops.ials_half_sweep(g, "user", Y, Xo, G=GY),
                "item_sweep": lambda: ops.ials_half_sweep(g, "item", X, Yo, G=GX),
                "item_uncut": lambda: ops.ials_half_sweep(g_uncut, "item", X, Yu, G=GX),
                "gram": lambda: ops.ials_gram(Y, g.buffers(d)["G"], g.buffers(d)["ws"]),
                "epoch": epoch}
        if have_torch:
            what["torch_user"] = lambda: torch_half_sweep(g.user, Y, GY, alpha0, Xt)
            what["torch_item"] = lambda: torch_half_sweep(g.item, X, GX, alpha0, Yt)
        ms = {k: [] for k in what}
        for _ in range(a.runs):
            for k, fn in what.items():
                with limit(a.limit, "%s d=%d" % (k, d)):
                    ms[k].append(timed_ms(fn, 1 if k.startswith("torch") else a.reps))
        res["ms"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()}
        for name, side in (("user", g.user), ("item", g.item)):
            flops = 2.0 * side.nnz * d * d + side.n_rows * d ** 3 / 3.0
            byts = side.nnz * d * 4.0
            t_f, t_b = flops / F32_FLOPS * 1e3, byts / HBM_BYTES * 1e3
            res["floor_%s" % name] = {"flops_ms": t_f, "bytes_ms": t_b, "binds": "flops" if t_f >= t_b else "bytes",
                                      "measured_over_floor": res["ms"]["%s_sweep" % name]["median"] / max(t_f, t_b)}
        if have_torch:
            res["torch_over_kernel"] = {s: res["ms"]["torch_%s" % s]["median"] / res["ms"]["%s_sweep" % s]["median"] for s in ("user", "item")}
        res["uncut_over_cut"] = res["ms"]["item_uncut"]["median"] / res["ms"]["item_sweep"]["median"]
        out["d%d" % d] = res
        sys.stderr.write("d=%d done: %s\n" % (d, json.dumps(res["ms"])))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
