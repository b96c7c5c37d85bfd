#!/usr/bin/env python
"""bench.py -- PDA BPR-MF hot path on MI355X: full-catalogue score + mask + top-K@50 users/s (headline `value`)
and BPR triplets/s (reported beside it), on synthetic Douban-shaped data (pda_amd/synthetic.py).

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]   (N>1: launched by torch.distributed.run, one rank per GPU)

A "step" is one pass of the evaluation hot path over one block of `--eval-block` users against the WHOLE item
catalogue: score + history mask + top-K on every rank's item shard (bf16 MFMA pre-filter, exact fp32 rescoring of the
survivors: bit-identical to the exact fp32 kernel), for N > 1 one RCCL all-to-all of the packed partial lists (rank r
receives every shard's list for ITS slice of the users) and the merge.  Inputs are resident in HBM before the timed
region.  Scaling is STRONG: the catalogue and the users per step are fixed while N grows (item-parallel sharding of
BASELINE config 3 -> 4).

The headline is a DENSE sweep: every user x item pair is scored, the catalogue being visited most popular first.  A plain
run measures only that: set-up, W warm-up steps, K timed steps, the result line with `roofline` (dominant kernel = the score
kernel, bound = bf16 MFMA; achieved from the algorithmic flops 2*Bu*I_local*d per launch and the kernel's HIP-event
duration in the timed steps).  --full adds everything beside it: `dense_natural_order` (the same in item-id order),
`ordered_sweep` (the product default for the PDA head: the same visiting order with exact early termination on a
popularity bound -- same results, most of the catalogue never scored), `raw_head`, `prep`, the measured peaks and the
box's clocks in `roofline`, `cpu_baseline` (torch-CPU restatement of the reference op sequence, oracle/cpu_baseline.py,
bounded sample, rank 0, N=1 only), `train` (fused BPR step throughput on BASELINE config 2, N=1 only), `per_config`,
`eval_block_2048` and, from four ranks on, `user_groups_grid`.
--dump-outputs DIR writes what the headline path returned in its last timed step as .npy files (dump_outputs).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3    # MI355X dense fp32 matrix peak (guides/MI355X_MICROARCH.md)
PEAK_BF16_MFMA_TFLOPS = 2500.0  # dense bf16 matrix peak (same guide; the 5 PF figure is 2:1 sparse)
PEAK_HBM_GBS = 8000.0


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--workload", default="c3", choices=["c1", "c2", "c3", "c5shard", "tiny"])
    p.add_argument("--table-dtype", default="auto", choices=["auto", "f32", "bf16"],
                   help="embedding table type (auto: bf16 for c5shard -- BASELINE config 5 --, f32 otherwise)")
    p.add_argument("--user-groups", type=int, default=0,
                   help="N > 1: user groups of the 2-D layout (0 = pda_amd.dist.default_user_groups: 1 = item shards only, BASELINE config 4's layout); "
                        "inside a group the catalogue is item-sharded, the groups split the users of a block")
    p.add_argument("--no-per-config", action="store_true", help="skip the per_config block (C1, C2: evaluation and training beside the headline)")
    p.add_argument("--eval-block", type=int, default=262144, help="users per step (the default of the product's --eval_block)")
    p.add_argument("--head", default="condition", choices=["main_branch", "condition"])
    p.add_argument("--K", type=int, default=50)
    p.add_argument("--no-train", action="store_true")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-cli-epoch", action="store_true", help="skip per_config.c1.cli_epoch (the drop-in CLI on the Douban-shaped synthetic: ~15 s)")
    p.add_argument("--train-steps", type=int, default=2048)
    p.add_argument("--cpu-budget", type=float, default=20.0, help="seconds of CPU work for the baseline sample")
    p.add_argument("--extras-path", default=None, help="where the full record goes (default: bench_extras.json in the cwd)")
    p.add_argument("--headline-only", action="store_true",
                   help="time only the headline sweep (PMC passes: the other sweep modes launch the same kernel template)")
    p.add_argument("--full", action="store_true",
                   help="measure everything beside the headline too (the other sweeps, training, CPU baseline, per_config, ...); "
                        "a plain run sets up, warms up, times the headline steps and prints the result line")
    p.add_argument("--dump-outputs", default=None, metavar="DIR",
                   help="after the timed steps, write the top-K lists of the last timed step to DIR/*.npy (rank 0)")
    p.add_argument("--train-sharded", action="store_true",
                   help="N>1 only: also time the item-parallel SGD step (pda_amd.dist.ItemShardedBPR); off by default -- "
                        "it is latency-bound by its per-step all-gather and buys capacity, not speed")
    return p.parse_args()


def dist_world_size():
    import torch.distributed as dist
    return dist.get_world_size()


def dist_backend():
    import torch.distributed as dist
    return dist.get_backend()


def profile_traffic(kernel_substr, workload=None):
    """HBM bytes per launch of the dominant kernel from the committed PMC summary of this round (rocprofv3 --pmc FETCH_SIZE
    / WRITE_SIZE in separate passes; FETCH_SIZE doubled per the gfx950 note in guides/MI355X_MICROARCH.md).  None when no
    summary for this kernel is present -- PMC cannot be collected from inside the timed process."""
    import glob
    import re
    pat = "*_%s_pmc.txt" % workload if workload else "*_pmc.txt"        # (round 2 on: one summary per workload)
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", pat)), reverse=True):
        txt = open(path).read()
        if kernel_substr not in txt and kernel_substr.split("_kernel")[0] not in txt:
            continue
        f = re.search(r"FETCH_SIZE\s+n=\s*\d+\s+mean=([0-9.e+]+)", txt)
        w = re.search(r"WRITE_SIZE\s+n=\s*\d+\s+mean=([0-9.e+]+)", txt)
        if f and w:
            return {"bytes_per_launch": (2.0 * float(f.group(1)) + float(w.group(1))) * 1024.0, "source": os.path.basename(path),
                    "note": "FETCH_SIZE x2 (gfx950 under-count of wide coalesced reads) + WRITE_SIZE, KiB -> bytes"}
    return None


class TimedScore:
    """Wraps ops.score_topk_keys with HIP events on the launch stream (torch's current stream)."""

    def __init__(self):
        from pda_amd import ops
        self.fn = ops.score_topk_keys
        self.events = []
        self.enabled = False
        self.prune = False
        self.stats = {}

    def __call__(self, *a, **k):
        k = dict(k, prune=self.prune, stats=self.stats)
        if not self.enabled:
            return self.fn(*a, **k)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = self.fn(*a, **k)
        e.record()
        self.events.append((s, e))
        return out

    def mean_ms(self):
        return sum(s.elapsed_time(e) for s, e in self.events) / max(1, len(self.events))

    def spread(self):
        """min / median / 90th percentile of the timed calls: one mean cannot tell a slow box from a regression."""
        t = sorted(s.elapsed_time(e) for s, e in self.events)
        if not t:
            return None
        return {"min": t[0], "median": t[len(t) // 2], "p90": t[min(len(t) - 1, int(0.9 * len(t)))], "max": t[-1], "calls": len(t)}


def gpu_clocks():
    """What the box reports about itself (rocm-smi), best effort: a lease that runs 7 % slower should be visible as such."""
    import subprocess
    out = {}
    try:
        txt = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--showtemp"], capture_output=True, text=True, timeout=20).stdout
        for ln in txt.splitlines():
            l = ln.lower()
            if "gpu[0]" not in l:
                continue
            for key, tag in (("sclk", "sclk clock level"), ("mclk", "mclk clock level"), ("power_w", "socket graphics package power"), ("power_w", "average graphics package power"),
                             ("temp_hotspot_c", "temperature (sensor junction)")):
                if tag in l:
                    out[key] = ln.split(":")[-1].strip()
    except Exception as e:                       # noqa: BLE001 -- diagnostics only
        out["error"] = str(e)[:80]
    return out


def bench_reference_block_protocol(args, dev, workload):
    """What a maintainer who keeps MF/train_new_api.py and swaps only the model wrapper sees (INTEGRATION.md route 2):
    DatasetApi_Model.do_recommendation called exactly as evaluation.generator_Rec_result_fast calls it (MF/train_new_api.py:780-794)
    -- blocks of 2 048 user ids as a Python list (:703,724-726), items = list(range(I)) (:785), pos_pop an ndarray [I] (:788), the
    train mask as the (int64 [nnz, 2], [-inf] * nnz, shape) triple built once per set_evaluate_obj_pre (:730-739), the result
    fetched to the host as an int32 ndarray [2048, 50] (:792).  Everything do_recommendation does is inside the timed region: list
    -> device conversions, the COO -> CSR conversion, the sweep, the merge, the copy back."""
    import numpy as np
    from pda_amd import ops, parse, synthetic
    from pda_amd import train_new_api as t
    W = synthetic.make_workload(workload, dev)
    a = parse.parse_args(["--train", "s_condition", "--test", "s_condition", "--embed_size", str(W.d), "--batch_size", "2048", "--verbose", "0"])
    small = {"n_users": 64, "n_items": 64}              # (tables replaced below: no second 600 MB allocation)
    m = t.DatasetApi_Model(a, small, 2048, None, dev)
    m.Recommender.weights = {"user_embedding": W.U, "item_embedding": W.I}
    m.Recommender.n_users, m.Recommender.n_items, m.n_items = W.n_users, W.n_items, W.n_items
    Bu, nb = 2048, (8 if workload == "tiny" else 48)
    ip, ix = W.hist_indptr.cpu().numpy(), W.hist_indices.cpu().numpy()
    items = list(range(W.n_items))
    pop = W.pop_last.cpu().numpy()
    blocks = []
    for b in range(nb + 2):
        u0 = (b * 9973 * 7) % max(1, W.n_users - Bu)
        users = list(range(u0, u0 + Bu))
        lens = (ip[u0 + 1:u0 + Bu + 1] - ip[u0:u0 + Bu]).astype(np.int64)
        rows = np.repeat(np.arange(Bu, dtype=np.int64), lens)
        cols = ix[ip[u0]:ip[u0 + Bu]].astype(np.int64)
        index = np.stack([rows, cols], axis=1)
        blocks.append((users, (index, np.array([-np.inf] * len(rows)).astype(np.float32), np.array([Bu, W.n_items]).astype(np.int64))))
    for users, mask in blocks[:2]:
        m.do_recommendation(None, users, items, "condition", pop, mask)
    torch.cuda.synchronize()
    def epoch():
        """one pass over the blocks as the reference's loop makes it; the caller's own line :788 (a 200 000-entry Python list as a fancy
        index: a fresh ndarray per block) is timed inside the same loop, so that the library's share is a difference of like with like"""
        caller = 0.0
        t0 = time.perf_counter()
        for users, mask in blocks[2:]:
            ta = time.perf_counter()
            pp = pop[items]
            caller += time.perf_counter() - ta
            out_ = m.do_recommendation(None, users, items, "condition", pp, mask)
        return time.perf_counter() - t0, caller, out_

    dt, caller_s, out = epoch()
    assert out.shape == (Bu, 50) and out.dtype == np.int32
    caller_ms = caller_s / nb * 1e3
    # the next evaluation epoch: the reference hands over the SAME mask arrays (built once per set_evaluate_obj_pre) -- their CSRs are on the device
    torch.cuda.synchronize()
    dt_rep, caller_rep_s, out = epoch()
    # the kernels alone on the same blocks (device-resident inputs): what the host conversions cost on top
    hs = [ops.HistoryCSR.from_coo(mask[0], Bu, dev) for _, mask in blocks[2:]]
    us = [torch.as_tensor(np.asarray(users, dtype=np.int32), device=dev) for users, _ in blocks[2:]]
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for u, h in zip(us, hs):
        ops.recommend_topk(W.U, W.I, u, 50, ops.HEAD_POP, W.pop_last, h)
    torch.cuda.synchronize()
    dk = time.perf_counter() - t1
    # the raw head ('main_branch': evaluated in every epoch, the only head of --train normal) through the same call: no popularity vector, the same COO masks
    for users, mask in blocks[:2]:
        m.do_recommendation(None, users, items, "main_branch", None, mask)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    for users, mask in blocks[2:]:
        out_r = m.do_recommendation(None, users, items, "main_branch", None, mask)
    dt_raw = time.perf_counter() - t2
    st_r = {}
    ops.score_topk_keys(W.U, W.I, us[0], 50, ops.HEAD_RAW, None, hs[0], stats=st_r)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    for u, h in zip(us, hs):
        ops.recommend_topk(W.U, W.I, u, 50, ops.HEAD_RAW, None, h)
    torch.cuda.synchronize()
    dk_raw = time.perf_counter() - t3
    raw_blk = {"ms_per_block": dt_raw / nb * 1e3, "users_per_s": Bu * nb / dt_raw, "device_only_ms_per_block": dk_raw / nb * 1e3,
               "kernel_identity": ops.kernel_identity(st_r["kernel_id"][0]) if "kernel_id" in st_r else None,
               "note": "rec_type 'main_branch' through do_recommendation, masks by block row (the COO triple): the funnel from one 1 024-user tile on"}
    assert out_r.shape == (Bu, 50)
    fl = 2.0 * Bu * W.n_items * W.d
    return {"users_per_s": Bu * nb / dt, "ms_per_block": dt / nb * 1e3, "blocks": nb, "users_per_block": Bu, "raw_head": raw_blk,
            "roofline_frac": fl / (dt / nb) / 1e12 / PEAK_BF16_MFMA_TFLOPS,
            "device_only": {"users_per_s": Bu * nb / dk, "ms_per_block": dk / nb * 1e3, "roofline_frac": fl / (dk / nb) / 1e12 / PEAK_BF16_MFMA_TFLOPS},
            "nnz_per_block": int(np.mean([len(mk[0]) for _, mk in blocks])),
            "caller_pop_gather_ms": caller_ms,
            "library_ms_per_block": dt / nb * 1e3 - caller_ms,          # do_recommendation itself: conversions, COO -> CSR, sweep, merge, copy back
            "repeat_epoch": {"ms_per_block": dt_rep / nb * 1e3, "library_ms_per_block": (dt_rep - caller_rep_s) / nb * 1e3, "users_per_s": Bu * nb / dt_rep,
                             "note": "the same blocks again, as the reference's next evaluation epoch calls them: the mask arrays are the same objects, their CSRs are cached on the device"},
            "note": "DatasetApi_Model.do_recommendation called like MF/train_new_api.py:792: Python lists in, COO mask triple, int32 ndarray "
                    "out, blocking; product-default sweep (early-terminating); device_only = the same blocks with ids and CSR already in HBM; "
                    "caller_pop_gather_ms = testing_popularity[batch_item] of the reference's loop (:788), part of ms_per_block, not of this library"}



def table_dtype_of(args, workload):
    td = args.table_dtype if args.table_dtype != "auto" else ("bf16" if workload == "c5shard" else "f32")
    return td, (torch.bfloat16 if td == "bf16" else torch.float32)


def bench_eval(args, rank, world, dev, workload=None, light=False, user_groups=None):
    """light: the per_config form -- headline sweep and early-terminating sweep only, a third of the steps."""
    import torch.distributed as dist
    from pda_amd import ops, synthetic
    from pda_amd.dist import ItemShardedTopK
    workload = workload or args.workload
    td_name, td = table_dtype_of(args, workload)
    steps = max(2, args.steps // 3) if light else args.steps
    if world > 1 and os.environ.get("PDA_BENCH_ONE_GPU") == "1":
        # N processes on ONE GPU (the plumbing check of tests/test_gpu_two_rank.py): eight of them generating config 3 at the same time spend
        # minutes in the GPU's time slicing (measured: still inside make_workload after 120 s; four ranks: 27 s for the whole run) -- one at a time
        for r in range(world):
            if r == rank:
                W = synthetic.make_workload(workload, dev, table_dtype=td)
                torch.cuda.synchronize()
            dist.barrier()
    else:
        W = synthetic.make_workload(workload, dev, table_dtype=td)
    head = ops.HEAD_POP if args.head == "condition" else ops.HEAD_RAW
    timed = TimedScore()
    # N > 1: `ugroups` user groups x (world / ugroups) item shards (pda_amd.dist.grid_layout)
    from pda_amd.dist import default_user_groups, make_item_group
    ugroups = (user_groups or args.user_groups or default_user_groups(world)) if world > 1 else 1
    gidx, grank, gsize, pgroup = make_item_group(rank, world, ugroups) if world > 1 else (0, 0, 1, None)
    # N = 1: the score call is wrapped with HIP events (roofline.kernel_ms).  N > 1: the product's own path -- early-terminating
    # sweeps run software-pipelined (pda_amd.dist.topk_blocks: the seed collectives of block b + 1 under the sweep of block b),
    # which a per-call wrapper would serialise; kernel_ms is then the step time.
    ev = ItemShardedTopK.from_full_tables(W.U, W.I, W.pop_last, grank, gsize, group=pgroup, score_fn=timed if world == 1 else None)
    world_all, world = world, gsize                     # below, "world" is the item-shard group; world_all the whole job
    hist = ops.HistoryCSR(W.hist_indptr, W.hist_indices, by_user=True)
    Bu = min(args.eval_block, W.n_users)
    n_blocks = args.warmup + steps
    starts = [(b * Bu) % max(1, W.n_users - Bu + 1) for b in range(n_blocks)]
    if W.n_users > (1 << 23) + Bu:
        # the whole user table of config 5: the timed blocks come from the TOP of the id range -- user ids above 2^23, i.e. row offsets uid * d * 2
        # and CSR offsets indptr[uid] * 4 beyond 2^31 bytes in every gather of the timed region
        top_blocks = max(1, (W.n_users - (1 << 23)) // Bu)
        starts = [W.n_users - (1 + b % top_blocks) * Bu for b in range(n_blocks)]
    per_g = Bu // ugroups                               # this group's users of every step
    blocks = [torch.arange(s + gidx * per_g, s + (gidx + 1) * per_g if gidx < ugroups - 1 else s + Bu, dtype=torch.int32, device=dev) for s in starts]
    if world_all > 1:
        del W.I                                           # every rank keeps only its shard of the item table
    sink = []

    last = [None, None]
    last_spread = [None]

    def run(bl, hd):
        # N > 1: the all-to-all exchange -- every rank merges and keeps the lists of its slice of the users
        for idx, val in ev.topk_blocks(bl, args.K, hd, hist, sharded=world > 1):
            sink.append(idx[0, 0])                        # keep the result alive without a sync
            last[0], last[1] = idx, val

    def timed_pass(prune, hd=None):
        """W untimed + K timed steps, barrier + synchronize on both sides, MAX over ranks."""
        hd = head if hd is None else hd
        timed.prune, timed.enabled, timed.events, timed.stats = prune, False, [], {}
        ev.prune = prune
        run(blocks[:max(1, args.warmup)], hd)
        torch.cuda.synchronize()
        if world_all > 1:
            dist.barrier()
        torch.cuda.synchronize()
        timed.enabled = True
        t0 = time.perf_counter()
        run(blocks[args.warmup:], hd)
        torch.cuda.synchronize()
        if world_all > 1:
            dist.barrier()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if world_all > 1:
            t = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t[0])
        last_spread[0] = timed.spread()
        return dt, (timed.mean_ms() if timed.events else dt / steps * 1e3), dict(timed.stats)

    # headline: a DENSE sweep -- every user x item pair is scored.  With the PDA head the catalogue is visited most
    # popular first (early_stop = 0: nothing is skipped; the running thresholds just rise early, so far fewer
    # candidates reach the lists).  The natural-order dense sweep is reported beside it.
    v2 = ops.score_impl(W.d, args.K, W.n_items) == "v2"
    use_order = head == ops.HEAD_POP and v2
    natural = None
    if args.full and use_order and not args.headline_only and not light:
        dt_n, k_ms_n, _ = timed_pass(False)
        natural = {"value": Bu * steps / dt_n, "unit": "users/s", "ms_per_step": dt_n / steps * 1e3, "kernel_ms": k_ms_n}
    clocks_before = gpu_clocks() if (args.full and world_all == 1 and not light) else None
    dt, k_ms, st_d = timed_pass("order" if use_order else False)
    headline_spread = last_spread[0]
    outputs = {"idx": last[0], "val": last[1], "users": blocks[-1] if world_all == 1 else None}
    clocks_after = gpu_clocks() if (args.full and world_all == 1 and not light) else None
    if os.environ.get("PDA_BENCH_DUMP") and user_groups is None:      # (N > 1: the replicated-hot-items path of pda_amd.dist)
        torch.save(last[0].cpu(), os.path.join(os.environ["PDA_BENCH_DUMP"], "topk_dense_w%d_r%d.pt" % (world_all, rank)))
    if use_order and "tiles_scored" in st_d:
        # (generation 4 counts whole 64-item tiles and whole 128-user tiles: >= the 32-item count)
        assert int(st_d["tiles_scored"][0]) >= st_d["tiles_dense"], "the dense sweep must score every tile"
    # beside it: the product default for the PDA head -- ordered sweep WITH exact early termination (same keys).
    ordered = None
    if args.full and use_order and not args.headline_only:
        dt_o, k_ms_o, st = timed_pass(True)
        frac = float(st["tiles_scored"][0]) / st["tiles_dense"] if "tiles_scored" in st else None
        ordered = {"value": Bu * steps / dt_o, "unit": "users/s", "ms_per_step": dt_o / steps * 1e3,
                   "kernel_ms": k_ms_o, "item_tiles_scored_frac": frac,
                   "note": "pda_score_topk_ordered_f32: catalogue visited most-popular-first, a user block stops once "
                           "pop + ||u||*pop*||i|| of everything unvisited is below every user's running K-th value; "
                           "bit-identical keys (tests/test_gpu_score_topk.py); data-dependent, hence not the headline"}
    if os.environ.get("PDA_BENCH_DUMP") and user_groups is None:      # tests/test_gpu_two_rank.py: the lists of the last step (this rank's rows)
        torch.save(last[0].cpu(), os.path.join(os.environ["PDA_BENCH_DUMP"], "topk_w%d_r%d.pt" % (world_all, rank)))
    # the raw head ('main_branch'): the reference evaluates it in EVERY evaluation epoch before the two PDA passes
    # (MF/train_new_api.py:1139-1141, head at :597-598) and it is the only head of --train normal.  Product-default sweep mode.
    raw = None
    if args.full and head == ops.HEAD_POP and v2 and not args.headline_only and world_all == 1:
        rp = ops.prune_default(ops.HEAD_RAW, W.d)
        dt_r, k_ms_r, st_r = timed_pass(rp, ops.HEAD_RAW)
        fl_r = 2.0 * blocks[0].numel() * ev.I_shard.shape[0] * W.d
        ident_r = ops.kernel_identity(st_r["kernel_id"][0]) if "kernel_id" in st_r else {"generation": 0}
        funnel = ident_r.get("geometry") == "funnel"
        gen_r = ops.score_kernel(W.d, args.K, ev.I_shard.shape[0], rp, ops.HEAD_RAW)
        raw = {"value": Bu * steps / dt_r, "unit": "users/s", "ms_per_step": dt_r / steps * 1e3, "kernel_ms": k_ms_r, "kernel_ms_spread": last_spread[0],
               "roofline_frac": fl_r / (k_ms_r * 1e-3) / 1e12 / PEAK_BF16_MFMA_TFLOPS, "kernel_identity": ident_r,
               "kernel": ("the funnel: sweep7_kernel<%d,%s> (emitting sweeps, fixed thresholds) + expand7 / threshold7 (bound-keyed pools) + resolve7 (one exact rescoring)"
                          % (W.d, td_name)) if funnel else "%s<%d,RAW,%s>" % ("sweep4_kernel" if gen_r == "v4" else "score_topk_v3_kernel", W.d, td_name),
               "sweep": "growing parts of the catalogue in a random visiting order" if funnel else
                        {"order": "dense, items visited largest norm first", False: "dense, natural item order", True: "early-terminating"}[rp],
               "exact_rescorings_per_user": (float(st_r["pairs_rescored"][0]) / blocks[0].numel()) if "pairs_rescored" in st_r else None,
               "rows_through_the_exact_fallback": int(st_r["fallback_rows"][0]) if "fallback_rows" in st_r else None,
               "note": "rec_type 'main_branch' (top_k(R + M), MF/train_new_api.py:597-598): evaluated in EVERY epoch, the only head of --train normal; bit-exact fp32 "
                       "scores and lists vs the oracle (tests/test_gpu_funnel.py, test_full_size_c3); the whole call is timed (every launch of the funnel)"}
    n_local = ev.I_shard.shape[0]
    Bu_rank = blocks[0].numel()                           # users this rank scores per step (its group's share)
    flops = 2.0 * Bu_rank * n_local * W.d
    nnz_blk = float(W.n_train) * Bu_rank / W.n_users
    esz = 2 if td_name == "bf16" else 4
    abytes = n_local * W.d * esz + n_local * 4 + Bu_rank * W.d * esz + nnz_blk * 4 + (Bu_rank + 1) * 8 + Bu_rank * args.K * 8
    impl = ops.score_impl(W.d, args.K, W.n_items)
    hd = "POP" if head else "RAW"
    alg_tf = flops / (k_ms * 1e-3) / 1e12
    hbm = {"algorithmic_bytes_per_launch": abytes, "achieved_GBs": abytes / (k_ms * 1e-3) / 1e9,
           "peak_GBs": PEAK_HBM_GBS, "frac": abytes / (k_ms * 1e-3) / 1e9 / PEAK_HBM_GBS}
    if impl == "v2":
        # v2 = bf16x3 MFMA pre-filter (3 bf16 MFMAs per fp32 product) + exact fp32 rescoring of the survivors.
        # dense sweeps of fp32 tables run the v3 kernel: ONE bf16 MFMA per k-step as pre-filter (+ one k-step that carries
        # the threshold test), survivors rescored exactly in fp32.
        gen = ops.score_kernel(W.d, args.K, n_local, "order" if use_order else False)
        # which kernel the timed launches ran: decoded from the identity word the sweep kernel itself wrote into the workspace
        ident = ops.kernel_identity(st_d["kernel_id"]) if "kernel_id" in st_d else {"generation": 0}
        geo_name = ident.get("geometry") if ident.get("generation") == 4 else None
        huge = geo_name == "huge"
        kname = "sweep5_kernel" if huge else ("sweep4_kernel" if gen == "v4" else "score_topk_v3_kernel")
        geo = {"lds": "256 users per workgroup, lists in LDS (Geo4<D, 0>)", "many": "many candidates: 128 users per workgroup (Geo4<D, 3>)",
               "huge": "huge: 1 024 users per workgroup, four 512-register waves, user rows in AGPRs, transposed product on v_mfma_f32_16x16x32_bf16, "
                       "VALU threshold test (no test k-step), sorted hand-over from the warm-up (pda_v5_sweep.h, tools/gen_v6_loop_asm.py)"}.get(geo_name, "")
        if W.d == 256 and huge:
            geo = ("huge at d = 256: 512 users per workgroup (128 users per wave: 8 blocks x 8 k-steps fill the 256 AGPRs), one workgroup per CU, "
                   "transposed product on v_mfma_f32_16x16x32_bf16, VALU threshold test (Loop6<256, 8>, pda_v5_sweep.h)")
        elif W.d == 256:
            geo = "256 users per workgroup, lists in the workspace, 8 + 3 + 1 waves (Geo4<256, 0>)"
        bf_s = "true" if td_name == "bf16" else "false"
        if huge:
            ktemplate = "sweep5_kernel<%d, %s, true, %d>" % (W.d, bf_s, 128 if W.d == 256 else 256)
        elif gen == "v4":
            ktemplate = "sweep4_kernel<%d, %d, %s, %s, %d>" % (W.d, 1 if head else 0, bf_s, "true" if ident.get("early_stop") else "false",
                                                             {"lds": 0, "many": 3}.get(geo_name, 0))
        else:
            ktemplate = None
        ksteps_exec = (W.d / 16) if huge else (W.d / 16 + 1)       # the huge geometry has no folded test k-step
        roof = {"kernel": "%s<%d,%s,%s>%s" % (kname, W.d, hd, td_name, " visiting order, early_stop=0" if use_order else " natural order"),
                "kernel_template": ktemplate, "kernel_identity": ident,
                "geometry": geo,
                "bound": "mfma", "achieved": alg_tf,
                "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": alg_tf / PEAK_BF16_MFMA_TFLOPS,
                "traffic": profile_traffic(kname, workload if (world_all == 1 and Bu == 262144) else "none"), "kernel_ms": k_ms,
                "kernel_ms_spread": headline_spread, "box": {"before": clocks_before, "after": clocks_after},
                # N = 1: HIP events around every score call on its launch stream; N > 1: the pipelined multi-rank path is not wrapped
                # per call -- the figure is then WALL time per step (max over ranks), collectives included
                "kernel_ms_source": "hip_events_per_call" if world_all == 1 else "wall_time_per_step_max_over_ranks",
                "flops_per_launch": flops,
                # generation 4's folded threshold test is one more MFMA k-step per tile (d/16 + 1 instead of d/16): executed > algorithmic;
                # the huge geometry tests in the VALU shadow (executed = algorithmic + the re-scored flagged half-tiles, < 1 %)
                "executed": {"bf16_mfma_TFLOPs": alg_tf * ksteps_exec / (W.d / 16),
                             "frac_of_bf16_peak": alg_tf * ksteps_exec / (W.d / 16) / PEAK_BF16_MFMA_TFLOPS,
                             "note": "achieved/frac above count the algorithmic 2*users*items*d only"},
                "fp32_equivalent": {"peak": PEAK_F32_MFMA_TFLOPS, "frac": alg_tf / PEAK_F32_MFMA_TFLOPS,
                                    "note": "same bit-exact fp32 results as the fp32-MFMA kernel (v1), whose roof this is"},
                "hbm": hbm}
    else:
        roof = {"kernel": "score_topk_kernel<%d,%s>" % (W.d, hd), "bound": "mfma", "achieved": alg_tf,
                "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": alg_tf / PEAK_F32_MFMA_TFLOPS,
                "traffic": profile_traffic("score_topk_kernel"), "kernel_ms": k_ms, "flops_per_launch": flops, "hbm": hbm}
    # What one evaluation pass over ALL users costs right after a weight update: the item-side preparation (bf16 rows in
    # visiting order + test pieces + bounds; the visiting order and the reordered history depend on pop only and survive)
    # plus ceil(U / Bu) steps.
    prep = None
    if args.full and impl == "v2" and world_all == 1:
        pop_h = ev.pop_shard if head == ops.HEAD_POP else None
        order = ops.visiting_order(ev.I_shard, pop_h) if use_order else None
        def do_prep():
            ops.mark_modified(ev.I_shard)
            if gen == "v4":
                ops.item_prep4(ev.I_shard, pop_h, order)
            elif use_order:
                ops.item_prep_ordered(ev.I_shard, pop_h)
            else:
                ops.item_prep(ev.I_shard)
        do_prep()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            do_prep()
        e1.record()
        torch.cuda.synchronize()
        prep_ms = e0.elapsed_time(e1) / 5
        n_steps_all = -(-W.n_users // Bu)
        pass_ms = prep_ms + n_steps_all * dt / steps * 1e3
        prep = {"prep_ms": prep_ms, "steps_per_pass": n_steps_all, "pass_ms_incl_prep": pass_ms,
                "users_per_s_incl_prep": W.n_users / (pass_ms * 1e-3),
                "note": "one pass over all %d users after a weight update = item prep + %d steps of the headline sweep" % (W.n_users, n_steps_all)}
    res = {"users_per_s": Bu * steps / dt, "ms_per_step": dt / steps * 1e3, "Bu": Bu, "W": W, "steps": steps, "table_dtype": td_name,
           "layout": {"user_groups": ugroups, "item_shards": gsize, "users_per_rank_and_step": Bu_rank, "items_per_rank": n_local},
           "roofline": roof, "hist": hist, "ordered": ordered, "natural": natural, "prep": prep, "raw_head": raw, "outputs": outputs}
    return res


def timed_graph_steps(body, n_steps, B, G=64):
    """`body(i)` = one training step; G of them captured into a HIP graph, replayed n_steps / G times."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for i in range(3):
            body(i)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(G):
            body(i)
    reps = max(1, n_steps // G)
    g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        g.replay()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"triplets_per_s": reps * G * B / dt, "us_per_step": dt / (reps * G) * 1e6, "steps": reps * G}


def sgd_rates_on_tables(args, dev, W, Bs=(2048, 4096)):
    """SGD step throughput on the tables of workload W (pre-staged device-sampled batches, HIP graphs of 64 steps):
    the fused hogwild step and the planned exact step (pda_triplet_plan + pda_bpr_step_plan_*: two launches, no atomics; the plan
    is the sampler's work, batches ahead).  bf16 tables (config 5): forward on the bf16 rows, fp32 masters take the update, the
    touched bf16 rows are re-rounded -- by three pda_refresh_rows_bf16 launches behind the fused step, inside the two launches of
    the planned one."""
    from pda_amd import ops
    bf = W.U.dtype == torch.bfloat16
    regs, lr, NB = 1e-2, 1e-2, 64
    esz = 2 if bf else 4
    out = {"tables": "%s: %d + %d rows x %d, %s" % (W.name.upper(), W.n_users, W.n_items, W.d, "bf16 rows + fp32 masters" if bf else "fp32"),
           "bytes_per_triplet": 6 * W.d * esz + 20}
    loss = torch.zeros(3, device=dev)
    Bs = [B for B in Bs if B <= W.n_users]            # (distinct users inside a batch: the sampler contract the planned step relies on)
    if bf:
        U16, I16, Um, Im = W.U.clone(), W.I.clone(), W.U.float(), W.I.float()
    else:
        U, I = W.U.clone(), W.I.clone()
    for B in Bs:
        raw = [ops.sample_triplets(W.hist_indptr, W.hist_indices, B, seed=2022, step=s_, n_pool=W.n_users, train_slots=W.hist_slots,
                                   neg_range=(0, W.n_items), pop_matrix=W.pop_train) for s_ in range(NB)]
        plans = [ops.triplet_plan(b[0], b[1], b[2])[0] for b in raw]
        sc = [None]
        if bf:
            fused = lambda i: ops.bpr_step_bf16(U16, I16, *raw[i % NB], regs=regs, reg_div=B, lr=lr, mode=ops.UPD_SGD_FUSED, U_master=Um, I_master=Im, loss_acc=loss)

            def planned(i):
                sc[0] = ops.bpr_step_plan(U16, I16, *raw[i % NB], regs=regs, reg_div=B, lr=lr, plan=plans[i % NB], scratch=sc[0], loss_acc=loss, U_master=Um, I_master=Im)
        else:
            fused = lambda i: ops.bpr_step(U, I, *raw[i % NB], regs=regs, reg_div=B, lr=lr, mode=ops.UPD_SGD_FUSED, loss_acc=loss)

            def planned(i):
                sc[0] = ops.bpr_step_plan(U, I, *raw[i % NB], regs=regs, reg_div=B, lr=lr, plan=plans[i % NB], scratch=sc[0], loss_acc=loss)
        r = {"fused_hogwild": timed_graph_steps(fused, args.train_steps, B), "exact_planned": timed_graph_steps(planned, args.train_steps, B)}
        for v in r.values():
            v["hbm_frac"] = v["triplets_per_s"] * out["bytes_per_triplet"] / 1e9 / PEAK_HBM_GBS
        out["B%d" % B] = r
    return out


def bench_train(args, dev, workload=None, quick=False):
    """Fused BPR step on BASELINE config 2 (50k x 20k, d=64, B=2048, PD/PDA s_condition), batches pre-staged in HBM
    by the device sampler; steps captured into HIP graphs of 64 launches (launch-bound regime).  quick: the per_config
    form (pre-staged fused SGD, reference-faithful Adam, one-launch step + sampler)."""
    from pda_amd import ops, synthetic
    W = synthetic.make_workload(workload or ("c2" if args.workload != "tiny" else "tiny"), dev)
    B, regs, lr, NB, G = 2048, 1e-2, 1e-2, 64, 64
    # pre-staged batches, grouped by positive item (pda_group_triplets_by_pos): the step kernel then combines whole runs
    batches = [ops.sample_triplets(W.hist_indptr, W.hist_indices, B, seed=2020, step=s, n_pool=W.n_users,
                                   train_slots=W.hist_slots, neg_range=(0, W.n_items), pop_matrix=W.pop_train, sort_by_pos=True)
               for s in range(NB)]
    out = {"workload": "%s: synthetic %d users x %d items, d=%d, B=%d, PD/PDA (s_condition, gamma=%.2f)" %
                       (W.name.upper(), W.n_users, W.n_items, W.d, B, W.gamma), "graph_launches": G}

    timed_graph = lambda body, n_steps: timed_graph_steps(body, n_steps, B, G)

    U, I = W.U.clone(), W.I.clone()
    loss = torch.zeros(3, device=dev)
    # (users are distinct inside a batch -- the sampler contract, B <= n_users --: their rows take plain stores)
    out["sgd_fused"] = timed_graph(lambda i: ops.bpr_step(U, I, *batches[i % NB], regs=regs, reg_div=B, lr=lr, mode=ops.UPD_SGD_FUSED,
                                                          loss_acc=loss, grouped=True, users_distinct=B <= W.n_users), args.train_steps)
    U, I = W.U.clone(), W.I.clone()
    out["sgd_fused_atomic_user_rows"] = timed_graph(lambda i: ops.bpr_step(U, I, *batches[i % NB], regs=regs, reg_div=B, lr=lr,
                                                                            mode=ops.UPD_SGD_FUSED, loss_acc=loss, grouped=True), args.train_steps)
    U, I = W.U.clone(), W.I.clone()
    raw_batches = [ops.sample_triplets(W.hist_indptr, W.hist_indices, B, seed=2020, step=s_, n_pool=W.n_users,
                                       train_slots=W.hist_slots, neg_range=(0, W.n_items), pop_matrix=W.pop_train, sort_by_pos=False)
                   for s_ in range(NB)]
    out["sgd_fused_batches_in_sampling_order"] = timed_graph(
        lambda i: ops.bpr_step(U, I, *raw_batches[i % NB], regs=regs, reg_div=B, lr=lr, mode=ops.UPD_SGD_FUSED, loss_acc=loss),
        args.train_steps)
    out["sgd_fused"]["bytes_per_triplet"] = 6 * W.d * 4 + 20
    out["sgd_fused"]["hbm_frac"] = out["sgd_fused"]["triplets_per_s"] * (6 * W.d * 4 + 20) / 1e9 / PEAK_HBM_GBS

    # the EXACT mini-batch step without atomics: plan (the sampler's work, batches ahead) + two launches; and the planned one-launch step
    U, I = W.U.clone(), W.I.clone()
    plans_raw = [ops.triplet_plan(b[0], b[1], b[2])[0] for b in raw_batches]
    sc = [None]

    def planned(i):
        sc[0] = ops.bpr_step_plan(U, I, *raw_batches[i % NB], regs=regs, reg_div=B, lr=lr, plan=plans_raw[i % NB], scratch=sc[0], loss_acc=loss)
    out["sgd_exact_planned"] = timed_graph(planned, args.train_steps)
    out["sgd_exact_planned"]["note"] = ("pda_triplet_plan (pre-staged with the batch) + pda_bpr_step_plan_f32: launch A per triplet (user rows by plain "
                                        "stores), launch B per distinct item row (segment sums in plan order): exact 'sum then apply', bit-reproducible, no atomics")
    out["sgd_exact_planned"]["hbm_frac"] = out["sgd_exact_planned"]["triplets_per_s"] * (6 * W.d * 4 + 20) / 1e9 / PEAK_HBM_GBS
    U, I = W.U.clone(), W.I.clone()
    out["sgd_planned_one_launch"] = timed_graph(lambda i: ops.bpr_step_plan(U, I, *raw_batches[i % NB], regs=regs, reg_div=B, lr=lr, plan=plans_raw[i % NB],
                                                                             exact=False, loss_acc=loss), args.train_steps)
    out["sgd_planned_one_launch"]["note"] = "plain stores on user rows and once-referenced item rows, atomics on shared item rows only (hogwild there)"
    U, I = W.U.clone(), W.I.clone()
    sc0 = [None]

    def old_exact(i):
        sc0[0] = ops.sgd_step_exact(U, I, *raw_batches[i % NB], regs=regs, reg_div=B, lr=lr, loss_acc=loss, scratch=sc0[0])
    out["sgd_exact_two_launch_atomics"] = timed_graph(old_exact, max(256, args.train_steps // 2))

    U, I = W.U.clone(), W.I.clone()
    st = [torch.zeros_like(t) for t in (U, U, U, I, I, I)]   # mU vU gU mI vI gI
    tcount = [0]

    def adam_body(i):
        tcount[0] += 1
        lr_t = ops.adam_lr_t(lr, min(tcount[0], 1000))       # host scalar frozen in the graph: fine for timing
        ops.bpr_step(U, I, *batches[i % NB], regs=regs, reg_div=B, mode=ops.UPD_DENSE_GRAD, gU=st[2], gI=st[5], loss_acc=loss)
        bt = batches[i % NB]
        ops.adam_mark_rows(bt[0], bt[1], bt[2], tbits[0], tbits[1])          # six streams: the gradient tables are read on the batch's rows only
        ops.adam_dense_sweep3(U, st[0], st[1], st[2], tbits[0], I, st[3], st[4], st[5], tbits[1], lr_t)
    tbits = ops.adam_touched_bitmaps(W.n_users, W.n_items, dev)
    out["adam_dense_five_launches"] = timed_graph(adam_body, max(256, args.train_steps // 4))
    out["adam_dense_five_launches"]["note"] = "round 5's step: pda_bpr_step_f32(DENSE_GRAD) + pda_adam_mark_rows + pda_adam_dense_sweep3_f32 (non-temporal streams) + two memsets"
    # round 6: the step in two launches (row tags written by the step kernel, the sweep out of the Infinity Cache while the tables fit it)
    U, I = W.U.clone(), W.I.clone()
    st = [torch.zeros_like(t) for t in (U, U, U, I, I, I)]
    tags = ops.adam_row_tags(W.n_users, W.n_items, dev)
    tcount[0] = 0

    def adam_step_body(i):
        tcount[0] += 1
        ops.adam_step(U, st[0], st[1], st[2], tags[0], I, st[3], st[4], st[5], tags[1], *batches[i % NB], regs=regs, reg_div=B, step=tcount[0],
                      lr_t=ops.adam_lr_t(lr, min(tcount[0], 1000)), grouped=True, users_distinct=B <= W.n_users, loss_acc=loss)
    out["adam_dense_reference_faithful"] = timed_graph(adam_step_body, max(256, args.train_steps // 4))
    out["adam_dense_reference_faithful"]["note"] = ("pda_adam_step_f32, policy by working set: %s" %
                                                    ("resident (plain accesses: the tables stay in the Infinity Cache)" if 3 * (W.n_users + W.n_items) * W.d * 4 <= (160 << 20) else
                                                     "streaming (non-temporal)") + "; two launches: bpr_step_kernel (gradients + row tags) + adam_dense_sweep4_kernel")
    sweep_bytes = 6 * (W.n_users + W.n_items) * W.d * 4
    r = out["adam_dense_reference_faithful"]
    r["algorithmic_bytes_per_step"] = sweep_bytes
    r["hbm_frac"] = sweep_bytes / (r["us_per_step"] * 1e-6) / 1e9 / PEAK_HBM_GBS

    # the whole loop on the device: one launch per `chunk` steps, a fresh device-sampled batch every step
    def loop_one_launch(Bl, chunk, n_chunks):
        U, I = W.U.clone(), W.I.clone()
        mk = lambda: (torch.empty(Bl, dtype=torch.int32, device=dev), torch.empty(Bl, dtype=torch.int32, device=dev),
                      torch.empty(Bl, dtype=torch.int32, device=dev), torch.empty(Bl, device=dev), torch.empty(Bl, device=dev))
        bufs = [mk(), mk()]
        ctr = torch.tensor([1], dtype=torch.int64, device=dev)
        kw = dict(n_pool=W.n_users, train_slots=W.hist_slots, neg_range=(0, W.n_items), pop_matrix=W.pop_train)
        ops.sample_triplets_into(bufs[1], W.hist_indptr, W.hist_indices, seed=7, step_dev=ctr, advance=False, **kw)
        ops.sample_triplets_into(bufs[0], W.hist_indptr, W.hist_indices, seed=7, step_dev=ctr, **kw)
        ws = torch.zeros(2, dtype=torch.int32, device=dev)

        def go():
            ops.bpr_train_steps(U, I, bufs, chunk, regs=regs, reg_div=Bl, lr=lr, train_indptr=W.hist_indptr, train_indices=W.hist_indices,
                                seed=7, step_ctr=ctr, loss_acc=loss, barrier_ws=ws, **kw)
        go()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_chunks):
            go()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert int(ws[1]) == 0, "the training loop kernel was not resident as a whole"
        n = chunk * n_chunks
        return {"triplets_per_s": n * Bl / dt, "us_per_step": dt / n * 1e6, "steps": n, "steps_per_launch": chunk, "B": Bl}
    chunk = 256 if W.name != "tiny" else 32          # (even: the buffer sets are back in place after every launch)
    out["sgd_fused_loop_one_launch"] = loop_one_launch(B, chunk, max(2, args.train_steps // chunk))
    out["sgd_fused_loop_one_launch"]["note"] = ("pda_bpr_train_steps_f32: a resident grid loops over the steps, the sampler one batch ahead, a "
                                                 "grid barrier between steps; fresh batch every step")
    out["sgd_fused_loop_one_launch"]["hbm_frac"] = out["sgd_fused_loop_one_launch"]["triplets_per_s"] * (6 * W.d * 4 + 20) / 1e9 / PEAK_HBM_GBS
    if quick:
        return out, W, batches
    U, I = W.U.clone(), W.I.clone()
    stepc = [0]

    def sampled_body(i):
        stepc[0] += 1
        b = ops.sample_triplets(W.hist_indptr, W.hist_indices, B, seed=7, step=stepc[0], n_pool=W.n_users,
                                train_slots=W.hist_slots, neg_range=(0, W.n_items), pop_matrix=W.pop_train)
        ops.bpr_step(U, I, *b, regs=regs, reg_div=B, lr=lr, mode=ops.UPD_SGD_FUSED, loss_acc=loss)
    torch.cuda.synchronize()
    for i in range(8):
        sampled_body(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = max(256, args.train_steps // 4)
    for i in range(n):
        sampled_body(i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out["sgd_fused_with_device_sampler_eager"] = {"triplets_per_s": n * B / dt, "us_per_step": dt / n * 1e6, "steps": n}

    # the same pipeline (sample -> sort by positive -> fused step) captured in HIP graphs: the batch counter lives in
    # device memory (pda_sample_triplets_dev + pda_counter_add), so every replayed step draws a NEW batch
    U, I = W.U.clone(), W.I.clone()
    step_dev = torch.zeros(2, dtype=torch.int64, device=dev)    # two slots: the sampler hands the counter on itself
    bufs = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
            torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float32, device=dev),
            torch.empty(B, dtype=torch.float32, device=dev))

    def graph_sampled_body(i):
        ops.sample_triplets_into(bufs, W.hist_indptr, W.hist_indices, seed=7, step_dev=step_dev, n_pool=W.n_users,
                                 train_slots=W.hist_slots, neg_range=(0, W.n_items), pop_matrix=W.pop_train, parity=i & 1)
        ops.bpr_step(U, I, *bufs, regs=regs, reg_div=B, lr=lr, mode=ops.UPD_SGD_FUSED, loss_acc=loss)
    out["sgd_fused_with_device_sampler_graph"] = timed_graph(graph_sampled_body, max(256, args.train_steps // 2))
    out["sgd_fused_with_device_sampler_graph"]["batches_drawn"] = int(step_dev.max().item())

    # one launch per step: the step on batch t, the sampler of batch t + 1 in spare workgroups of the same kernel
    # (pda_bpr_step_sample_f32) -- two sets of batch buffers, a new batch every replayed step
    U, I = W.U.clone(), W.I.clone()
    step_dev2 = torch.zeros(2, dtype=torch.int64, device=dev)
    mk = lambda: (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                  torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float32, device=dev),
                  torch.empty(B, dtype=torch.float32, device=dev))
    two = [mk(), mk()]
    skw = dict(n_pool=W.n_users, train_slots=W.hist_slots, neg_range=(0, W.n_items), pop_matrix=W.pop_train)
    ops.sample_triplets_into(two[0], W.hist_indptr, W.hist_indices, seed=7, step_dev=step_dev2, parity=0, **skw)

    def fused_sampled_body(i):
        ops.bpr_step_and_sample(U, I, *two[i & 1], regs=regs, reg_div=B, lr=lr, next_out=two[(i + 1) & 1], train_indptr=W.hist_indptr,
                                train_indices=W.hist_indices, seed=7, step_dev=step_dev2, parity=(i + 1) & 1, loss_acc=loss, **skw)
    out["sgd_fused_step_and_next_batch_sampler_one_launch_graph"] = timed_graph(fused_sampled_body, max(256, args.train_steps // 2))
    out["sgd_fused_step_and_next_batch_sampler_one_launch_graph"]["batches_drawn"] = int(step_dev2.max().item())

    # the sampler MANY batches ahead (the reference's generator thread fills a queue): one launch draws and groups 32 batches,
    # 32 step launches consume them -- a fresh batch every step, grouped by positive item, at the price of two launches per 32
    U, I = W.U.clone(), W.I.clone()
    AH = 32
    step_dev3 = torch.zeros(2, dtype=torch.int64, device=dev)
    many = (torch.empty((AH, B), dtype=torch.int32, device=dev), torch.empty((AH, B), dtype=torch.int32, device=dev),
            torch.empty((AH, B), dtype=torch.int32, device=dev), torch.empty((AH, B), dtype=torch.float32, device=dev),
            torch.empty((AH, B), dtype=torch.float32, device=dev))
    calls = [0]

    def ahead_body(i):
        if i % AH == 0:
            ops.sample_batches_into(many, W.hist_indptr, W.hist_indices, seed=7, step_dev=step_dev3, parity=calls[0] & 1, group_by_pos=True, **skw)
            calls[0] += 1
        j = i % AH
        ops.bpr_step(U, I, many[0][j], many[1][j], many[2][j], many[3][j], many[4][j], regs=regs, reg_div=B, lr=lr, mode=ops.UPD_SGD_FUSED,
                     loss_acc=loss, grouped=True)
    out["sgd_fused_sampler_32_batches_ahead_graph"] = timed_graph(ahead_body, max(256, args.train_steps // 2))
    out["sgd_fused_sampler_32_batches_ahead_graph"]["batches_drawn"] = int(step_dev3.max().item())
    out["sgd_fused_sampler_32_batches_ahead_graph"]["note"] = ("pda_sample_batches_dev: one launch draws (and groups by positive item) the next 32 "
                                                              "batches, bit for bit the per-step sampler's; 32 step launches consume them")

    # the same with the EXACT step: one more launch per 32 batches plans them (pda_triplet_plan), two launches per step
    U, I = W.U.clone(), W.I.clone()
    step_dev4 = torch.zeros(2, dtype=torch.int64, device=dev)
    many2 = tuple(torch.empty_like(t) for t in many)
    plans32 = torch.empty((AH, _lib_plan_bytes(B)), dtype=torch.uint8, device=dev)
    calls2, sc2 = [0], [None]

    def ahead_exact_body(i):
        if i % AH == 0:
            ops.sample_batches_into(many2, W.hist_indptr, W.hist_indices, seed=7, step_dev=step_dev4, parity=calls2[0] & 1, group_by_pos=False, **skw)
            ops.triplet_plan(many2[0], many2[1], many2[2], out=plans32)
            calls2[0] += 1
        j = i % AH
        sc2[0] = ops.bpr_step_plan(U, I, many2[0][j], many2[1][j], many2[2][j], many2[3][j], many2[4][j], regs=regs, reg_div=B, lr=lr, plan=plans32[j],
                                   scratch=sc2[0], loss_acc=loss)
    out["sgd_exact_planned_sampler_32_batches_ahead_graph"] = timed_graph(ahead_exact_body, max(256, args.train_steps // 2))
    out["sgd_exact_planned_sampler_32_batches_ahead_graph"]["batches_drawn"] = int(step_dev4.max().item())
    return out, W, batches


def _lib_plan_bytes(B):
    from pda_amd import _lib
    return _lib.load().pda_triplet_plan_bytes(B)


def bench_adam_big_tables(args, dev, workload):
    """The reference's optimiser (TF-1.14 Adam, dense decay) on the HEADLINE workload's tables, B = 2048: one sweep over both
    tables per step vs the same arithmetic without the sweep (pda_adam_lazy_f32: idle rows replay their decay when next
    needed).  Eager launches, the step counter advancing (a captured graph would freeze it); 512 distinct device-sampled
    batches, so a user row comes back after ~n_users / B steps as in training; the final sync is timed separately."""
    from pda_amd import ops, synthetic
    W = synthetic.make_workload(workload, dev)
    B, regs, lr = 2048, 1e-2, 1e-2
    NBt = 512 if workload != "tiny" else 32
    batches = [ops.sample_triplets(W.hist_indptr, W.hist_indices, B, seed=2021, step=s, n_pool=W.n_users, train_slots=W.hist_slots,
                                   neg_range=(0, W.n_items), pop_matrix=W.pop_train) for s in range(NBt)]
    out = {"workload": "%s tables (%d + %d rows x %d), B=%d" % (W.name.upper(), W.n_users, W.n_items, W.d, B)}
    loss = torch.zeros(3, device=dev)
    z = torch.zeros_like

    def run(lazy, steps, fast=False, six=True):
        U, I = W.U.float().clone(), W.I.float().clone()
        st = [z(U), z(U), z(U), z(I), z(I), z(I)]
        tb = ops.adam_touched_bitmaps(W.n_users, W.n_items, dev)
        lz = ops.LazyAdamState(W.n_users, W.n_items, lr, dev, fast=fast) if lazy else None
        t = 0

        def step():
            nonlocal t
            t += 1
            b = batches[(t - 1) % NBt]
            if lazy:
                ops.adam_lazy(0, lz, U, st[0], st[1], st[2], I, st[3], st[4], st[5], b[0], b[1], b[2], t)
            ops.bpr_step(U, I, *b, regs=regs, reg_div=B, mode=ops.UPD_DENSE_GRAD, gU=st[2], gI=st[5], loss_acc=loss)
            if lazy:
                ops.adam_lazy(1, lz, U, st[0], st[1], st[2], I, st[3], st[4], st[5], b[0], b[1], b[2], t)
            elif six:
                ops.adam_mark_rows(b[0], b[1], b[2], tb[0], tb[1])
                ops.adam_dense_sweep3(U, st[0], st[1], st[2], tb[0], I, st[3], st[4], st[5], tb[1], ops.adam_lr_t(lr, t))
            else:
                ops.adam_dense_sweep2(U, st[0], st[1], st[2], I, st[3], st[4], st[5], ops.adam_lr_t(lr, t))
        for _ in range(8):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        r = {"triplets_per_s": steps * B / dt, "us_per_step": dt / steps * 1e6, "steps": steps}
        if lazy:
            t1 = time.perf_counter()
            ops.adam_lazy_sync(lz, U, st[0], st[1], I, st[3], st[4], t)
            torch.cuda.synchronize()
            r["final_sync_ms"] = (time.perf_counter() - t1) * 1e3
        return r
    out["dense_sweep"] = run(False, 24 if workload != "tiny" else 8)
    sweep_bytes = 6 * (W.n_users + W.n_items) * W.d * 4
    out["dense_sweep"]["algorithmic_bytes_per_step"] = sweep_bytes
    out["dense_sweep"]["hbm_frac"] = sweep_bytes / (out["dense_sweep"]["us_per_step"] * 1e-6) / 1e9 / PEAK_HBM_GBS
    out["dense_sweep"]["kernel"] = "adam_mark_rows_kernel + adam_dense_sweep3_kernel: six streams (x, m, v read and written; the gradient tables only on the batch's rows)"
    out["dense_sweep_seven_streams"] = run(False, 24 if workload != "tiny" else 8, six=False)     # pda_adam_dense_sweep2_f32: reads the dense gradient tables too
    out["replay"] = run(True, 1536 if workload != "tiny" else 64)
    out["replay"]["note"] = ("pda_adam_lazy_f32: bit-identical tables after the sync (tests/test_gpu_bpr_step.py); three launches per step, "
                             "traffic = the batch rows")
    # the same three launches per step captured in HIP graphs of 64 steps: the step counter lives in device memory
    # (pda_adam_lazy_dev_f32), so a replayed graph advances the optimiser and the host is out of the loop
    def run_graph(fast, steps):
        U, I = W.U.float().clone(), W.I.float().clone()
        st = [z(U), z(U), z(U), z(I), z(I), z(I)]
        lz = ops.LazyAdamState(W.n_users, W.n_items, lr, dev, fast=fast)
        t_dev = torch.tensor([1, 0], dtype=torch.int32, device=dev)
        n_tab = steps + 4 * 64 + 8
        lz.rates(n_tab)

        calls = [0]                                  # (the counter slots alternate with every step enqueued, warm-up steps included)

        def body(i):
            b = batches[i % NBt]
            par = calls[0] & 1
            calls[0] += 1
            ops.adam_lazy_dev(0, lz, U, st[0], st[1], st[2], I, st[3], st[4], st[5], b[0], b[1], b[2], t_dev, par, n_tab)
            ops.bpr_step(U, I, *b, regs=regs, reg_div=B, mode=ops.UPD_DENSE_GRAD, gU=st[2], gI=st[5], loss_acc=loss)
            ops.adam_lazy_dev(1, lz, U, st[0], st[1], st[2], I, st[3], st[4], st[5], b[0], b[1], b[2], t_dev, par, n_tab)
        r = timed_graph_steps(body, steps, B)
        r["steps_taken_on_device"] = int(t_dev.max().item()) - 1
        return r
    out["replay_fast_graph"] = run_graph(True, 1536 if workload != "tiny" else 128)
    out["replay_fast_graph"]["note"] = "the three launches of a step in HIP graphs of 64 steps, the step counter in device memory (pda_adam_lazy_dev_f32)"
    out["replay_fast"] = run(True, 1536 if workload != "tiny" else 64, fast=True)
    out["replay_fast"]["note"] = ("PDA_ADAM_REPLAY_FAST (--adam_sweep replay_fast, an explicit opt-in; the default above 64 MB of tables is the bit-identical replay): the same catch-up to 1e-6 on x instead of bit "
                                  "for bit -- running sqrt, hardware reciprocal, closed-form powers for m and v")
    return out


def bench_train_sharded(args, rank, world, dev):
    """Item-parallel SGD on BASELINE config 2 across `world` ranks: global batch 2048, B_local = 2048 / world, positives
    and negatives inside the rank's item slice, ONE all-gather of (user grads, ids, loss shares) per step."""
    import torch.distributed as dist
    from pda_amd import synthetic
    from pda_amd.dist import ItemShardedBPR, ShardSampler, shard_range
    W = synthetic.make_workload("c2" if args.workload != "tiny" else "tiny", dev)
    Bg = 2048 if args.workload != "tiny" else 512
    Bl, NB, steps = Bg // world, 32, 256
    lo, hi = shard_range(W.n_items, rank, world)
    tr = ItemShardedBPR(W.U, W.I[lo:hi].clone(), lo, regs=1e-2, lr=1e-2, global_batch=Bg, rank=rank, world=world)
    smp = ShardSampler(W.hist_indptr, W.hist_indices, lo, hi, Bl, seed=2020, rank=rank, train_slots=W.hist_slots,
                       pop_matrix=W.pop_train)
    batches = [smp(s) for s in range(NB)]
    for b in batches[:4]:
        tr.step(*b)
    torch.cuda.synchronize()
    dist.barrier()
    t0 = time.perf_counter()
    for s_ in range(steps):
        loss = tr.step(*batches[s_ % NB])
    torch.cuda.synchronize()
    dist.barrier()
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t[0])
    return {"triplets_per_s": Bg * steps / dt, "us_per_step": dt / steps * 1e6, "global_batch": Bg, "steps": steps,
            "exchange_bytes_per_rank_per_step": Bl * (W.d + 4) * 4, "last_loss": float(loss[0]),
            "note": "eager; one all_gather_into_tensor per step; strong scaling of one 2048-triplet step"}


def cli_epoch(cpu_entry):
    """python -m pda_amd.train_new_api on the Douban-shaped synthetic (tools/cli_epoch.py: three epochs, an evaluation after each): the
    wall-clock the reference itself prints (`Epoch %d [%.1fs]`, MF/train_new_api.py:1110), sampler + 3 371 steps of the reference's optimiser
    + the three evaluation heads -- the drop-in number."""
    import subprocess
    root = os.path.dirname(os.path.abspath(__file__))
    try:
        p = subprocess.run([sys.executable, os.path.join(root, "tools", "cli_epoch.py"), "--epochs", "3"], capture_output=True, text=True, timeout=600, cwd=root)
        line = [l for l in p.stdout.splitlines() if l.startswith("{")]
        if p.returncode != 0 or not line:
            return {"error": (p.stderr or p.stdout)[-400:]}
        r = json.loads(line[-1])
    except Exception as e:              # noqa: BLE001 -- a figure beside the headline must not take the line down
        return {"error": repr(e)[:400]}
    out = {k: r[k] for k in ("shape", "epoch_s", "train_epoch_s", "eval_epoch_s", "epoch_print_s", "steps_per_epoch", "us_per_step_through_the_cli", "main_wall_s") if k in r}
    out["cli"] = "python -m pda_amd.train_new_api --train s_condition --test s_condition --batch_size 2048 --log_interval 1 (adam, device sampler)"
    out["us_per_step_through_the_cli"] = r["train_epoch_s"] / r["steps_per_epoch"] * 1e6 if r.get("train_epoch_s") else None
    tr = (cpu_entry or {}).get("train") if isinstance(cpu_entry, dict) else None
    if tr and tr.get("value"):
        out["cpu_restatement_epoch_s"] = r["steps_per_epoch"] * 2048 / tr["value"]
        out["cpu_restatement_note"] = "steps_per_epoch x 2048 / cpu_baseline.train (torch-CPU restatement of the reference's train step on the C2 tables, dense-decay Adam, this box's host threads)"
    return out


def cpu_baseline(args, ev_res, train_pack, budget=None, full=True):
    """Reference op sequence on the host cores (torch CPU fp32), bounded sample.  kind = "port".  Protocol of BASELINE.md
    section 3: 3 warm-up blocks, median of up to 10 timed 2048-user blocks (fewer if the budget runs out).
    full: also the single-thread figure, the native top-K variant and the training port."""
    from oracle import cpu_baseline as cb
    budget = budget or args.cpu_budget
    W = ev_res["W"]
    # The threads that can actually run: the container's CPU quota, not the machine's logical CPUs (the GPU boxes of round 3 show
    # 256 logical CPUs under a cgroup quota of 16 -- 128 threads there are 16 cores' worth of time, throttled).
    logical = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q = open("/sys/fs/cgroup/cpu.max").read().split()
        if q[0] != "max":
            quota = float(q[0]) / float(q[1])
    except (OSError, ValueError, IndexError):
        try:
            qq, pp = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read()), int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            quota = qq / pp if qq > 0 else None
        except (OSError, ValueError):
            quota = None
    cores = max(1, min(torch.get_num_threads(), logical, int(quota + 0.5) if quota else logical))
    torch.set_num_threads(cores)
    try:
        import ctypes as _C0
        _C0.CDLL("libgomp.so.1").omp_set_num_threads(cores)
    except OSError:
        pass
    U, pop = W.U.float().cpu(), W.pop_last.cpu()
    I = W.I.float().cpu()
    indptr, indices = W.hist_indptr.cpu(), W.hist_indices.cpu()
    blocks, coos = [], []
    for b in range(13):
        s = (b * 2048) % max(1, W.n_users - 2048)
        users = torch.arange(s, min(s + 2048, W.n_users))
        lo, hi = int(indptr[users[0]]), int(indptr[users[-1] + 1])
        lens = (indptr[users + 1] - indptr[users])
        rows = torch.repeat_interleave(torch.arange(users.numel()), lens)
        blocks.append(users)
        coos.append((rows, indices[lo:hi].long()))
    rec = "condition" if args.head == "condition" else "main_branch"
    # value: the native C / OpenMP port (oracle/pda_cpu_port.c: fused, AVX2 + FMA, cache-blocked, heap top-K, all host threads) --
    # the path written for host cores.  Beside it the torch restatement of the TF op sequence in three threadings.
    rate, n = cb.time_eval(U, I, pop, blocks, coos, args.K, rec, budget_s=budget * 0.5, block_fn=cb.eval_block_native)
    cpu_model = "unknown"
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                cpu_model = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    out = {"value": rate, "unit": "users/s", "cores": cores, "kind": "port", "cpu_model": cpu_model,
           "host_logical_cpus": logical, "cgroup_cpu_quota": quota,
           "protocol": "3 warm-up blocks, median of the timed 2048-user blocks (up to 10, bounded by the budget)",
           "sample": "%d users in 2048-user reference blocks x full %d-item catalogue, d=%d; C / OpenMP port of the path "
                     "(oracle/pda_cpu_port.c: fused score + head + mask + heap top-K, AVX2 + FMA, 32 users x 4 items cache blocks) on "
                     "%d host threads; NOT TensorFlow itself (TF 1.14 cannot be installed here)" % (n, W.n_items, W.d, cores)}
    if not full:
        return out
    rate_b, n_b = cb.time_eval(U, I, pop, blocks, coos, args.K, rec, budget_s=budget * 0.4, block_fn=cb.eval_block_blocked)
    out["torch_op_sequence_blocked"] = {"value": rate_b, "unit": "users/s", "users": n_b, "threads": cores,
                                        "what": "torch-CPU restatement of the TF op sequence (matmul, elu+1, *pop, scatter -inf, topk) on 64-row x "
                                                "16 384-item pieces over the host threads, the K best of the pieces' candidates at the end"}
    rate_i, n_i = cb.time_eval(U, I, pop, blocks, coos, args.K, rec, budget_s=budget * 0.4)
    out["torch_intraop_threads"] = {"value": rate_i, "unit": "users/s", "users": n_i, "threads": cores,
                                    "what": "the same ops on whole 2048-user blocks, parallelism left to torch's intra-op pool (round 1-2's figure)"}
    if cb.eval_block_reference_topk(U[:4], I[:64], pop[:64], torch.arange(4), torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long), 8, rec) is not None:
        rate_r, n_r = cb.time_eval(U, I, pop, blocks, coos, args.K, rec, budget_s=budget * 0.4, block_fn=cb.eval_block_reference_topk)
        out["reference_arg_topk"] = {"value": rate_r, "unit": "users/s", "users": n_r, "threads": cores,
                                     "what": "matmul + head + mask as above; the selection by the reference's own arg_top_k_2d "
                                             "(util/cython/include/arg_topk.h:29, compiled where it lies into oracle/_ref)"}
    # BASELINE.md section 3 "CPU-native-topk": the same block with the selection by a from-scratch native top-K (a heap per row,
    # rows over all OpenMP threads: the algorithm class of the reference's arg_topk.h)
    rate_n, n_n = cb.time_eval(U, I, pop, blocks, coos, args.K, rec, budget_s=budget * 0.6, block_fn=cb.eval_block_native_topk)
    out["native_topk"] = {"value": rate_n, "unit": "users/s", "users": n_n, "threads": cores,
                          "what": "matmul + head + mask as above, top-K by oracle_arg_topk_2d (per-row heap select, OpenMP over rows)"}
    # also a single-thread figure (a short sample)
    torch.set_num_threads(1)
    rate1, n1 = cb.time_eval(U, I, pop, blocks, coos, args.K, rec, budget_s=min(6.0, budget / 3), warmups=1, reps=3)
    torch.set_num_threads(cores)
    out["single_thread"] = {"value": rate1, "unit": "users/s", "users": n1}
    # the native port on ONE thread (a 256-user block): what the host threads buy it
    try:
        import ctypes as _C
        gomp = _C.CDLL("libgomp.so.1")
        gomp.omp_set_num_threads(1)
        sub = [(blocks[0][:256], (coos[0][0][coos[0][0] < 256], coos[0][1][coos[0][0] < 256]))]
        rate_n1, n_n1 = cb.time_eval(U, I, pop, [b for b, _ in sub] * 3, [c for _, c in sub] * 3, args.K, rec, budget_s=6.0, warmups=1, reps=2,
                                     block_fn=cb.eval_block_native)
        gomp.omp_set_num_threads(cores)
        out["native_single_thread"] = {"value": rate_n1, "unit": "users/s", "users": n_n1, "threads_speedup": rate / rate_n1}
    except OSError:
        pass
    if train_pack is not None:
        _, W2, batches = train_pack
        cpu_batches = [tuple(t.cpu().long() if t.dtype == torch.int32 else t.cpu() for t in b) for b in batches[:16]]
        r, steps = cb.time_train(W2.U.cpu(), W2.I.cpu(), cpu_batches, 1e-2, 2048, 1e-2, budget_s=min(8.0, budget))
        out["train"] = {"value": r, "unit": "triplets/s", "steps": steps,
                        "sample": "C2 tables, B=2048, dense-decay Adam over both full tables (reference-faithful)"}
    return out


DUMP_BYTES = 48 << 20              # a dump stays below 64 MB: item ids as float64, scores as float32, user ids as float64


def dump_outputs(path, out):
    """What the headline path returned for the last timed step, as its caller receives it: the top-K item ids (float64, exact
    for any int32 id) and their fp32 scores, row r belonging to user users[r].  A block larger than DUMP_BYTES allows is
    sampled: a fixed set of rows (seed 0), the same in every run with the same arguments."""
    import numpy as np
    idx, val, users = out["idx"], out["val"], out["users"]
    n, K = idx.shape
    cap = DUMP_BYTES // (K * 12 + 8)
    rows = np.arange(n) if n <= cap else np.sort(np.random.default_rng(0).choice(n, cap, replace=False))
    sel = torch.as_tensor(rows, device=idx.device)
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "topk_items.npy"), idx.index_select(0, sel).double().cpu().numpy())
    np.save(os.path.join(path, "topk_scores.npy"), val.index_select(0, sel).float().cpu().numpy())
    if users is not None:
        np.save(os.path.join(path, "users.npy"), users.index_select(0, sel).double().cpu().numpy())


def main():
    args = parse()
    if os.environ.get("PDA_BENCH_WATCHDOG"):           # debugging aid: every thread's stack to stderr after N seconds, then exit
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["PDA_BENCH_WATCHDOG"]), exit=True)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world == 1 and args.gpus > 1:
        print("bench.py --gpus %d must be launched with torch.distributed.run (one rank per GPU)" % args.gpus, file=sys.stderr)
        sys.exit(2)
    # PDA_BENCH_ONE_GPU=1 is a plumbing check only (tests/test_gpu_two_rank.py): every rank on cuda:0 over gloo
    one_gpu = os.environ.get("PDA_BENCH_ONE_GPU") == "1"
    if one_gpu:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist
        if one_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)  # backend "nccl" IS RCCL on ROCm
    ev = bench_eval(args, rank, world, dev)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, ev["outputs"])
    # `value` is BASELINE config 4's layout: the catalogue item-sharded over ALL ranks, one list exchange among them.  Beside it, from four
    # ranks on: the two-dimensional layout of rounds 2 - 4 (user groups x item shards of 2)
    ev_grid = None
    from pda_amd.dist import grid_user_groups
    if args.full and world >= 4 and ev["layout"]["user_groups"] == 1 and grid_user_groups(world) != 1 and not args.headline_only:
        e2 = bench_eval(args, rank, world, dev, light=True, user_groups=grid_user_groups(world))
        ev_grid = {"value": e2["users_per_s"], "unit": "users/s", "ms_per_step": e2["ms_per_step"], "layout": e2["layout"],
                   "early_terminating_sweep": e2["ordered"],
                   "note": "--user-groups %d: groups of two item shards, the groups split the users of a step and never talk (pda_amd.dist.grid_layout); "
                           "predicted 6.9 x one GPU at eight ranks from per-rank steps against 6.1 - 6.9 x for item shards only (DESIGN.md section 4)"
                           % grid_user_groups(world)}
        del e2
        torch.cuda.empty_cache()
    sharded_train = bench_train_sharded(args, rank, world, dev) if (args.full and world > 1 and args.train_sharded) else None
    train_pack = None
    if args.full and world == 1 and not args.no_train:
        train_pack = bench_train(args, dev)
        if not args.headline_only and args.workload in ("c3", "tiny"):
            train_pack[0]["adam_on_headline_tables"] = bench_adam_big_tables(args, dev, args.workload)
        if not args.headline_only and args.workload in ("c3", "c5shard", "tiny"):
            # BASELINE configs 3 and 5: the SGD step on the headline workload's own tables (d = 128 fp32 / d = 256 bf16)
            td = table_dtype_of(args, args.workload)[1]
            key = "sgd_bf16" if td == torch.bfloat16 else "sgd_on_headline_tables"
            from pda_amd import synthetic as _syn
            train_pack[0][key] = sgd_rates_on_tables(args, dev, _syn.make_workload(args.workload, dev, table_dtype=td))
            torch.cuda.empty_cache()
    block2048 = None
    if args.full and world == 1 and not args.headline_only and args.workload in ("c3", "c2", "c1", "tiny") and args.head == "condition":
        block2048 = bench_reference_block_protocol(args, dev, args.workload)
        torch.cuda.empty_cache()
    cpu = None
    if args.full and world == 1 and rank == 0 and not args.no_cpu_baseline:
        cpu = cpu_baseline(args, ev, train_pack)
    # roofs measured on this box, beside the datasheet's (north_star: "measured roofline")
    from pda_amd import ops as _ops
    peaks = _ops.measured_peaks(dev) if (args.full and rank == 0) else None
    if peaks:
        r = ev["roofline"]
        r["peak_measured"] = peaks["bf16_mfma_TFLOPs"] if r["peak"] == PEAK_BF16_MFMA_TFLOPS else None
        if r["peak_measured"]:
            r["frac_of_measured"] = r["achieved"] / r["peak_measured"]
        r["hbm"]["peak_measured_GBs"] = peaks["hbm_copy_GBs"]
        r["peaks_measured"] = peaks
    # the smaller BASELINE configs beside the headline: evaluation (headline sweep + early-terminating sweep) and training
    per_config = None
    if args.full and world == 1 and rank == 0 and not args.no_per_config and not args.headline_only and args.workload == "c3":
        per_config = {}
        for wl in ("c1", "c2"):
            e = bench_eval(args, rank, world, dev, workload=wl, light=True)
            entry = {"workload": "%s: %d users x %d items, d=%d" % (wl.upper(), e["W"].n_users, e["W"].n_items, e["W"].d),
                     "eval": {"users_per_s": e["users_per_s"], "ms_per_step": e["ms_per_step"], "users_per_step": e["Bu"],
                              "roofline_frac": e["roofline"]["frac"], "kernel": e["roofline"]["kernel"], "kernel_ms": e["roofline"]["kernel_ms"],
                              "early_terminating_sweep": e["ordered"], "prep": e["prep"],
                              "raw_head": None if e["raw_head"] is None else {k: e["raw_head"][k] for k in ("value", "unit", "ms_per_step", "kernel_ms", "roofline_frac", "kernel_identity",
                                                                                                               "exact_rescorings_per_user", "rows_through_the_exact_fallback")},
                              "note": "a %d-item catalogue is %d tiles of 64: the fixed cost per user block (exact warm-up on the "
                                      "first 256 items, list hand-over, launch) is a visible share of the step" % (e["W"].n_items, -(-e["W"].n_items // 64))}}
            if not args.no_train:
                t = bench_train(args, dev, workload=wl, quick=True)[0]
                entry["train"] = {k: t[k] for k in ("sgd_fused", "sgd_exact_planned", "sgd_planned_one_launch", "sgd_fused_loop_one_launch", "sgd_fused_batches_in_sampling_order", "adam_dense_reference_faithful", "adam_dense_five_launches") if k in t}
            if not args.no_cpu_baseline:
                entry["cpu_baseline"] = cpu_baseline(args, e, None, budget=6.0, full=False)
            if wl == "c1" and not args.no_train and not args.no_cli_epoch:
                entry["cli_epoch"] = cli_epoch(cpu)
                if entry["cli_epoch"].get("train_epoch_s"):
                    entry["cli_epoch_s"] = entry["cli_epoch"]["train_epoch_s"]
                    ev_s = entry["cli_epoch"].get("eval_epoch_s") or []
                    entry["cli_eval_s"] = min(ev_s[1:]) if len(ev_s) > 1 else (ev_s[0] if ev_s else None)
            per_config[wl] = entry
            del e
            torch.cuda.empty_cache()
    if rank == 0:
        W = ev["W"]
        line = {
            "metric": "users/sec full-catalogue top-K@%d (eval)" % args.K, "value": ev["users_per_s"], "unit": "users/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ev["ms_per_step"],
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": ev["table_dtype"],
            "data": "synthetic",
            # (kept under 120 characters: the driver's record truncates longer strings)
            "config": {"workload": "%s: synthetic %d users x %d items, d=%d, %s head, masked top-K@%d"
                                   % (args.workload.upper(), W.n_users, W.n_items, W.d,
                                      "PDA condition ((elu+1)*pop^%.2f)" % W.gamma if args.head == "condition" else "raw",
                                      args.K),
                       "users_per_step": ev["Bu"],
                       # what torch.distributed itself reports: a SCALE record shows that RCCL ("nccl") saw N ranks
                       "ranks_seen": (dist_world_size() if world > 1 else 1), "backend": (dist_backend() if world > 1 else None),
                       "sharding": ("%d user group(s) x %d item shards: inside a group item-parallel (every rank owns an item slice), one RCCL "
                                    "all-to-all of the partial top-K lists per step, result sharded by user slice; the groups split the users "
                                    "of a step" % (ev["layout"]["user_groups"], ev["layout"]["item_shards"])) if world > 1 else "single GPU",
                       "layout": ev["layout"],
                       "item_shard_path": (("popularity head: 256 replicated hot rows, a rank's 1 / R of the users warmed up on them, their K-th values "
                                            "all-gathered as the seed, cold shards swept from empty lists (pda_amd.dist._topk_blocks_hot: 2 collectives per block)")
                                           if (ev["layout"]["item_shards"] >= 3 or ev["layout"]["users_per_rank_and_step"] >= 131072) else
                                           "two item shards, small blocks: every rank warms up its users itself; early-terminating sweeps exchange a seed (<= 3 collectives per block)")
                                          if (world > 1 and ev["layout"]["item_shards"] > 1) else None,
                       "train_nnz": W.n_train,
                       "arithmetic": ("fp32 tables and fp32 results, bit-identical to the exact fp32-MFMA kernel; bf16 MFMA only as a "
                                      "pre-filter with a rigorous error bound, every returned score recomputed in fp32") if ev["table_dtype"] == "f32" else
                                     ("bf16 tables; scores = the fp32 fmaf chain on the widened values (exact products), bit-identical to the exact "
                                      "kernel on the widened tables; the bf16 MFMA pass is a pre-filter with a rigorous error bound")},
            "roofline": ev["roofline"], "cpu_baseline": cpu, "dense_natural_order": ev["natural"],
            "ordered_sweep": ev["ordered"], "raw_head": ev["raw_head"], "user_groups_grid": ev_grid, "prep": ev["prep"], "per_config": per_config,
            "eval_block_2048": block2048,
            "train": train_pack[0] if train_pack else ({"item_parallel_sgd": sharded_train} if sharded_train else None),
        }
        emit(line, args)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


CONTRACT_LINE_LIMIT = 8192          # bytes: the driver's record parsed 18.7 kB in round 4 and not 21 kB in round 5; stay far below


def _pick(d, keys):
    return None if d is None else {k: d[k] for k in keys if k in d}


def compact_contract_line(line):
    """The ONE stdout line the driver parses: the contract fields, `roofline`, `cpu_baseline` and a short `summary`.
    Everything else of `line` goes to bench_extras.json / stderr (emit)."""
    r = line["roofline"] or {}
    c = line["cpu_baseline"]
    cfg = line["config"]
    out = {k: line[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                "vs_baseline", "dtype", "data")}
    out["config"] = {"workload": cfg["workload"][:120], "users_per_step": cfg["users_per_step"], "ranks_seen": cfg["ranks_seen"],
                     "backend": cfg["backend"], "layout": cfg["layout"]}
    rr = _pick(r, ("kernel_template", "kernel_identity", "bound", "achieved", "peak", "unit", "frac", "kernel_ms", "kernel_ms_spread",
                   "kernel_ms_source", "flops_per_launch", "peak_measured", "frac_of_measured"))
    t = r.get("traffic")
    rr["traffic"] = t if (t is None or not isinstance(t, dict)) else _pick(t, ("bytes_per_launch", "source"))
    rr["hbm"] = _pick(r.get("hbm"), ("algorithmic_bytes_per_launch", "frac", "peak_measured_GBs"))
    out["roofline"] = rr
    if c is not None:
        cc = _pick(c, ("value", "unit", "cores", "kind", "cpu_model"))
        cc["sample"] = str(c.get("sample", ""))[:200]
        if isinstance(c.get("train"), dict):
            cc["train"] = _pick(c["train"], ("value", "unit"))
        out["cpu_baseline"] = cc
    else:
        out["cpu_baseline"] = None
    # <= 1 kB: the other measured figures by name (all of it, with notes, is in bench_extras.json)
    s = {}
    rh = line.get("raw_head")
    if rh:
        s["raw_head"] = _pick(rh, ("ms_per_step", "roofline_frac"))
    od = line.get("ordered_sweep")
    if od:
        s["ordered_sweep"] = _pick(od, ("ms_per_step", "value"))
    pc = line.get("per_config")
    if pc:
        for wl, e in pc.items():
            ev = e.get("eval", {})
            ent = {"eval_frac": ev.get("roofline_frac"), "eval_ms": ev.get("ms_per_step")}
            if ev.get("raw_head"):
                ent["raw_frac"] = ev["raw_head"].get("roofline_frac")
                ent["raw_ms"] = ev["raw_head"].get("ms_per_step")
            tr = e.get("train") or {}
            if "adam_dense_reference_faithful" in tr:
                ent["adam_us"] = tr["adam_dense_reference_faithful"].get("us_per_step")
                ent["adam_hbm_frac"] = tr["adam_dense_reference_faithful"].get("hbm_frac")
            if "sgd_fused" in tr:
                ent["sgd_fused_us"] = tr["sgd_fused"].get("us_per_step")
            for k in ("cli_epoch_s", "cli_eval_s"):
                if k in e:
                    ent[k] = e[k]
            s[wl] = ent
    b = line.get("eval_block_2048")
    if b:
        s["eval_block_2048"] = {"ms": b.get("ms_per_block"), "device_only_frac": (b.get("device_only") or {}).get("roofline_frac"),
                                "frac": b.get("roofline_frac")}
    tr = line.get("train")
    if tr:
        a = tr.get("adam_on_headline_tables")
        if a and "dense_sweep" in a:
            s["adam_c3_sweep"] = _pick(a["dense_sweep"], ("us_per_step", "hbm_frac"))
        if "adam_dense_reference_faithful" in tr:
            s["adam_c2"] = _pick(tr["adam_dense_reference_faithful"], ("us_per_step", "hbm_frac"))
        if "sgd_fused" in tr:
            s["sgd_fused_c2"] = _pick(tr["sgd_fused"], ("us_per_step", "triplets_per_s"))
    s["extras"] = "bench_extras.json"

    def rnd(o):
        if isinstance(o, float):
            return float("%.6g" % o) if o == o and abs(o) != float("inf") else None
        if isinstance(o, dict):
            return {k: rnd(v) for k, v in o.items()}
        if isinstance(o, (list, tuple)):
            return [rnd(v) for v in o]
        return o
    out["summary"] = rnd(s)
    for k in ("roofline", "cpu_baseline", "config"):
        out[k] = rnd(out[k])
    return out


def emit(line, args):
    """Extras first (file + stderr, one JSON object per section), then the compact contract line as the LAST stdout line."""
    path = args.extras_path or "bench_extras.json"
    try:
        with open(path, "w") as f:
            json.dump(line, f)
        if os.path.isdir("gpurun_out") and not args.extras_path:
            with open(os.path.join("gpurun_out", "bench_extras.json"), "w") as f:
                json.dump(line, f)
    except OSError as e:
        print("bench_extras.json not written: %s" % e, file=sys.stderr)
    for k in ("per_config", "train", "eval_block_2048", "raw_head", "ordered_sweep", "dense_natural_order", "prep", "user_groups_grid"):
        if line.get(k) is not None:
            print(json.dumps({"extras": k, k: line[k]}), file=sys.stderr)
    sys.stderr.flush()
    text = json.dumps(compact_contract_line(line), allow_nan=False)
    if len(text) >= CONTRACT_LINE_LIMIT:
        raise SystemExit("bench.py: the contract line is %d bytes (limit %d): trim compact_contract_line" % (len(text), CONTRACT_LINE_LIMIT))
    sys.stdout.flush()
    print(text, flush=True)


if __name__ == "__main__":
    main()
