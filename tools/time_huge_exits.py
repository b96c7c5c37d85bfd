"""Two measurements around the dense call of the huge geometry (beside tools/time_huge.py).

exits   what the waves of sweep5_kernel spend OUTSIDE their asm loops: needs the profiling build
            tools/build_variant.sh exitprof -DPDA_V5_EXITPROF;  PDA_HIP_LIB=pda_amd/csrc/ab/libpda_hip_exitprof.so python tools/time_huge_exits.py exits c3
        (per workgroup the slowest wave of every counter, 100 MHz wall clock; the launch is one round, so the workgroup with the most time
        outside sets the kernel's time).  The counters slow the kernel a little: times of the call itself come from a product build.
        Beside max / mean / min of the workgroups' whole time: every workgroup's decided half-tile, the wall clock at which it went test-free,
        and the half-tiles it ran for other workgroups (the shared tail, pda_amd/csrc/pda_tail_share.h; PDA_SWEEP_TAIL_SHARE=0 in front: unshared).
pieces  the cost of one more entry of the test-free loop, same build: every workgroup runs its own decided range in n = 1, 2, 4, 8, 16 equal pieces,
        nobody shares; the slope of the call's time over n is the cost of an entry
            PDA_HIP_LIB=pda_amd/csrc/ab/libpda_hip_exitprof.so python tools/time_huge_exits.py pieces c3
mask    the warm-position mask table (ops.warm_mask_table): its one-time build, and a call with and without it at several block sizes
            python tools/time_huge_exits.py mask c3 2048,50000,262144 [order|stop]
warm    the dense call with its warm-up as one kernel (PDA_WARM_ONE_KERNEL=1) and as score + select kernel, at several block sizes
            python tools/time_huge_exits.py warm c3 2048,4096,50000,262144 [order [row]]
        row: the block's histories as a CSR by block row (no mask table: warm_mask4_kernel in front of the score kernel).  Blocks under
        4 096 users get the huge geometry only when forced: PDA_SCORE_LISTS=huge in front of the command
usage: time_huge_exits.py exits|pieces|mask|warm [workload=c3] [users per block(s)] [sweep] [row]"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
from pda_amd import _lib, ops, synthetic  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "exits"
wl = sys.argv[2] if len(sys.argv) > 2 else "c3"
sizes = [int(x) for x in (sys.argv[3] if len(sys.argv) > 3 else "262144").split(",")]
sweep = {"order": "order", "stop": True}[sys.argv[4] if len(sys.argv) > 4 else "order"]
dev = torch.device("cuda")
td = torch.bfloat16 if wl == "c5shard" else torch.float32
W = synthetic.make_workload(wl, dev, table_dtype=td)
hist = ops.HistoryCSR(W.hist_indptr, W.hist_indices, by_user=True)


by_row = len(sys.argv) > 5 and sys.argv[5] == "row"


def call(users, st=None):
    h = hist
    if by_row:          # (users are the first rows of the table: their part of the CSR is the block's CSR by block row)
        h = call.__dict__.get(len(users))
        if h is None:
            ip = W.hist_indptr[:len(users) + 1].clone()
            h = call.__dict__[len(users)] = ops.HistoryCSR(ip, W.hist_indices[:int(ip[-1])].clone(), by_user=False)
    return ops.score_topk_keys(W.U, W.I, users, 50, ops.HEAD_POP, W.pop_last, h, prune=sweep, stats=st)


def timed(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


if mode in ("exits", "pieces"):
    lib = _lib.load()
    if not hasattr(lib, "pda_debug_v5_exitprof"):
        sys.exit("this library has no exit counters: build with tools/build_variant.sh exitprof -DPDA_V5_EXITPROF and select it with PDA_HIP_LIB")
    lib.pda_debug_v5_exitprof.restype, lib.pda_debug_v5_exitprof.argtypes = C.c_int, [C.c_void_p, C.c_int]
    Bu = min(sizes[0], W.n_users)
    users = torch.arange(Bu, dtype=torch.int32, device=dev)
    st = {}
    for _ in range(3):
        k = call(users, st)
    torch.cuda.synchronize()
    ident = ops.kernel_identity(st["kernel_id"][0])
    assert ident.get("geometry") == "huge" and int(st["error"][0]) == 0, ident
    UT = 512 if W.d == 256 else 1024
    wgs = -(-Bu // UT) * k.shape[0]
    nw = 8
    if hasattr(lib, "pda_debug_v5_exitprof_words"):
        lib.pda_debug_v5_exitprof_words.restype = C.c_int
        nw = int(lib.pda_debug_v5_exitprof_words())
    if mode == "pieces":
        lib.pda_debug_v5_tail_pieces.restype, lib.pda_debug_v5_tail_pieces.argtypes = C.c_int, [C.c_int]
        print("%s %d users x %d splits, %d workgroups: the decided range of every workgroup in n equal pieces, nobody shares" % (wl, Bu, k.shape[0], wgs))
        res = {}
        for rnd in range(3):
            for n in (1, 2, 4, 8, 16):
                _lib.check(lib.pda_debug_v5_tail_pieces(n), "pda_debug_v5_tail_pieces")
                call(users, st)
                res.setdefault(n, []).append((timed(lambda: call(users), 5), float(st["huge_entries"][0]) / (4 * wgs)))
        _lib.check(lib.pda_debug_v5_tail_pieces(0), "pda_debug_v5_tail_pieces")
        for n, r in res.items():
            print("  n = %2d: call %s ms, %.2f entries per wave" % (n, " / ".join("%.4f" % t for t, _ in r), r[0][1]))
        ns = np.array(sorted(res)), np.array([min(t for t, _ in res[n]) for n in sorted(res)])
        slope = np.polyfit(ns[0], ns[1], 1)[0]
        print("  slope of the fastest times over n: %.2f us per entry (all 256 workgroups enter at once: an upper bound for a lone entry)" % (slope * 1e3))
        sys.exit(0)
    buf = np.zeros((wgs, 4, nw), dtype=np.uint64)
    _lib.check(lib.pda_debug_v5_exitprof(buf.ctypes.data_as(C.c_void_p), wgs), "pda_debug_v5_exitprof")
    us = buf.astype(np.float64) / 100.0                # 100 MHz -> microseconds
    wg = us.max(axis=1)                                # per workgroup: the slowest wave of every counter
    exits = buf[:, :, 4].max(axis=1)
    names = ["extract", "rescore_ring", "exit -> next loop call", "outside the loops", "exits", "kernel", "before the first entry", "sort and emit"]
    slow = int(np.argmax(wg[:, 3]))
    print("%s %d users x %d splits, %d workgroups; %.2f loop entries per wave; call %.3f ms" %
          (wl, Bu, k.shape[0], wgs, float(st["huge_entries"][0]) / (4 * wgs), timed(lambda: call(users), 5)))
    for f in (3, 0, 1, 2, 6, 7, 5):
        print("  %-24s max %9.1f us   mean %9.1f us   (workgroup %d: %9.1f us)" % (names[f], wg[:, f].max(), wg[:, f].mean(), slow, wg[slow, f]))
    print("  exits per workgroup: max %d  mean %.2f; workgroup %d (most time outside): %d exits, %.1f us per exit" %
          (exits.max(), exits.mean(), slow, exits[slow], wg[slow, 3] / max(1, int(exits[slow]))))
    longest = int(np.argmax(wg[:, 5]))
    print("  longest workgroup %d: kernel %.1f us, outside %.1f us, %d exits; shortest kernel %.1f us" %
          (longest, wg[longest, 5], wg[longest, 3], exits[longest], wg[:, 5].min()))
    print("  whole time of the workgroups: max %.1f us   mean %.1f us   min %.1f us   (max - mean %.1f us)" %
          (wg[:, 5].max(), wg[:, 5].mean(), wg[:, 5].min(), wg[:, 5].max() - wg[:, 5].mean()))
    if nw >= 12:
        dec, t_free, other, hend = buf[:, 0, 8].astype(np.int64), us[:, :, 9].max(axis=1), buf[:, 0, 10].astype(np.int64), buf[:, 0, 11].astype(np.int64)
        went = t_free > 0
        print("  decided half-tile (of %d .. %d per split): max %d  mean %.1f  min %d; %d of %d workgroups went test-free" %
              (hend.min(), hend.max(), dec[went].max() if went.any() else -1, dec[went].mean() if went.any() else -1, dec[went].min() if went.any() else -1, int(went.sum()), wgs))
        print("  entered the test-free part at: max %.1f us   mean %.1f us   min %.1f us" %
              ((t_free[went].max(), t_free[went].mean(), t_free[went].min()) if went.any() else (0, 0, 0)))
        print("  half-tiles run for other workgroups: total %d, by %d workgroups (max %d); chunks %d" %
              (other.sum(), int((other > 0).sum()), other.max(), int(st["tail_stolen_chunks"][0]) if "tail_stolen_chunks" in st else -1))
else:
    order = ops.visiting_order(W.I, W.pop_last)
    prep = ops.item_prep4(W.I, W.pop_last, order)

    def build():
        hist.__dict__.pop("_warm_mask_cache", None)
        return ops.warm_mask_table(hist, prep, order, 0, W.n_items, W.d)

    tab = build()
    print("%s: table of %d users (%.1f MB)%s" % (wl, W.n_users, W.n_users * 32 / 1e6, "" if tab is not None else ": beyond the budget, not built"))
    if tab is not None:
        print("  one-time build: %.3f ms" % timed(build, 5))
    for Bu in sizes:
        Bu = min(Bu, W.n_users)
        users = torch.arange(Bu, dtype=torch.int32, device=dev)
        if mode == "warm":
            # the dense call's warm-up as warm4_kernel (PDA_WARM_ONE_KERNEL=1) against score + select kernel, whole call, four alternating rounds
            res, wit = {"1": [], "": []}, {}
            for flag in ("1", "", "1", "", "1", "", "1", ""):
                os.environ["PDA_WARM_ONE_KERNEL"] = flag
                st = {}
                call(users, st)
                wit[flag] = int(st["warm_kernels"][0])
                res[flag].append(timed(lambda: call(users), 20 if Bu <= 65536 else 6))
            os.environ.pop("PDA_WARM_ONE_KERNEL")
            print("  %7d users%s, sweep %s, %s: one kernel (witness %d) %s ms | two kernels (witness %d) %s ms" %
                  (Bu, " by block row" if by_row else "", sweep, ops.kernel_identity(st["kernel_id"][0]).get("geometry"), wit["1"], " / ".join("%.4f" % x for x in res["1"]),
                   wit[""], " / ".join("%.4f" % x for x in res[""])))
            continue
        res = {}
        for flag in ("0", "1", "0", "1"):
            os.environ["PDA_WARM_MASK_TABLE"] = flag
            st = {}
            call(users, st)
            n = 20 if Bu <= 65536 else 6
            res.setdefault(flag, []).append(timed(lambda: call(users), n))
            cand = float(st["pairs_rescored"][0]) / Bu
        print("  %7d users, sweep %s: per-call walk %s ms | table %s ms   (pairs rescored per user %.3f)" %
              (Bu, sweep, " / ".join("%.4f" % x for x in res["0"]), " / ".join("%.4f" % x for x in res["1"]), cand))
