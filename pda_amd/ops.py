"""Thin, typed front-ends over the C ABI (include/pda_hip.h).  Tensors in, tensors out; every call is
stream-ordered on torch's current HIP stream.  No arithmetic happens here."""
from __future__ import annotations

import math
import os
from typing import Optional, Tuple

import ctypes as C

import torch

from . import _lib
from ._lib import (HEAD_POP, HEAD_RAW, HIST_BY_BLOCK_ROW, HIST_BY_USER_ID, UPD_ANY_ORDER, UPD_DENSE_GRAD, UPD_NONE, UPD_USERS_DISTINCT,  # noqa: F401
                   UPD_SGD_FUSED, check, ptr, stream_ptr)

ADAM_BETA1, ADAM_BETA2, ADAM_EPS = 0.9, 0.999, 1e-8   # tf.train.AdamOptimizer defaults (MF/model_api.py:83)


def _need(t: Optional[torch.Tensor], dtype, name: str, optional=False):
    if t is None:
        if optional:
            return None
        raise ValueError(f"{name} is required")
    if not t.is_cuda:
        raise ValueError(f"{name} must live in HBM (cuda tensor); pda_amd has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous (row-major)")
    return t


class HistoryCSR:
    """Train-item mask in the layout the kernel wants: CSR, int64 indptr, int32 GLOBAL item ids sorted
    ascending inside each row.  ``by_user`` tells whether rows are user ids or block rows
    (the reference builds block-row COO per 2048-user block, MF/train_new_api.py:730-739)."""

    def __init__(self, indptr: torch.Tensor, indices: torch.Tensor, by_user: bool):
        self.indptr = _need(indptr, torch.int64, "hist indptr")
        self.indices = _need(indices, torch.int32, "hist indices")
        self.mode = HIST_BY_USER_ID if by_user else HIST_BY_BLOCK_ROW

    @staticmethod
    def from_lists(rows, device, by_user: bool) -> "HistoryCSR":
        """rows: iterable of per-row item lists (any order, duplicates allowed) -> sorted CSR on device."""
        import numpy as np
        lens = np.fromiter((len(r) for r in rows), dtype=np.int64)
        indptr = np.zeros(len(lens) + 1, dtype=np.int64)
        np.cumsum(lens, out=indptr[1:])
        flat = np.empty(int(indptr[-1]), dtype=np.int32)
        for r, items in enumerate(rows):
            flat[indptr[r]:indptr[r + 1]] = np.sort(np.asarray(items, dtype=np.int32))
        return HistoryCSR(torch.from_numpy(indptr).to(device), torch.from_numpy(flat).to(device), by_user)

    @staticmethod
    def from_coo(index, n_rows: int, device) -> "HistoryCSR":
        """The reference's sparse mask triple index int64[nnz,2] = (row, item) (MF/train_new_api.py:736), built per 2 048-user
        block and handed over with every do_recommendation call (:791): one host -> device copy, then sorted and counted ON THE
        DEVICE (one 64-bit sort of row << 32 | item, a bincount, a cumsum) -- a numpy lexsort of the ~100 000 entries of a block
        cost more than the block's sweep."""
        import numpy as np
        idx = torch.from_numpy(np.ascontiguousarray(np.asarray(index, dtype=np.int64).reshape(-1, 2))).to(device, non_blocking=True)
        if idx.shape[0] == 0:
            return HistoryCSR(torch.zeros(n_rows + 1, dtype=torch.int64, device=device), torch.zeros(0, dtype=torch.int32, device=device), by_user=False)
        # (rows beyond n_rows or negative entries are a malformed mask: an error, as np.add.at / the reference's sparse tensor raise -- one min / max on
        # the device, checked behind the sort)
        bad = (idx[:, 0] < 0) | (idx[:, 0] >= n_rows) | (idx[:, 1] < 0)
        key = torch.sort((idx[:, 0] << 32) | idx[:, 1]).values
        if bool(bad.any()):
            raise IndexError("mask triple: row index outside [0, %d) or a negative item id" % n_rows)
        items = (key & 0xFFFFFFFF).to(torch.int32)
        indptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=device)
        torch.cumsum(torch.bincount(key >> 32, minlength=n_rows)[:n_rows], 0, out=indptr[1:])
        return HistoryCSR(indptr, items, by_user=False)


def auto_splits(n_users_blk: int, n_items_local: int) -> int:
    return _lib.load().pda_score_topk_auto_splits(n_users_blk, n_items_local)


import weakref

# id(tensor) -> (weakref(tensor), tensor._version, prep buffer).  Validated by OBJECT identity, never by address:
# the caching allocator hands the same address to the next table of the same shape.
_PREP_CACHE = {}


def item_prep(I_shard: torch.Tensor) -> torch.Tensor:
    """pda_item_prep_f32 (bf16 hi/lo planes + padded norms of an item shard), cached per weight version: any
    in-place update of the table bumps tensor._version and triggers a re-split."""
    lib = _lib.load()
    key = id(I_shard)
    hit = _PREP_CACHE.get(key)
    if hit is not None and hit[0]() is I_shard:
        if hit[1] == I_shard._version:
            return hit[2]
        buf = hit[2]
    else:
        n, d = I_shard.shape
        nbytes = lib.pda_item_prep_bf16_bytes(n, d) if I_shard.dtype == torch.bfloat16 else lib.pda_item_prep_bytes(n, d)
        buf = torch.empty(nbytes, dtype=torch.uint8, device=I_shard.device)
    if I_shard.dtype == torch.bfloat16:
        check(lib.pda_item_prep_bf16(ptr(I_shard), I_shard.shape[0], I_shard.shape[1], ptr(buf), stream_ptr()), "pda_item_prep_bf16")
    else:
        check(lib.pda_item_prep_f32(ptr(I_shard), I_shard.shape[0], I_shard.shape[1], ptr(buf), stream_ptr()), "pda_item_prep_f32")
    for k in [k for k, v in _PREP_CACHE.items() if v[0]() is None]:
        del _PREP_CACHE[k]                                   # drop entries whose table died
    _PREP_CACHE[key] = (weakref.ref(I_shard), I_shard._version, buf)
    return buf


_ORDER_CACHE = {}      # id(pop or table) -> (weakref, _version, order i32[n])
_PREP_ORD_CACHE = {}   # id(I_shard) -> (weakref(I), I._version, order, pop weakref|None, pop _version, prep buffer)


def visiting_order(I_shard: torch.Tensor, pop_shard: Optional[torch.Tensor]) -> torch.Tensor:
    """The order in which the ordered sweep (pda_score_topk_ordered_f32) visits the shard: most popular first
    (PDA head; does not depend on the weights, so the reordered history survives training), largest norm first (raw
    head).  Only a heuristic -- any permutation gives the same result -- hence computed here, with torch."""
    src = pop_shard if pop_shard is not None else I_shard
    hit = _ORDER_CACHE.get(id(src))
    if hit is not None and hit[0]() is src and hit[1] == src._version:
        return hit[2]
    key = pop_shard.abs() if pop_shard is not None else torch.linalg.vector_norm(I_shard.float(), dim=1)
    order = torch.argsort(key, descending=True, stable=True).to(torch.int32)
    for k in [k for k, v in _ORDER_CACHE.items() if v[0]() is None]:
        del _ORDER_CACHE[k]
    _ORDER_CACHE[id(src)] = (weakref.ref(src), src._version, order)
    return order


def item_prep_ordered(I_shard: torch.Tensor, pop_shard: Optional[torch.Tensor], order: Optional[torch.Tensor] = None):
    """pda_item_prep_ordered_f32, cached per (weight version, pop version, order).  Returns (prep buffer, order)."""
    lib = _lib.load()
    if order is None:
        order = visiting_order(I_shard, pop_shard)
    n, d = I_shard.shape
    hit = _PREP_ORD_CACHE.get(id(I_shard))
    buf = None
    if hit is not None and hit[0]() is I_shard:
        buf = hit[5]
        same_pop = (hit[3] is None and pop_shard is None) or (hit[3] is not None and pop_shard is not None and hit[3]() is pop_shard
                                                             and hit[4] == pop_shard._version)
        if hit[1] == I_shard._version and hit[2] is order and same_pop:
            return buf, order
    bf = I_shard.dtype == torch.bfloat16
    if buf is None:
        nbytes = lib.pda_item_prep_ordered_bf16_bytes(n, d) if bf else lib.pda_item_prep_ordered_bytes(n, d)
        buf = torch.empty(nbytes, dtype=torch.uint8, device=I_shard.device)
    order = _need(order, torch.int32, "order")
    if order.numel() != n:
        raise ValueError("order must have one entry per local item row")
    fn = lib.pda_item_prep_ordered_bf16 if bf else lib.pda_item_prep_ordered_f32
    check(fn(ptr(I_shard), ptr(pop_shard), ptr(order), n, d, ptr(buf), stream_ptr()), "pda_item_prep_ordered")
    for k in [k for k, v in _PREP_ORD_CACHE.items() if v[0]() is None]:
        del _PREP_ORD_CACHE[k]
    _PREP_ORD_CACHE[id(I_shard)] = (weakref.ref(I_shard), I_shard._version, order,
                                    weakref.ref(pop_shard) if pop_shard is not None else None,
                                    pop_shard._version if pop_shard is not None else 0, buf)
    return buf, order


_PREP4_CACHE = {}      # id(I_shard) -> (weakref(I), I._version, order|None, pop weakref|None, pop _version, prep buffer)
SWEEP_WARM_PER_SPLIT = 1024   # PDA_SWEEP_WARM_PER_SPLIT (include/pda_hip.h)
SWEEP_WARM_ONE_KERNEL = 2048  # PDA_SWEEP_WARM_ONE_KERNEL (include/pda_hip_experimental.h)
SWEEP_TAIL_NO_SHARE = 4096        # PDA_SWEEP_TAIL_NO_SHARE (include/pda_hip_experimental.h): the huge geometry's test-free tails are not shared
SWEEP_TAIL_OTHERS_FIRST = 8192    # PDA_SWEEP_TAIL_OTHERS_FIRST (tests)
SWEEP_TAIL_MIN2 = 16384           # PDA_SWEEP_TAIL_MIN2 (tests)
TOPK_K_V4 = 54         # pda_score_topk4_*: K <= 54 (57 list slots per user)


def item_prep4(I_shard: torch.Tensor, pop_shard: Optional[torch.Tensor], order: Optional[torch.Tensor]) -> torch.Tensor:
    """pda_item_prep4_f32 / _bf16 (padded item rows in visiting order + suffix bounds), cached per (weight version, pop
    version, order object).  order None = natural item order."""
    lib = _lib.load()
    n, d = I_shard.shape
    hit = _PREP4_CACHE.get(id(I_shard))
    buf = None
    if hit is not None and hit[0]() is I_shard:
        buf = hit[5]
        same_pop = (hit[3] is None and pop_shard is None) or (hit[3] is not None and pop_shard is not None and hit[3]() is pop_shard
                                                             and hit[4] == pop_shard._version)
        if hit[1] == I_shard._version and hit[2] is order and same_pop:
            return buf
    if buf is None:
        buf = torch.empty(lib.pda_item_prep4_bytes(n, d), dtype=torch.uint8, device=I_shard.device)
    if order is not None:
        order = _need(order, torch.int32, "order")
        if order.numel() != n:
            raise ValueError("order must have one entry per local item row")
    fn = lib.pda_item_prep4_bf16 if I_shard.dtype == torch.bfloat16 else lib.pda_item_prep4_f32
    check(fn(ptr(I_shard), ptr(pop_shard), ptr(order), n, d, ptr(buf), stream_ptr()), "pda_item_prep4")
    for k in [k for k, v in _PREP4_CACHE.items() if v[0]() is None]:
        del _PREP4_CACHE[k]
    _PREP4_CACHE[id(I_shard)] = (weakref.ref(I_shard), I_shard._version, order,
                                 weakref.ref(pop_shard) if pop_shard is not None else None,
                                 pop_shard._version if pop_shard is not None else 0, buf)
    return buf


_PREP7_CACHE = {}


def item_prep7(I_shard: torch.Tensor, order: torch.Tensor) -> torch.Tensor:
    """pda_item_prep7_f32 / _bf16: the funnel's item prep (no popularity, the half-tile image in fp16), cached per (weight version, order object) beside
    the generation-4 prep of the same table (an evaluation epoch alternates between the two heads)."""
    lib = _lib.load()
    n, d = I_shard.shape
    hit = _PREP7_CACHE.get(id(I_shard))
    buf = None
    if hit is not None and hit[0]() is I_shard:
        buf = hit[3]
        if hit[1] == I_shard._version and hit[2] is order:
            return buf
    if buf is None:
        buf = torch.empty(lib.pda_item_prep4_bytes(n, d), dtype=torch.uint8, device=I_shard.device)
    order = _need(order, torch.int32, "order")
    if order.numel() != n:
        raise ValueError("order must have one entry per local item row")
    fn = lib.pda_item_prep7_bf16 if I_shard.dtype == torch.bfloat16 else lib.pda_item_prep7_f32
    check(fn(ptr(I_shard), ptr(order), n, d, ptr(buf), stream_ptr()), "pda_item_prep7")
    for k in [k for k, v in _PREP7_CACHE.items() if v[0]() is None]:
        del _PREP7_CACHE[k]
    _PREP7_CACHE[id(I_shard)] = (weakref.ref(I_shard), I_shard._version, order, buf)
    return buf


def score_kernel(d: int, K: int, nloc: int, prune=None, head: int = HEAD_POP) -> str:
    """Which pre-filtered kernel generation serves a call.  All of them return the same keys; the choice is by measured
    speed (65 536 users per block).  Generation 4 (pda_score_topk_v4.hip: two MFMA waves per SIMD, loader and rescoring
    waves, register-resident exact warm-up) for every sweep in visiting order -- C3 dense 3.40 vs 4.61 ms, early-terminating
    0.42 vs 0.49 ms; C1/C2 0.31 vs 0.60 ms; a config-5 shard 3.2 vs 4.5 ms -- and, since its many-candidates geometry (round 3),
    for the natural-order sweeps at d <= 128; generation 3 for natural order and the raw head at d = 256, whose visiting order
    by norm leaves 300+ candidates per user (19.6 vs 29.3 ms: generation 4 keeps the d = 256 lists in HBM).  PDA_SCORE_KERNEL=v3|v4
    forces one (A/B measurements, cross-checks)."""
    import os
    forced = os.environ.get("PDA_SCORE_KERNEL", "")
    fits = d in (64, 128, 256) and K <= TOPK_K_V4 and nloc <= (1 << 26)
    if forced in ("v3", "old"):
        return "v3"
    if forced == "v4":
        return "v4" if fits else "v3"
    if not fits or (d == 256 and (head == HEAD_RAW or not prune)):
        return "v3"
    return "v4"        # (natural order at d <= 128 too since the many-candidates geometry: C3 65 536 users 7.0 vs 8.8 ms)


# The huge geometry (pda_v5_sweep.h) wants a workgroup of 1 024 users on every CU: a block of fewer than 256 x 1 024 users fills the chip
# with ITEM SPLITS (huge_splits below) -- cheap since round 4's shared warm-up (one exact warm-up per user, not per split)
HUGE_MIN_USERS = 196609         # (kept for callers that pass their own n_splits: from here on the hint is given whatever the split count)
HUGE_MIN_WORKGROUPS = 128       # of 256 CUs
HUGE_SPLIT_MIN_USERS = 4096     # below: the 256-user geometry
HUGE_MIN_TILES_PER_SPLIT = 32   # 64-item tiles: a workgroup's prologue (1 024 thresholds, 256 AGPRs per wave) wants a sweep behind it


def huge_splits(n_users: int, n_items_local: int, d: int = 128) -> int:
    """Item splits with which the huge geometry runs a block of n_users (one workgroup = 1 024 users x one split), or 0 when it should
    not (then the 256-user / wide geometry serves the call).  The time of a launch follows rounds of 256 workgroups x tiles per split:
    cost(S) = ceil(user tiles x S / 256) x (fixed cost of a workgroup + 1 / S), plus a little per split (the merge, the empty splits'
    output rows); the smallest S at the minimum wins.  Measured, config 3, with the shared warm-up (profiles/round4_shared_warm.txt): 8 192 users x 32 splits 0.47 ms
    (256-user geometry 0.58), 16 384 x 16 0.72 (1.01), 32 768 x 8 1.21 (1.82), 65 536 x 4 2.30 (wide 3.1), 131 072 x 2 4.27 (5.6);
    config 2 / config 1 (313 / 407 tiles) x 5 splits 0.37 / 0.39 ms (0.46 / 0.50)."""
    forced = os.environ.get("PDA_HUGE_SPLITS")          # A/B measurements only
    if forced and n_users >= HUGE_SPLIT_MIN_USERS:
        return int(forced)
    return _lib.load().pda_score_topk_huge_splits(n_users, n_items_local, d)      # (the rule lives in the library since round 5: pda_score_topk_plan)


SWEEP_MODE = {None: -1, False: 0, True: 1, "order": 2}
PATH_NAMES = {1: "v1", 2: "v3", 3: "v3", 4: "v4", 7: "funnel"}


def score_plan(n_users: int, n_items_local: int, d: int, K: int = 50, head: int = HEAD_POP, prune=None, bf16: bool = False,
               hist: Optional["HistoryCSR"] = None) -> dict:
    """pda_score_topk_plan: which entry point, item splits, geometry hint, visiting order and workspace the LIBRARY chooses for a call
    (prune: None = its default for the head, False = natural order, True = early-terminating, "order" = dense in visiting order)."""
    p = _lib.ScorePlan()
    check(_lib.load().pda_score_topk_plan(n_users, n_items_local, d, K, head, SWEEP_MODE[prune], int(bool(bf16)),
                                          -1 if hist is None else hist.mode, C.byref(p)), "pda_score_topk_plan")
    return {"path": p.path, "kernel": PATH_NAMES[p.path], "sweep_mode": {0: False, 1: True, 2: "order"}[p.sweep_mode], "n_splits": p.n_splits,
            "early_stop": p.early_stop, "order": p.order, "prep_with_pop": bool(p.prep_with_pop), "workspace_bytes": int(p.workspace_bytes),
            "keys_rows": int(p.keys_rows)}


def few_candidates_hint(head: int, prune, n_users: int = 0, d: int = 0, n_items_local: int = 0, n_splits: int = 0) -> int:
    """The geometry hint (PDA_SWEEP_HUGE | PDA_SWEEP_MANY_CANDIDATES | 0) for pda_score_topk4_* when the caller passes its own n_splits --
    the rules of pda_score_topk_plan (results identical whatever the hint; PDA_SCORE_LISTS=lds|many|huge forces one for A/B measurements
    and tests).  (The name is round 3's: PDA_SWEEP_FEW_CANDIDATES and PDA_SWEEP_WIDE named geometries that round 5 removed.)"""
    forced = os.environ.get("PDA_SCORE_LISTS", "")
    if forced in ("lds", "many", "huge"):
        return {"lds": 0, "many": 8, "huge": 128}[forced]
    if head == HEAD_POP and prune == "order" and d in (64, 128, 256) and n_items_local > 0 and n_splits > 0 \
            and n_splits == huge_splits(n_users, n_items_local, d):
        return 128          # (the caller splits the catalogue as huge_splits says: score_topk_keys with n_splits left to the library)
    if head == HEAD_POP and prune == "order" and n_users >= HUGE_MIN_USERS and d in (64, 128):
        return 128          # PDA_SWEEP_HUGE: 1 024-user workgroups of four 512-register waves, eight MFMAs per LDS read, no test k-step
    early = prune is True or (prune == 1 and prune != "order")
    if d in (64, 128) and not early and (head == HEAD_RAW or not prune):
        # PDA_SWEEP_MANY_CANDIDATES: hundreds of list insertions per user (raw head; popularity head in natural item order) -- 128
        # users per workgroup with eight rescoring waves.  Same box: C3 262 144 users raw 31.3 -> 28.1 ms, natural order 34.2 ->
        # 28.3 ms; C2 raw 3.39 -> 2.10 ms, natural 4.37 -> 2.39 ms.  (Early-terminating raw sweeps: 30.5 vs 37.8 ms, not hinted.)
        return 8
    return 0


def seed_exchange_applies(d: int, K: int, head: int, prune=None, impl: Optional[str] = None) -> bool:
    """Does score_topk_keys(seed_reduce=...) call seed_reduce for these arguments?  A function of arguments that are the same
    on every rank, so that ranks which cannot score (an empty item shard) still know whether to join the two all-reduces."""
    if prune is None:
        prune = prune_default(head, d)
    return (impl or score_impl(d, K, 0)) == "v2" and prune is True and d in (64, 128, 256) and K <= TOPK_K_V4


def seed_rounds(seed_shards: int) -> int:
    """Bisection rounds that tighten the seed of an item-sharded early-terminating sweep (pda_topk_seed_refine; one all-reduce
    of 4 bytes per user each): none up to 3 shards (two shards score 1.07 x the tiles of one GPU with the plain seed), three
    from 4 shards on (config 3: four shards 1.39 x -> 0.98 x, eight shards 1.78 x -> 1.03 x).  PDA_SEED_ROUNDS overrides; the same on every rank."""
    forced = os.environ.get("PDA_SEED_ROUNDS")
    if forced is not None and forced != "":
        return min(4, max(0, int(forced)))
    return 3 if seed_shards >= 4 else 0


def seed_thresholds(seed_shards: int) -> int:
    """Common thresholds of the ONE count exchange that replaces seed_rounds(seed_shards) sequential bisection rounds: the
    2^rounds - 1 interior grid points those rounds walk (7 from four shards on; 0 = the plain seed, no count exchange)."""
    return (1 << seed_rounds(seed_shards)) - 1


def check_order(prep_ord: torch.Tensor, n: int, d: int):
    """Synchronising: raises if the order given to item_prep_ordered was not a permutation of 0..n-1."""
    check(_lib.load().pda_item_prep_ordered_check(ptr(prep_ord), n, d, stream_ptr()), "pda_item_prep_ordered_check")


def hist_reordered(hist: "HistoryCSR", prep_ord: torch.Tensor, order: torch.Tensor, item_offset: int, n: int, d: int) -> torch.Tensor:
    """pda_hist_reorder, cached on the HistoryCSR per visiting order (the order object, not its contents)."""
    cache = hist.__dict__.setdefault("_ord_cache", [])
    for o, off, ind in cache:
        if o is order and off == item_offset:
            return ind
    out = torch.empty_like(hist.indices)
    check(_lib.load().pda_hist_reorder(ptr(prep_ord), n, d, item_offset, ptr(hist.indptr), ptr(hist.indices),
                                       hist.indptr.numel() - 1, ptr(out), stream_ptr()), "pda_hist_reorder")
    del cache[:-3]
    cache.append((order, item_offset, out))
    return out


WARM_MASK_TABLE_BUDGET = 64 << 20      # bytes: 32 per row of the history, i.e. 2 M users (config 5's 10 M users keep the per-call kernel)


def warm_mask_table(hist: "HistoryCSR", prep: torch.Tensor, order: Optional[torch.Tensor], item_offset: int, n: int, d: int) -> Optional[torch.Tensor]:
    """pda_score_topk4_phase_mask_table: uint32 [rows of the history, 8], row u = the train-item bits of visiting positions 0 .. 255 for user id u
    (what warm_mask4_kernel computes per call for a row whose user is u).  It depends on the train set and the visiting order only, so it is
    cached on the HistoryCSR per (prep object, order object, item_offset, n, device), as hist_reordered is; a new order drops the old table.
    None: a history by block row, a table beyond WARM_MASK_TABLE_BUDGET, or PDA_WARM_MASK_TABLE=0 (A/B runs, tests) -- the call then
    walks the histories itself, as before."""
    if hist is None or hist.mode != HIST_BY_USER_ID or os.environ.get("PDA_WARM_MASK_TABLE", "") == "0":
        return None
    rows = hist.indptr.numel() - 1
    if rows <= 0 or rows * 32 > WARM_MASK_TABLE_BUDGET:
        return None
    cache = hist.__dict__.setdefault("_warm_mask_cache", [])
    for pr, o, off, nn, dv, tab in cache:
        if pr() is prep and (o() if o is not None else None) is order and off == item_offset and nn == n and dv == prep.device:
            return tab
    # the prep buffer and the order are held weakly, as _PREP4_CACHE holds its tensors: the history pins neither (hundreds of MB at config 3).
    # A table goes when its prep or order died, or when its prep has a new order.
    cache[:] = [c for c in cache if c[0]() is not None and (c[1] is None or c[1]() is not None)
                and not (c[0]() is prep and c[2] == item_offset and c[3] == n)][-3:]
    tab = torch.empty((rows, 8), dtype=torch.int32, device=prep.device)
    check(_lib.load().pda_score_topk4_phase_mask_table(ptr(prep), n, d, item_offset, ptr(hist.indptr), ptr(hist.indices), rows, ptr(tab), stream_ptr()),
          "pda_score_topk4_phase_mask_table")
    cache.append((weakref.ref(prep), weakref.ref(order) if order is not None else None, item_offset, n, prep.device, tab))
    return tab


def mark_modified(*tensors):
    """Tell torch that a kernel wrote these tensors through raw pointers: bumps tensor._version, which is what keys
    the item_prep cache (and autograd's in-place checks)."""
    for t in tensors:
        if t is not None:
            torch.autograd.graph.increment_version(t)


def score_impl(d: int, K: int, item_hi: int) -> str:
    """'v2' = the pre-filtered kernels (bf16 MFMA filter + exact fp32 rescoring: pda_score_topk_v3.hip / _v4.hip; the label
    is historical) where they apply, else 'v1' (exact fp32 MFMA).  Same results.  PDA_SCORE_IMPL=v1|v2 forces one (A/B
    measurements, cross-checks)."""
    import os
    forced = os.environ.get("PDA_SCORE_IMPL", "")
    ok = d in (64, 128, 256) and K <= TOPK_CAP_V2
    if forced == "v1" or not ok:
        return "v1"
    return "v2"


TOPK_CAP_V2 = _lib.TOPK_CAP - 4


_POP_OK = {}           # id(pop) -> (weakref, _version): popularity vectors already checked


def _check_pop(pop_shard: torch.Tensor):
    """The PDA head's filters and bounds are derived for pop >= 0 (it is pop^gamma of a min-max-normalised count,
    MF/train_new_api.py:952-959).  Checked once per tensor version (one device sync).  NaN entries are tolerated: their
    head is NaN, every comparison with it is false, the item is never recommended."""
    hit = _POP_OK.get(id(pop_shard))
    if hit is not None and hit[0]() is pop_shard and hit[1] == pop_shard._version:
        return
    if bool((pop_shard < 0).any()):        # NaN passes: such items simply never rank (the reference's BPRMF-A search feeds NaNs)
        raise ValueError("pop_shard must be >= 0 (it is pop**gamma of a normalised count)")
    for k in [k for k, v in _POP_OK.items() if v[0]() is None]:
        del _POP_OK[k]
    _POP_OK[id(pop_shard)] = (weakref.ref(pop_shard), pop_shard._version)


def prune_default(head: int, d: Optional[int] = None):
    """How the catalogue is swept (results are identical in all three):
        True     visiting order (popular first) + exact early termination -- the default for the popularity-weighted head
        "order"  visiting order, every tile scored (a dense sweep whose thresholds rise early: fewer candidates) -- the
                 default for the raw head at d <= 128 (largest norm first, generation 4: C3 8.3 vs 9.0 ms, C2 3.2 vs 4.0 ms)
        False    natural item order, every tile scored -- the raw head at d = 256 (generation 3: 16.5 vs 22.9 ms)
    PDA_SCORE_PRUNE=0|1|order forces one."""
    import os
    forced = os.environ.get("PDA_SCORE_PRUNE", "")
    if forced in ("0", "1"):
        return forced == "1"
    if forced == "order":
        return "order"
    if head == HEAD_POP:
        return True
    return "order" if d in (64, 128) else False


class SeededCall:
    """One user block of an item-sharded early-terminating sweep between its steps (seeded_begin -> the MAX all-reduce of
    .bounds -> seeded_counts -> the SUM all-reduce of .counts -> seeded_finish): what lets pda_amd.dist run the two collectives
    of block b + 1 on a side stream under the sweep of block b."""
    __slots__ = ("lib", "fnp", "common", "wt", "out", "ws", "bounds", "counts", "n_thr", "K", "nu", "n_splits", "nloc", "stats", "keep")


def seeded_begin(U, I_shard, users, K, head, pop_shard, hist, item_offset=0, n_splits=0, seed_shards=1, prune=True,
                 stats: Optional[dict] = None) -> SeededCall:
    """Step 1: the exact warm-up of this shard (pda_score_topk4_phase_*, phase 1) and the shard's three bounds per user
    (pda_topk_seed_bounds) -> .bounds float32 [3, Bu], to be MAX-reduced over the shards in place."""
    lib = _lib.load()
    bf = I_shard.dtype == torch.bfloat16
    U = _need(U, torch.bfloat16 if bf else torch.float32, "U")
    I_shard = _need(I_shard, torch.bfloat16 if bf else torch.float32, "I_shard")
    users = _need(users, torch.int32, "users")
    pop_shard = _need(pop_shard, torch.float32, "pop_shard", optional=True)
    nu, nloc, d = users.numel(), I_shard.shape[0], I_shard.shape[1]
    if U.shape[1] != d:
        raise ValueError("U and I_shard disagree on embed dim")
    if pop_shard is not None and pop_shard.numel() != nloc:
        raise ValueError("pop_shard must have one entry per local item row")
    if nloc > (1 << 26):
        raise ValueError("seeded item-sharded evaluation: at most 2^26 item rows per shard")
    if head == HEAD_POP and pop_shard is not None:
        _check_pop(pop_shard)
    if hist is not None and hist.indices.numel() == 0:
        hist = None
    c = SeededCall()
    order = visiting_order(I_shard, pop_shard if head == HEAD_POP else None)
    prep = item_prep4(I_shard, pop_shard if head == HEAD_POP else None, order)
    if n_splits <= 0:
        n_splits = lib.pda_score_topk4_auto_splits(nu, nloc, d)
    c.lib, c.K, c.nu, c.n_splits, c.nloc, c.stats = lib, K, nu, n_splits, nloc, stats
    c.out = torch.empty((n_splits, nu, K), dtype=torch.int64, device=U.device)
    c.ws = torch.empty(lib.pda_score_topk4_workspace_bytes(nu, nloc, d, n_splits), dtype=torch.uint8, device=U.device)
    c.fnp = lib.pda_score_topk4_phase_bf16 if bf else lib.pda_score_topk4_phase_f32
    c.common = (ptr(U), ptr(I_shard), ptr(prep), ptr(pop_shard), ptr(users), nu, item_offset, nloc, d,
                ptr(hist.indptr) if hist else None, ptr(hist.indices) if hist else None, hist.mode if hist else 0, K, head,
                1 | few_candidates_hint(head, True, nu, d), n_splits)
    c.keep = (U, I_shard, prep, pop_shard, users, hist)          # the pointers above stay valid until seeded_finish
    # R shards warm up R x 64 warm_tiles items between them: two tiles each on 2 shards, one from 4 shards on
    c.wt = int(os.environ.get("PDA_WARM_TILES", "0")) or max(1, 4 // max(1, seed_shards))
    check(c.fnp(*c.common, 1, c.wt, None, ptr(c.out), ptr(c.ws), stream_ptr()), "pda_score_topk4_phase (warm-up)")
    c.bounds = torch.empty((3, nu), dtype=torch.float32, device=U.device)
    m = -(-K // max(1, seed_shards))
    check(lib.pda_topk_seed_bounds(ptr(c.out), n_splits, nu, K, m, ptr(c.bounds), stream_ptr()), "pda_topk_seed_bounds")
    c.n_thr, c.counts = seed_thresholds(seed_shards), None
    return c


def kth_value(keys: torch.Tensor, pos: int) -> torch.Tensor:
    """pda_topk_kth_value: keys int64 [S, Bu, K] (sorted lists) -> float32 [Bu], the value at rank `pos` (0-based; the largest over
    the S lists, -inf where no list is that long)."""
    keys = _need(keys, torch.int64, "keys")
    S, nu, K = keys.shape
    out = torch.empty(nu, dtype=torch.float32, device=keys.device)
    check(_lib.load().pda_topk_kth_value(ptr(keys), S, nu, K, int(pos), ptr(out), stream_ptr()), "pda_topk_kth_value")
    return out


def remap_key_items(keys: torch.Tensor, gid: torch.Tensor) -> torch.Tensor:
    """pda_topk_remap_items, IN PLACE: the item field of packed keys from local row ids of a gathered table to gid[local]."""
    keys = _need(keys, torch.int64, "keys")
    gid = _need(gid, torch.int32, "gid")
    check(_lib.load().pda_topk_remap_items(ptr(keys), keys.numel(), ptr(gid), gid.numel(), stream_ptr()), "pda_topk_remap_items")
    return keys


def sweep_from_seed(U, I_shard, users, K, head, pop_shard, hist, item_offset, seed: torch.Tensor, n_splits: int = 0, prune="order",
                    stats: Optional[dict] = None) -> torch.Tensor:
    """pda_score_topk4_phase_* with phase 4: the sweep of the whole shard from EMPTY lists against `seed` (float32 [Bu]: a lower
    bound of every user's final K-th value, -inf = none) -- no warm-up on this shard.  -> packed keys int64 [n_splits, Bu, K] of the
    pairs at or above the seed (a list may end shorter than K, or empty)."""
    lib = _lib.load()
    bf = I_shard.dtype == torch.bfloat16
    U = _need(U, torch.bfloat16 if bf else torch.float32, "U")
    I_shard = _need(I_shard, torch.bfloat16 if bf else torch.float32, "I_shard")
    users = _need(users, torch.int32, "users")
    seed = _need(seed, torch.float32, "seed")
    pop_shard = _need(pop_shard, torch.float32, "pop_shard", optional=True)
    nu, nloc, d = users.numel(), I_shard.shape[0], I_shard.shape[1]
    if seed.numel() != nu:
        raise ValueError("seed must have one entry per user of the block")
    if d not in (64, 128, 256) or K > TOPK_K_V4:
        raise ValueError("sweep_from_seed: embed dim 64/128/256 and K <= %d" % TOPK_K_V4)
    if head == HEAD_POP and pop_shard is not None:
        _check_pop(pop_shard)
    if hist is not None and hist.indices.numel() == 0:
        hist = None
    order = visiting_order(I_shard, pop_shard if head == HEAD_POP else None) if prune else None
    prep = item_prep4(I_shard, pop_shard if head == HEAD_POP else None, order)
    if n_splits <= 0:
        n_splits = lib.pda_score_topk4_auto_splits(nu, nloc, d)
        if head == HEAD_POP and prune == "order" and d in (64, 128, 256) and not os.environ.get("PDA_SCORE_LISTS") and pop_shard is not None:
            n_splits = huge_splits(nu, nloc, d) or n_splits
    out = torch.empty((n_splits, nu, K), dtype=torch.int64, device=U.device)
    ws = torch.empty(lib.pda_score_topk4_workspace_bytes(nu, nloc, d, n_splits), dtype=torch.uint8, device=U.device)
    es = (1 if prune is True else 0) | few_candidates_hint(head, prune, nu, d, nloc, n_splits)
    fn = lib.pda_score_topk4_phase_bf16 if bf else lib.pda_score_topk4_phase_f32
    check(fn(ptr(U), ptr(I_shard), ptr(prep), ptr(pop_shard), ptr(users), nu, item_offset, nloc, d,
             ptr(hist.indptr) if hist else None, ptr(hist.indices) if hist else None, hist.mode if hist else 0, K, head, es, n_splits,
             4, 0, ptr(seed), ptr(out), ptr(ws), stream_ptr()), "pda_score_topk4_phase (sweep from a seed)")
    if os.environ.get("PDA_CHECK_SWEEP_ERRORS"):
        err = int(ws[0:4].view(torch.int32)[0])
        if err != 0:
            raise RuntimeError("pda_score_topk4_phase: the sweep reported protocol error %d" % err)
    if stats is not None:
        stats["pairs_rescored"] = ws[4:8].view(torch.int32)
        stats["kernel_id"] = ws[16:20].view(torch.int32)
        stats["huge_entries"] = ws[20:24].view(torch.int32)
        stats["huge_free_halftiles"] = ws[28:32].view(torch.int32)
        stats["error"] = ws[0:4].view(torch.int32)
    return out


def tail_record_offset(nu: int) -> int:
    """Byte offset, in the workspace of pda_score_topk4_*, of the huge geometry's shared-tail records (pda_amd/csrc/pda_tail_share.h): directly
    behind the counters."""
    return (_lib.load().pda_score_topk_workspace_bytes(nu) + 255) & ~255


def seeded_counts(c: SeededCall) -> Optional[torch.Tensor]:
    """Step 2 (after the MAX all-reduce of c.bounds): this shard's warm-up entries at or above the common thresholds ->
    int32 [n_thr, Bu], to be SUM-reduced in place; None below four shards (plain seed: no second collective)."""
    if c.n_thr <= 0:
        return None
    c.counts = torch.empty((c.n_thr, c.nu), dtype=torch.int32, device=c.bounds.device)
    check(c.lib.pda_topk_seed_counts(ptr(c.out), c.n_splits, c.nu, c.K, ptr(c.bounds), c.n_thr, ptr(c.counts), stream_ptr()),
          "pda_topk_seed_counts")
    return c.counts


def seeded_finish(c: SeededCall) -> torch.Tensor:
    """Step 3 (after the SUM all-reduce of c.counts): the seed per user (pda_topk_seed_pick) and the sweep that prunes against
    it (phase 2).  Returns the shard's packed keys int64 [n_splits, Bu, K]; lists may end shorter than K."""
    seed = torch.empty(c.nu, dtype=torch.float32, device=c.bounds.device)
    check(c.lib.pda_topk_seed_pick(ptr(c.bounds), ptr(c.counts), c.n_thr if c.counts is not None else 0, c.nu, c.K, ptr(seed), stream_ptr()),
          "pda_topk_seed_pick")
    check(c.fnp(*c.common, 2, c.wt, ptr(seed), ptr(c.out), ptr(c.ws), stream_ptr()), "pda_score_topk4_phase (sweep)")
    if c.stats is not None:
        c.stats["tiles_scored"] = c.ws[8:16].view(torch.int64)
        c.stats["pairs_rescored"] = c.ws[4:8].view(torch.int32)
        c.stats["tiles_dense"] = ((c.nloc + 31) // 32) * ((c.nu + 127) // 128)
        c.stats["kernel_id"] = c.ws[16:20].view(torch.int32)
        c.stats["error"] = c.ws[0:4].view(torch.int32)
    out, c.keep = c.out, None
    return out


def score_topk_keys(U, I_shard, users, K=50, head=HEAD_RAW, pop_shard=None, hist: Optional[HistoryCSR] = None,
                    item_offset=0, n_splits=0, out: Optional[torch.Tensor] = None, impl: Optional[str] = None,
                    prune=None, stats: Optional[dict] = None, seed_reduce=None, seed_shards: int = 1, seed_sum=None,
                    warm_tiles: int = 0) -> torch.Tensor:
    """pda_score_topk_f32 / pda_score_topk_prepped_f32 / pda_score_topk_ordered_f32 / pda_score_topk4_* -> packed keys
    int64[n_splits, Bu, K] (uint64 bit patterns), best first.  All of them return the same keys.

    seed_reduce (item-sharded evaluation over `seed_shards` shards, early-terminating sweep): a callable that receives this
    shard's float32 [3, Bu] bounds (pda_topk_seed_bounds: warm-up values at rank K, at rank ceil(K / seed_shards), and minus the
    latter) and turns them IN PLACE into the maximum over all shards (ONE dist.all_reduce MAX).  seed_sum (optional; int32
    [n_thr, Bu] -> the sum over the shards in place, ONE all_reduce SUM): the counts at seed_thresholds(seed_shards) common
    thresholds tighten the bound first.  The sweep prunes against the resulting seed (pda_score_topk4_phase_*); the shard's lists
    may end shorter than K -- merge them with the other shards' lists.  (seeded_begin / seeded_counts / seeded_finish are the
    same three steps as separate calls.)
    warm_tiles (generation 4 only; 0 = the library's default of 4): 64-item tiles per split scored by the exact warm-up kernel --
    an item shard of an R-rank job wants 4 / R (pda_amd.dist): the R warm-ups cover R x 64 x warm_tiles items between them."""
    lib = _lib.load()
    bf = I_shard is not None and I_shard.dtype == torch.bfloat16       # bf16 tables: pda_score_topk_bf16 (both tables bf16)
    U = _need(U, torch.bfloat16 if bf else torch.float32, "U")
    I_shard = _need(I_shard, torch.bfloat16 if bf else torch.float32, "I_shard")
    users = _need(users, torch.int32, "users")
    pop_shard = _need(pop_shard, torch.float32, "pop_shard", optional=True)
    nu, nloc, d = users.numel(), I_shard.shape[0], I_shard.shape[1]
    if bf:
        if d not in (64, 128, 256) or K > TOPK_CAP_V2 or impl == "v1":
            raise ValueError("bf16 tables: embed dim 64/128/256, K <= %d, no v1 entry point" % TOPK_CAP_V2)
        impl = "v2"
    if U.shape[1] != d:
        raise ValueError("U and I_shard disagree on embed dim")
    if pop_shard is not None and pop_shard.numel() != nloc:
        raise ValueError("pop_shard must have one entry per local item row")
    if head == HEAD_POP and pop_shard is not None:       # (a missing pop_shard is the library's PDA_ERR_ARG)
        _check_pop(pop_shard)
    if hist is not None and hist.indices.numel() == 0:
        hist = None                       # an all-empty mask: the kernel must never dereference a 0-length buffer
    n_splits_auto = n_splits <= 0
    out_given = out
    impl = impl or score_impl(d, K, item_offset + nloc)
    if prune is None:
        prune = prune_default(head, d)
    if seed_reduce is not None and seed_exchange_applies(d, K, head, prune, impl):
        if out_given is not None:
            raise ValueError("the seeded sweep allocates its own output")
        c = seeded_begin(U, I_shard, users, K, head, pop_shard, hist, item_offset, n_splits, seed_shards, stats=stats)
        seed_reduce(c.bounds)
        cnt = seeded_counts(c) if seed_sum is not None else None
        if cnt is not None:
            seed_sum(cnt)
        return seeded_finish(c)
    if n_splits_auto and out_given is None and impl == "v2" and funnel_applies(d, K, nu, nloc, head, prune, hist):
        return score_topk_funnel(U, I_shard, users, K, hist, item_offset, stats)
    if n_splits <= 0:
        n_splits = lib.pda_score_topk_auto_splits(nu, nloc)
    if out is None:
        out = torch.empty((n_splits, nu, K), dtype=torch.int64, device=U.device)
    elif out.shape != (n_splits, nu, K) or out.dtype != torch.int64:
        raise ValueError("out must be int64 [n_splits, Bu, K]")
    if impl == "v2" and score_kernel(d, K, nloc, prune, head) == "v4":
        order = visiting_order(I_shard, pop_shard if head == HEAD_POP else None) if prune else None
        prep = item_prep4(I_shard, pop_shard if head == HEAD_POP else None, order)
        forced_env = any(os.environ.get(k) for k in ("PDA_SCORE_LISTS", "PDA_SCORE_KERNEL", "PDA_HUGE_SPLITS"))
        plan = None
        if n_splits_auto and out_given is None and not forced_env and not (head == HEAD_POP and pop_shard is None):
            # the library's own plan (pda_score_topk_plan): item splits and geometry hint
            plan = score_plan(nu, nloc, d, K, head, prune, bf, hist)
            if plan["kernel"] != "v4":
                plan = None
        if plan is not None:
            n_splits = plan["n_splits"]
            out = torch.empty((n_splits, nu, K), dtype=torch.int64, device=U.device)
        elif n_splits_auto and out_given is None:
            n_splits = lib.pda_score_topk4_auto_splits(nu, nloc, d)
            if head == HEAD_POP and prune == "order" and d in (64, 128, 256) and not os.environ.get("PDA_SCORE_LISTS") and pop_shard is not None:
                n_splits = huge_splits(nu, nloc, d) or n_splits          # the huge geometry on a block that does not fill the chip by itself
            out = torch.empty((n_splits, nu, K), dtype=torch.int64, device=U.device)
        ws = torch.empty(lib.pda_score_topk4_workspace_bytes(nu, nloc, d, n_splits), dtype=torch.uint8, device=U.device)
        hint = plan["early_stop"] if plan is not None else ((1 if prune is True else 0) | few_candidates_hint(head, prune, nu, d, nloc, n_splits))
        es = hint | ((min(4, max(0, int(warm_tiles))) & 7) << 4)
        if os.environ.get("PDA_WARM_PER_SPLIT"):      # A/B measurements and cross-checks: every item split warms up on its own tiles (before round 4)
            es |= SWEEP_WARM_PER_SPLIT
        if os.environ.get("PDA_WARM_ONE_KERNEL"):     # A/B measurements and tests: the dense call's warm-up as warm4_kernel, not as score + select kernel
            es |= SWEEP_WARM_ONE_KERNEL
        if os.environ.get("PDA_SWEEP_TAIL_SHARE") == "0":   # A/B measurements and tests: every workgroup of the huge geometry runs its own test-free tail
            es |= SWEEP_TAIL_NO_SHARE
        if os.environ.get("PDA_SWEEP_TAIL_OTHERS_FIRST"):    # tests: a workgroup looks at the other workgroups' records before it runs its own range
            es |= SWEEP_TAIL_OTHERS_FIRST
        if os.environ.get("PDA_SWEEP_TAIL_MIN_CHUNK") == "2":   # tests: chunks down to 2 half-tiles
            es |= SWEEP_TAIL_MIN2
        # the warm-position masks of every user, built once per history and order: the call gathers them instead of walking the histories
        # (one warm-up over the front of the whole order: one split, or the shared warm-up of several)
        tab = warm_mask_table(hist, prep, order, item_offset, nloc, d) if hist and (n_splits == 1 or not (es & SWEEP_WARM_PER_SPLIT)) else None
        if tab is not None:
            fn = lib.pda_score_topk4_phase_masked_bf16 if bf else lib.pda_score_topk4_phase_masked_f32
            check(fn(ptr(U), ptr(I_shard), ptr(prep), ptr(pop_shard), ptr(users), nu, item_offset, nloc, d,
                     ptr(hist.indptr), ptr(hist.indices), hist.mode, K, head, es, n_splits, ptr(tab), tab.shape[0],
                     ptr(out), ptr(ws), stream_ptr()), "pda_score_topk4_phase_masked")
        else:
            fn = lib.pda_score_topk4_bf16 if bf else lib.pda_score_topk4_f32
            check(fn(ptr(U), ptr(I_shard), ptr(prep), ptr(pop_shard), ptr(users), nu, item_offset, nloc, d,
                     ptr(hist.indptr) if hist else None, ptr(hist.indices) if hist else None, hist.mode if hist else 0,
                     K, head, es, n_splits, ptr(out), ptr(ws), stream_ptr()), "pda_score_topk4")
        if os.environ.get("PDA_CHECK_SWEEP_ERRORS"):          # (tests: synchronising) a bounded wait of the sweep ran out, or the huge geometry's self-check failed
            err = int(ws[0:4].view(torch.int32)[0])
            if err != 0:
                raise RuntimeError("pda_score_topk4: the sweep reported protocol error %d" % err)
        if stats is not None:
            stats["tiles_scored"] = ws[8:16].view(torch.int64)
            stats["pairs_rescored"] = ws[4:8].view(torch.int32)
            stats["tiles_dense"] = ((nloc + 31) // 32) * ((nu + 127) // 128)
            stats["kernel_id"] = ws[16:20].view(torch.int32)     # written by the sweep kernel itself: see kernel_identity()
            stats["huge_entries"] = ws[20:24].view(torch.int32)  # huge geometry: entries of its asm loop, summed over the waves (1 per wave + 1 per flagged half-tile)
            stats["huge_free_halftiles"] = ws[28:32].view(torch.int32)  # huge geometry: 32-item half-tiles run without threshold tests (behind the decided half-tile), summed over the workgroups
            stats["warm_kernels"] = ws[32:36].view(torch.int32)  # which exact warm-up ran: 0 = warm4_kernel, 5 = warm_score5_kernel + warm_select5_kernel
            stats["tail_stolen_chunks"] = ws[36:40].view(torch.int32)     # huge geometry: chunks of test-free half-tiles run for ANOTHER workgroup
            stats["tail_stolen_halftiles"] = ws[40:44].view(torch.int32)  # ... and the half-tiles in them
            stats["tail_records"] = ws[tail_record_offset(nu):tail_record_offset(nu) + 8 * (-(-nu // (512 if d == 256 else 1024)) * n_splits)].view(torch.int64)  # one per workgroup: end << 32 | next (0: nothing published)
            stats["error"] = ws[0:4].view(torch.int32)           # 0, or which bounded wait of the sweep ran out (1 .. 4: hand-over words; 5, 6: huge geometry)
            stats["workspace"] = ws                               # (tests read the huge geometry's user image out of it: huge_image_offsets)
            stats["n_splits"] = n_splits
            stats["warm_mask_table"] = tab                        # the cached table handed to the call, or None (that the library reads it: test_an_altered_table_changes_the_keys)
        return out
    if impl == "v2" and prune:
        prep, order = item_prep_ordered(I_shard, pop_shard if head == HEAD_POP else None)
        hist_ord = hist_reordered(hist, prep, order, item_offset, nloc, d) if hist else None
        ws = torch.empty(lib.pda_score_topk_workspace_bytes(nu), dtype=torch.uint8, device=U.device)
        fn = lib.pda_score_topk_ordered_bf16 if bf else lib.pda_score_topk_ordered_f32
        check(fn(ptr(U), ptr(I_shard), ptr(prep), ptr(pop_shard), ptr(users), nu, item_offset,
                                             nloc, d, ptr(hist.indptr) if hist else None,
                                             ptr(hist.indices) if hist else None, ptr(hist_ord), hist.mode if hist else 0,
                                             K, head, 0 if prune == "order" else 1, n_splits, ptr(out), ptr(ws), stream_ptr()),
              "pda_score_topk_ordered")
        if stats is not None:            # device scalar (no sync here): item tiles scored, summed over workgroups
            stats["tiles_scored"] = ws[8:16].view(torch.int64)
            stats["pairs_rescored"] = ws[4:8].view(torch.int32)        # v3 kernel only (0 otherwise)
            stats["tiles_dense"] = ((nloc + 31) // 32) * ((nu + 127) // 128)
            stats["kernel_id"] = ws[16:20].view(torch.int32)
        return out
    if impl == "v2":
        prep = item_prep(I_shard)
        ws = torch.empty(lib.pda_score_topk_workspace_bytes(nu), dtype=torch.uint8, device=U.device)   # per call: re-entrant
        fn = lib.pda_score_topk_bf16 if bf else lib.pda_score_topk_prepped_f32
        check(fn(ptr(U), ptr(I_shard), ptr(prep), ptr(pop_shard), ptr(users), nu, item_offset,
                                             nloc, d, ptr(hist.indptr) if hist else None,
                                             ptr(hist.indices) if hist else None, hist.mode if hist else 0, K, head,
                                             n_splits, ptr(out), ptr(ws), stream_ptr()), "pda_score_topk_prepped_f32")
        return out
    check(lib.pda_score_topk_f32(ptr(U), ptr(I_shard), ptr(pop_shard), ptr(users), nu, item_offset, nloc, d,
                                 ptr(hist.indptr) if hist else None, ptr(hist.indices) if hist else None,
                                 hist.mode if hist else 0, K, head, n_splits, ptr(out), stream_ptr()),
          "pda_score_topk_f32")
    return out


# ---- the funnel (pda_score_topk7_*): the raw head on large user blocks ------------------------------------------------------------
# Measured (config 3, same box): 262 144 users 22.3 vs 29.7 ms for generation 4's many-candidates geometry, 65 536 users 6.4 vs 7.3 ms; config 2 (50 000 users
# x 20 000 items, d = 64) 3.3 vs 2.1 ms -- a funnel is ~25 launches whose per-row work does not shrink with the catalogue.
FUNNEL_MIN_USERS = 1             # (round 6; 1 024 before: a partly filled 1 024-user tile still wins -- 256 users x 200 000 items 0.27 - 0.32 vs 2.0 - 2.2 ms for generation 4)
FUNNEL_MIN_ITEMS = 4096           # (round 6: the funnel's own minimum; 8 192 items x 4 096 users 0.32 vs 0.43 ms for generation 4)
FUNNEL_BLOCK_ROW_MAX_USERS = 16384        # a mask by BLOCK ROW (the reference's per-block COO triple): the exact fallback sweeps the whole block again if a row fails
FUNNEL_SMALL_ITEMS, FUNNEL_SMALL_MAX_USERS = 20000, 16384     # catalogues below 20 000 items: up to 16 384 users (16 384 items x 65 536 users: 2.1 vs 1.9 ms for generation 4)
_FUNNEL_ORDER = {}               # (n, device) -> a fixed pseudo-random permutation (the object is what the prep cache keys on)


def funnel_order(I_shard: torch.Tensor) -> torch.Tensor:
    """The visiting order of a funnel: a RANDOM permutation of the shard (seeded by its size: reproducible).  The ranks of the funnel's
    thresholds assume that the items seen so far are a uniform sample of the catalogue; results are exact for any order."""
    key = (I_shard.shape[0], str(I_shard.device))
    o = _FUNNEL_ORDER.get(key)
    if o is None:
        g = torch.Generator(device="cpu").manual_seed(0x5EED + I_shard.shape[0])
        o = torch.randperm(I_shard.shape[0], generator=g).to(torch.int32).to(I_shard.device)
        _FUNNEL_ORDER[key] = o
    return o


FUNNEL_WORKSPACE_BUDGET = 24 << 30      # PDA_FUNNEL_WORKSPACE_BUDGET (include/pda_hip.h)


def funnel_applies(d: int, K: int, nu: int, nloc: int, head: int, prune, hist: Optional[HistoryCSR]) -> bool:
    """Does score_topk_keys serve this call with the funnel?  (PDA_SCORE_FUNNEL=0 | 1 forces it off / on wherever it can run.)"""
    can = head == HEAD_RAW and d in (64, 128, 256) and K <= TOPK_K_V4 and 4096 <= nloc <= (1 << 26) and prune is not True \
        and (hist is None or hist.mode == HIST_BY_USER_ID or nu <= FUNNEL_BLOCK_ROW_MAX_USERS)
    forced = os.environ.get("PDA_SCORE_FUNNEL", "")
    if forced == "0" or not can:
        return False
    if forced == "1":
        return True
    return nu >= FUNNEL_MIN_USERS and nloc >= FUNNEL_MIN_ITEMS and (nloc >= FUNNEL_SMALL_ITEMS or nu <= FUNNEL_SMALL_MAX_USERS) \
        and not os.environ.get("PDA_SCORE_KERNEL") and not os.environ.get("PDA_SCORE_LISTS") \
        and _lib.load().pda_score_topk7_workspace_bytes(nu, nloc, d) <= FUNNEL_WORKSPACE_BUDGET     # (~27 KB per user: pda_score_topk_plan's rule)


def score_topk_funnel(U, I_shard, users, K=50, hist: Optional[HistoryCSR] = None, item_offset=0, stats: Optional[dict] = None) -> torch.Tensor:
    """pda_score_topk7_f32 / _bf16: the raw head through the funnel -> packed keys int64 [1, Bu, K] (the item splits are merged inside)."""
    lib = _lib.load()
    bf = I_shard.dtype == torch.bfloat16
    U = _need(U, torch.bfloat16 if bf else torch.float32, "U")
    I_shard = _need(I_shard, torch.bfloat16 if bf else torch.float32, "I_shard")
    users = _need(users, torch.int32, "users")
    nu, nloc, d = users.numel(), I_shard.shape[0], I_shard.shape[1]
    if hist is not None and hist.indices.numel() == 0:
        hist = None
    prep = item_prep7(I_shard, funnel_order(I_shard))
    out = torch.empty((1, nu, K), dtype=torch.int64, device=U.device)
    nbytes = lib.pda_score_topk7_workspace_bytes(nu, nloc, d)
    if nbytes == 0:
        raise ValueError("the funnel: embed dim 64 / 128 / 256")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=U.device)
    fn = lib.pda_score_topk7_bf16 if bf else lib.pda_score_topk7_f32
    check(fn(ptr(U), ptr(I_shard), ptr(prep), ptr(users), nu, item_offset, nloc, d, ptr(hist.indptr) if hist else None,
             ptr(hist.indices) if hist else None, hist.mode if hist else 0, K, HEAD_RAW, ptr(out), ptr(ws), stream_ptr()), "pda_score_topk7")
    if stats is not None:
        stats["pairs_rescored"] = ws[4:8].view(torch.int32)
        stats["kernel_id"] = ws[16:20].view(torch.int32)
        stats["error"] = ws[0:4].view(torch.int32)
        stats["fallback_rows"] = ws[24:28].view(torch.int32)      # rows served by the exact fallback (generation 4) inside the call
        stats["workspace"] = ws                                   # (tools/check_funnel.py reads the rows' state out of it)
    return out


GEOMETRY_NAMES = {0: "lds", 3: "many", 4: "huge", 7: "funnel"}          # (1, 2, 5, 6: the geometries round 5 removed)


def kernel_identity(word) -> dict:
    """Decodes the word the sweep kernels write at workspace + 16 (stats["kernel_id"]): which kernel generation, geometry and
    template instance a score_topk_keys call actually ran.  Synchronising when given the device tensor.  0 = no pre-filtered
    sweep ran (every split ended inside its warm-up, or generation 1)."""
    w = int(word) & 0xFFFFFFFF
    if w == 0:
        return {"generation": 0}
    return {"generation": w >> 28, "geometry": GEOMETRY_NAMES.get((w >> 8) & 15, "?") if (w >> 28) == 4 else None,
            ("early_stop" if (w >> 28) == 4 else "visiting_order"): bool((w >> 12) & 1), "head": (w >> 13) & 1, "bf16": bool((w >> 14) & 1), "d": (w & 15) * 64}


def huge_image_offsets(nu: int, nloc: int, d: int, n_splits: int):
    """pda_score_topk4_phase_image_offsets -> (byte offsets of the user image, the padded norms and the warm-up rows' K-th values in the
    workspace of a pda_score_topk4_* call, rows of the padded image)."""
    offs = (C.c_size_t * 4)()
    check(_lib.load().pda_score_topk4_phase_image_offsets(nu, nloc, d, n_splits, C.cast(offs, C.c_void_p)), "pda_score_topk4_phase_image_offsets")
    return int(offs[0]), int(offs[1]), int(offs[2]), int(offs[3])


def warm_mask_offsets(nu: int, nloc: int, d: int, n_splits: int):
    """pda_score_topk4_phase_mask_offsets -> (byte offset, bytes) of the warm-position masks warm_mask4_kernel leaves in the workspace of a
    pda_score_topk4_* call: uint32 [128-user tiles x warm-up splits][128][8]."""
    offs = (C.c_size_t * 2)()
    check(_lib.load().pda_score_topk4_phase_mask_offsets(nu, nloc, d, n_splits, C.cast(offs, C.c_void_p)), "pda_score_topk4_phase_mask_offsets")
    return int(offs[0]), int(offs[1])


def warm_mask_rows(prep: torch.Tensor, users: torch.Tensor, hist: "HistoryCSR", item_offset: int, nloc: int, d: int, warm_tiles: int = 4) -> torch.Tensor:
    """pda_score_topk4_phase_mask_rows: warm_mask4_kernel on a block as a call of its own (one warm-up over the front of the whole order)
    -> int32 [block rows padded to whole 128-user tiles, 8]."""
    users = _need(users, torch.int32, "users")
    nu = users.numel()
    out = torch.empty((-(-nu // 128) * 128, 8), dtype=torch.int32, device=users.device)
    check(_lib.load().pda_score_topk4_phase_mask_rows(ptr(prep), ptr(users), nu, item_offset, nloc, d, ptr(hist.indptr), ptr(hist.indices), hist.mode,
                                                      warm_tiles, ptr(out), stream_ptr()), "pda_score_topk4_phase_mask_rows")
    return out


def huge_user_image(U: torch.Tensor, users: torch.Tensor):
    """pda_score_topk4_phase_user_image: the block as a phase-2 sweep of the huge geometry prepares it by itself
    -> (image uint8 [n_pad * 2 d], padded norms float32 [n_pad])."""
    lib = _lib.load()
    bf = U.dtype == torch.bfloat16
    U = _need(U, torch.bfloat16 if bf else torch.float32, "U")
    users = _need(users, torch.int32, "users")
    d, nu = U.shape[1], users.numel()
    ut = 512 if d == 256 else 1024
    n_pad = -(-nu // ut) * ut
    ufrag = torch.empty(n_pad * 2 * d, dtype=torch.uint8, device=U.device)
    unorm = torch.empty(n_pad, dtype=torch.float32, device=U.device)
    check(lib.pda_score_topk4_phase_user_image(ptr(U), 1 if bf else 0, ptr(users), nu, d, ptr(ufrag), ptr(unorm), stream_ptr()),
          "pda_score_topk4_phase_user_image")
    return ufrag, unorm


def funnel_user_image(U: torch.Tensor, users: torch.Tensor):
    """pda_score_topk7_phase_user_image: the block as the funnel prepares it -> (fp16 image uint8 [n_pad * 2 d], padded norms float32 [n_pad],
    padded norms of the rounding residuals float32 [n_pad])."""
    lib = _lib.load()
    bf = U.dtype == torch.bfloat16
    U = _need(U, torch.bfloat16 if bf else torch.float32, "U")
    users = _need(users, torch.int32, "users")
    d, nu = U.shape[1], users.numel()
    ut = 512 if d == 256 else 1024
    n_pad = -(-nu // ut) * ut
    ufrag = torch.empty(n_pad * 2 * d, dtype=torch.uint8, device=U.device)
    unorm = torch.empty(n_pad, dtype=torch.float32, device=U.device)
    uerr = torch.empty(n_pad, dtype=torch.float32, device=U.device)
    check(lib.pda_score_topk7_phase_user_image(ptr(U), 1 if bf else 0, ptr(users), nu, d, ptr(ufrag), ptr(unorm), ptr(uerr), stream_ptr()),
          "pda_score_topk7_phase_user_image")
    return ufrag, unorm, uerr


def _bloom_out(users: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
    if out is None:
        return torch.empty((users.numel(), 32), dtype=torch.int32, device=users.device)
    out = _need(out, torch.int32, "out")
    if out.dim() != 2 or out.shape[1] != 32 or out.shape[0] < users.numel():
        raise ValueError("out must be int32 [at least the block's rows, 32]")
    return out


def hist_bloom_rows(prep: torch.Tensor, users: torch.Tensor, hist: "HistoryCSR", skip_if_ordered: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pda_score_topk4_phase_bloom_rows: hist_bloom4_kernel on a block as a call of its own -> int32 [block rows, 32], the 1 024-bit Bloom filter
    of every row's train-item ids.  out: the caller's buffer (rows beyond the block, and every row where skip_if_ordered applies, stay as they are)."""
    users = _need(users, torch.int32, "users")
    out = _bloom_out(users, out)
    check(_lib.load().pda_score_topk4_phase_bloom_rows(ptr(prep), ptr(users), users.numel(), ptr(hist.indptr), ptr(hist.indices), hist.mode,
                                                       1 if skip_if_ordered else 0, ptr(out), stream_ptr()), "pda_score_topk4_phase_bloom_rows")
    return out


def funnel_bloom_rows(prep7: torch.Tensor, users: torch.Tensor, hist: "HistoryCSR", item_offset: int, nloc: int, d: int,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pda_score_topk7_phase_bloom_rows: hist_bloom7_kernel on a block as a call of its own -> int32 [block rows, 32], the Bloom filter of the
    visiting positions (prep7's) of every row's train items inside the shard."""
    users = _need(users, torch.int32, "users")
    out = _bloom_out(users, out)
    check(_lib.load().pda_score_topk7_phase_bloom_rows(ptr(prep7), ptr(users), users.numel(), item_offset, nloc, d, ptr(hist.indptr), ptr(hist.indices),
                                                       hist.mode, ptr(out), stream_ptr()), "pda_score_topk7_phase_bloom_rows")
    return out


def topk_merge(keys: torch.Tensor, users=None, hist: Optional[HistoryCSR] = None, want="idx_val"):
    """pda_topk_merge.  keys int64[R, Bu, K].  want: 'keys' -> int64[Bu,K];  'idx_val' -> (int32, float32)."""
    lib = _lib.load()
    keys = _need(keys, torch.int64, "keys")
    R, nu, K = keys.shape
    dev = keys.device
    out_keys = out_idx = out_val = None
    if want == "keys":
        out_keys = torch.empty((nu, K), dtype=torch.int64, device=dev)
    else:
        out_idx = torch.empty((nu, K), dtype=torch.int32, device=dev)
        out_val = torch.empty((nu, K), dtype=torch.float32, device=dev)
    if users is not None:
        users = _need(users, torch.int32, "users")
    if hist is not None and hist.indices.numel() == 0:
        hist = None
    check(lib.pda_topk_merge(ptr(keys), R, nu, K, ptr(out_keys), ptr(out_idx), ptr(out_val), ptr(users),
                             ptr(hist.indptr) if hist else None, ptr(hist.indices) if hist else None,
                             hist.mode if hist else 0, stream_ptr()), "pda_topk_merge")
    return out_keys if want == "keys" else (out_idx, out_val)


def recommend_topk(U, I_shard, users, K=50, head=HEAD_RAW, pop_shard=None, hist=None, item_offset=0,
                   n_splits=0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Single-GPU convenience: score + mask + top-K + split merge -> (idx int32[Bu,K], val f32[Bu,K])."""
    keys = score_topk_keys(U, I_shard, users, K, head, pop_shard, hist, item_offset, n_splits)
    return topk_merge(keys, users, hist, want="idx_val")


def bpr_step(U, I, users, pos, neg, pos_pop=None, neg_pop=None, *, regs: float, reg_div: float, lr: float = 0.0,
             mode: int = UPD_NONE, grads_out=None, gU=None, gI=None, loss_acc: Optional[torch.Tensor] = None,
             grouped: bool = False, users_distinct: bool = False):
    """pda_bpr_step_f32.  grads_out = (g_user, g_pos, g_neg) float32 [B,d] or None.  grouped: the batch went through
    group_triplets_by_pos / sort_triplets_by_pos (equal positives adjacent); otherwise PDA_UPD_ANY_ORDER is set.
    users_distinct: the caller's assertion that no user id repeats in the batch (the sampler contract, pda_amd.sampler
    .distinct_users): PDA_UPD_USERS_DISTINCT, the fused step's user rows take plain stores instead of atomics."""
    lib = _lib.load()
    U = _need(U, torch.float32, "U")
    I = _need(I, torch.float32, "I")
    users, pos, neg = (_need(t, torch.int32, n) for t, n in ((users, "users"), (pos, "pos"), (neg, "neg")))
    pos_pop = _need(pos_pop, torch.float32, "pos_pop", optional=True)
    neg_pop = _need(neg_pop, torch.float32, "neg_pop", optional=True)
    B, d = users.numel(), U.shape[1]
    if pos.numel() != B or neg.numel() != B:
        raise ValueError("users/pos/neg must have the same length")
    gu = gp = gn = None
    if grads_out is not None:
        gu, gp, gn = (_need(t, torch.float32, "grads_out") for t in grads_out)
    gU = _need(gU, torch.float32, "gU", optional=True)
    gI = _need(gI, torch.float32, "gI", optional=True)
    loss_acc = _need(loss_acc, torch.float32, "loss_acc", optional=True)
    check(lib.pda_bpr_step_f32(ptr(U), ptr(I), ptr(users), ptr(pos), ptr(neg), ptr(pos_pop), ptr(neg_pop), B, d,
                               float(regs), float(reg_div), float(lr),
                               mode | (0 if grouped else UPD_ANY_ORDER) | (UPD_USERS_DISTINCT if users_distinct and mode == UPD_SGD_FUSED else 0),
                               ptr(gu), ptr(gp), ptr(gn), ptr(gU), ptr(gI), ptr(loss_acc), stream_ptr()), "pda_bpr_step_f32")
    if mode == UPD_SGD_FUSED:
        mark_modified(U, I)


def sgd_step_exact(U, I, users, pos, neg, pos_pop=None, neg_pop=None, *, regs: float, reg_div: float, lr: float,
                   loss_acc: Optional[torch.Tensor] = None, scratch=None):
    """The exact mini-batch SGD step: pda_bpr_step_f32(PDA_UPD_NONE) writes the per-occurrence gradients of the whole batch
    against the unchanged tables, pda_sgd_apply_f32 scatters them.  `scratch` = (g_user, g_pos, g_neg) float32 [B, d] to
    reuse between steps (allocated when None).  Returns the scratch tuple."""
    lib = _lib.load()
    B, d = users.numel(), U.shape[1]
    if scratch is None:
        scratch = tuple(torch.empty((B, d), dtype=torch.float32, device=U.device) for _ in range(3))
    bpr_step(U, I, users, pos, neg, pos_pop, neg_pop, regs=regs, reg_div=reg_div, mode=UPD_NONE, grads_out=scratch, loss_acc=loss_acc)
    check(lib.pda_sgd_apply_f32(ptr(U), ptr(I), ptr(users), ptr(pos), ptr(neg), ptr(scratch[0]), ptr(scratch[1]), ptr(scratch[2]),
                                B, d, float(lr), stream_ptr()), "pda_sgd_apply_f32")
    mark_modified(U, I)
    return scratch


PLAN_LDS_MAX_B = 4096     # pda_triplet_plan sorts a batch inside one workgroup's LDS up to here
_PLAN_WS = {}


def triplet_plan_bytes(B: int) -> int:
    return _lib.load().pda_triplet_plan_bytes(B)


def triplet_plan(users, pos, neg, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pda_triplet_plan: users / pos / neg int32 [B] or [n, B] -> uint8 [n, pda_triplet_plan_bytes(B)] (one plan per batch; the
    plan of batch j is out[j]).  B <= 4096: one workgroup per batch; larger batches: pda_triplet_plan_large, a device-wide sort
    per batch (same plan bytes)."""
    lib = _lib.load()
    users, pos, neg = (_need(t, torch.int32, n) for t, n in ((users, "users"), (pos, "pos"), (neg, "neg")))
    B = users.shape[-1]
    n = users.numel() // B
    nb = lib.pda_triplet_plan_bytes(B)
    if out is None:
        out = torch.empty((n, nb), dtype=torch.uint8, device=users.device)
    elif out.shape != (n, nb) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("out must be contiguous uint8 [n_batches, pda_triplet_plan_bytes(B)]")
    if B > PLAN_LDS_MAX_B:
        key = (B, users.device)
        ws = _PLAN_WS.get(key)
        if ws is None:
            ws = _PLAN_WS[key] = torch.empty(lib.pda_triplet_plan_large_workspace_bytes(B), dtype=torch.uint8, device=users.device)
        u2, p2, n2 = users.reshape(n, B), pos.reshape(n, B), neg.reshape(n, B)
        for j in range(n):
            check(lib.pda_triplet_plan_large(ptr(u2[j]), ptr(p2[j]), ptr(n2[j]), B, ptr(out[j]), ptr(ws), stream_ptr()), "pda_triplet_plan_large")
        return out
    check(lib.pda_triplet_plan(ptr(users), ptr(pos), ptr(neg), B, n, ptr(out), stream_ptr()), "pda_triplet_plan")
    return out


def plan_header(plan: torch.Tensor):
    """Host view of a plan's header (synchronising; tests and diagnostics): (segments, a user occurs twice, 2B, B)."""
    return tuple(int(x) for x in plan.reshape(-1)[:16].view(torch.int32).cpu())


def bpr_step_plan(U, I, users, pos, neg, pos_pop=None, neg_pop=None, *, regs: float, reg_div: float, lr: float, plan: torch.Tensor,
                  scratch: Optional[torch.Tensor] = None, exact: bool = True, loss_acc: Optional[torch.Tensor] = None,
                  U_master=None, I_master=None) -> Optional[torch.Tensor]:
    """pda_bpr_step_plan_f32 / _bf16 (U, I bf16 with fp32 U_master / I_master): the exact mini-batch SGD step of a batch with
    DISTINCT users, two launches, no atomics (exact=False: one launch, plain stores on user rows and once-referenced item rows,
    atomics on shared item rows; fp32 tables only).  plan = triplet_plan(users, pos, neg)[j].  Returns the scratch buffer for reuse."""
    lib = _lib.load()
    bf = U.dtype == torch.bfloat16
    users, pos, neg = (_need(t, torch.int32, n) for t, n in ((users, "users"), (pos, "pos"), (neg, "neg")))
    pos_pop = _need(pos_pop, torch.float32, "pos_pop", optional=True)
    neg_pop = _need(neg_pop, torch.float32, "neg_pop", optional=True)
    plan = _need(plan, torch.uint8, "plan")
    B, d = users.numel(), U.shape[1]
    if plan.numel() != lib.pda_triplet_plan_bytes(B):
        raise ValueError("plan does not belong to a batch of %d triplets" % B)
    if exact:
        ns = lib.pda_bpr_step_plan_scratch_bytes(B, d) // 4
        if scratch is None or scratch.numel() != ns:
            scratch = torch.empty(ns, dtype=torch.float32, device=U.device)
    loss_acc = _need(loss_acc, torch.float32, "loss_acc", optional=True)
    if bf:
        U, I = _need(U, torch.bfloat16, "U"), _need(I, torch.bfloat16, "I")
        U_master, I_master = _need(U_master, torch.float32, "U_master"), _need(I_master, torch.float32, "I_master")
        if not exact:
            raise ValueError("bf16 tables take the exact planned step only")
        check(lib.pda_bpr_step_plan_bf16(ptr(U), ptr(I), ptr(U_master), ptr(I_master), ptr(users), ptr(pos), ptr(neg), ptr(pos_pop), ptr(neg_pop),
                                         B, d, float(regs), float(reg_div), float(lr), ptr(plan), ptr(scratch), ptr(loss_acc), stream_ptr()),
              "pda_bpr_step_plan_bf16")
        mark_modified(U, I, U_master, I_master)
    else:
        U, I = _need(U, torch.float32, "U"), _need(I, torch.float32, "I")
        check(lib.pda_bpr_step_plan_f32(ptr(U), ptr(I), ptr(users), ptr(pos), ptr(neg), ptr(pos_pop), ptr(neg_pop), B, d, float(regs),
                                        float(reg_div), float(lr), ptr(plan), ptr(scratch), 1 if exact else 0, ptr(loss_acc), stream_ptr()),
              "pda_bpr_step_plan_f32")
        mark_modified(U, I)
    return scratch


def bpr_step_bf16(U16, I16, users, pos, neg, pos_pop=None, neg_pop=None, *, regs: float, reg_div: float, lr: float = 0.0,
                  mode: int = UPD_NONE, U_master=None, I_master=None, grads_out=None, gU=None, gI=None,
                  loss_acc: Optional[torch.Tensor] = None, refresh: bool = True):
    """pda_bpr_step_bf16 (+ pda_refresh_rows_bf16 of the touched rows after a fused SGD update)."""
    lib = _lib.load()
    U16 = _need(U16, torch.bfloat16, "U16")
    I16 = _need(I16, torch.bfloat16, "I16")
    users, pos, neg = (_need(t, torch.int32, n) for t, n in ((users, "users"), (pos, "pos"), (neg, "neg")))
    pos_pop = _need(pos_pop, torch.float32, "pos_pop", optional=True)
    neg_pop = _need(neg_pop, torch.float32, "neg_pop", optional=True)
    U_master = _need(U_master, torch.float32, "U_master", optional=True)
    I_master = _need(I_master, torch.float32, "I_master", optional=True)
    B, d = users.numel(), U16.shape[1]
    gu = gp = gn = None
    if grads_out is not None:
        gu, gp, gn = (_need(t, torch.float32, "grads_out") for t in grads_out)
    gU = _need(gU, torch.float32, "gU", optional=True)
    gI = _need(gI, torch.float32, "gI", optional=True)
    loss_acc = _need(loss_acc, torch.float32, "loss_acc", optional=True)
    check(lib.pda_bpr_step_bf16(ptr(U16), ptr(I16), ptr(U_master), ptr(I_master), ptr(users), ptr(pos), ptr(neg), ptr(pos_pop),
                                ptr(neg_pop), B, d, float(regs), float(reg_div), float(lr), mode | UPD_ANY_ORDER, ptr(gu), ptr(gp), ptr(gn),
                                ptr(gU), ptr(gI), ptr(loss_acc), stream_ptr()), "pda_bpr_step_bf16")
    if mode == UPD_SGD_FUSED:
        mark_modified(U_master, I_master)
        if refresh:
            refresh_rows_bf16(U_master, U16, users)
            refresh_rows_bf16(I_master, I16, pos)
            refresh_rows_bf16(I_master, I16, neg)


def refresh_rows_bf16(master, shadow, rows=None):
    """pda_refresh_rows_bf16: shadow[rows] = bf16(master[rows]) (RNE); rows None = the whole table."""
    lib = _lib.load()
    master = _need(master, torch.float32, "master")
    shadow = _need(shadow, torch.bfloat16, "shadow")
    rows = _need(rows, torch.int32, "rows", optional=True)
    n = rows.numel() if rows is not None else master.shape[0]
    check(lib.pda_refresh_rows_bf16(ptr(master), ptr(shadow), ptr(rows), n, master.shape[1], stream_ptr()), "pda_refresh_rows_bf16")
    mark_modified(shadow)


def bpr_step_shard(U, I_shard, item_offset: int, users, pos, neg, pos_pop=None, neg_pop=None, *, regs: float, reg_div: float,
                   mean_div: float, lr: float, g_user: torch.Tensor, loss_acc: Optional[torch.Tensor] = None,
                   gI_shard: Optional[torch.Tensor] = None):
    """pda_bpr_step_shard_f32: one rank's part of an item-parallel SGD step.  pos/neg are GLOBAL ids inside
    [item_offset, item_offset + I_shard.shape[0]); g_user float32 [B_local, >=d] (row stride = g_user.stride(0))."""
    lib = _lib.load()
    U = _need(U, torch.float32, "U")
    I_shard = _need(I_shard, torch.float32, "I_shard")
    users, pos, neg = (_need(t, torch.int32, n) for t, n in ((users, "users"), (pos, "pos"), (neg, "neg")))
    pos_pop = _need(pos_pop, torch.float32, "pos_pop", optional=True)
    neg_pop = _need(neg_pop, torch.float32, "neg_pop", optional=True)
    if g_user.dtype != torch.float32 or not g_user.is_cuda:
        raise ValueError("g_user must be a float32 cuda tensor")
    if loss_acc is not None and (loss_acc.dtype != torch.float32 or not loss_acc.is_cuda or loss_acc.numel() != 3 or loss_acc.stride(0) != 1):
        raise ValueError("loss_acc must be 3 consecutive float32 on the device")
    B, d = users.numel(), U.shape[1]
    if g_user.shape != (B, d) or g_user.stride(1) != 1:
        raise ValueError("g_user must be float32 [B_local, d] with unit inner stride")
    check(lib.pda_bpr_step_shard_f32(ptr(U), ptr(I_shard), int(item_offset), ptr(users), ptr(pos), ptr(neg), ptr(pos_pop),
                                     ptr(neg_pop), B, d, float(regs), float(reg_div), float(mean_div), float(lr),
                                     ptr(g_user), g_user.stride(0), ptr(_need(gI_shard, torch.float32, "gI_shard", optional=True)),
                                     ptr(loss_acc), stream_ptr()), "pda_bpr_step_shard_f32")
    if gI_shard is None:
        mark_modified(I_shard)


def apply_user_grads(U, users, g, lr: float):
    """pda_apply_user_grads_f32: U[users[i]] -= lr * g[i].  g float32 [n, d] whose rows may be strided (a column slice
    of the packed exchange buffer); its storage must start 16-byte aligned."""
    lib = _lib.load()
    U = _need(U, torch.float32, "U")
    users = _need(users, torch.int32, "users")
    if g.dtype != torch.float32 or not g.is_cuda or g.stride(1) != 1:
        raise ValueError("g must be a float32 cuda tensor with unit inner stride")
    n, d = g.shape
    check(lib.pda_apply_user_grads_f32(ptr(U), ptr(users), ptr(g), n, d, g.stride(0), float(lr), stream_ptr()),
          "pda_apply_user_grads_f32")
    mark_modified(U)


def score_dense(U, I, users, head: int, pop=None, items=None) -> torch.Tensor:
    """pda_score_dense_f32: the ratings matrix float32 [len(users), n_items] (batch_ratings / condition_ratings of the reference), every entry
    the exact fmaf chain of the top-K kernels.  items: int32 row ids of I or None (all rows); pop: float32 per returned column."""
    U, I = _need(U, torch.float32, "U"), _need(I, torch.float32, "I")
    users = _need(users, torch.int32, "users")
    items = _need(items, torch.int32, "items", optional=True)
    pop = _need(pop, torch.float32, "pop", optional=True)
    n = I.shape[0] if items is None else items.numel()
    if pop is not None and pop.numel() != n:
        raise ValueError("pop holds one value per returned column")
    out = torch.empty((users.numel(), n), dtype=torch.float32, device=U.device)
    check(_lib.load().pda_score_dense_f32(ptr(U), ptr(I), ptr(pop), ptr(users), users.numel(), ptr(items), n, U.shape[1], int(head), ptr(out), stream_ptr()),
          "pda_score_dense_f32")
    return out


def adam_lr_t(lr: float, t: int, beta1=ADAM_BETA1, beta2=ADAM_BETA2) -> float:
    """lr * sqrt(1-beta2^t) / (1-beta1^t)  [TF-ext AdamOptimizer._apply_sparse_shared]."""
    return lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)


def adam_dense_sweep2(var_a, m_a, v_a, g_a, var_b, m_b, v_b, g_b, lr_t: float, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS):
    """pda_adam_dense_sweep2_f32: the dense-decay Adam sweep over both tables of the model in one launch."""
    lib = _lib.load()
    for t in (var_a, m_a, v_a, g_a, var_b, m_b, v_b, g_b):
        _need(t, torch.float32, "adam state")
    check(lib.pda_adam_dense_sweep2_f32(ptr(var_a), ptr(m_a), ptr(v_a), ptr(g_a), var_a.numel(), ptr(var_b), ptr(m_b), ptr(v_b), ptr(g_b),
                                        var_b.numel(), lr_t, beta1, beta2, eps, stream_ptr()), "pda_adam_dense_sweep2_f32")
    mark_modified(var_a)
    mark_modified(var_b)


def adam_touched_bitmaps(n_users: int, n_items: int, device):
    """Zeroed "touched by this step" bitmaps for adam_mark_rows / adam_dense_sweep3 (one bit per table row)."""
    return (torch.zeros((n_users + 31) // 32, dtype=torch.int32, device=device), torch.zeros((n_items + 31) // 32, dtype=torch.int32, device=device))


def adam_mark_rows(users, pos, neg, touched_u, touched_i):
    """pda_adam_mark_rows: the batch's rows into the bitmaps."""
    if pos.numel() != users.numel() or neg.numel() != users.numel():
        raise ValueError("users/pos/neg must have the same length")
    check(_lib.load().pda_adam_mark_rows(ptr(_need(users, torch.int32, "users")), ptr(_need(pos, torch.int32, "pos")), ptr(_need(neg, torch.int32, "neg")),
                                         users.numel(), ptr(touched_u), ptr(touched_i), stream_ptr()), "pda_adam_mark_rows")


def adam_dense_sweep3(var_a, m_a, v_a, g_a, touched_a, var_b, m_b, v_b, g_b, touched_b, lr_t: float, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS):
    """pda_adam_dense_sweep3_f32: the dense-decay Adam sweep over both tables without reading the gradient tables outside the marked rows
    (bit-identical to adam_dense_sweep2); clears the marks."""
    lib = _lib.load()
    for t in (var_a, m_a, v_a, g_a, var_b, m_b, v_b, g_b):
        _need(t, torch.float32, "adam state")
    check(lib.pda_adam_dense_sweep3_f32(ptr(var_a), ptr(m_a), ptr(v_a), ptr(g_a), var_a.shape[0], ptr(touched_a), ptr(var_b), ptr(m_b), ptr(v_b), ptr(g_b),
                                        var_b.shape[0], ptr(touched_b), var_a.shape[1], lr_t, beta1, beta2, eps, stream_ptr()), "pda_adam_dense_sweep3_f32")
    mark_modified(var_a)
    mark_modified(var_b)


ADAM_CACHE_AUTO, ADAM_CACHE_RESIDENT, ADAM_CACHE_STREAM = 0, 1, 2


def adam_row_tags(n_users: int, n_items: int, device):
    """Zeroed per-row step tags for adam_step / adam_dense_sweep4 (i32 per table row; a row is 'touched by step t' iff its tag == t)."""
    return torch.zeros(n_users, dtype=torch.int32, device=device), torch.zeros(n_items, dtype=torch.int32, device=device)


def adam_step(U, mU, vU, gU, tagU, I, mI, vI, gI, tagI, users, pos, neg, pos_pop=None, neg_pop=None, *, regs: float, reg_div: float, step: int,
              lr_t: float, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS, grouped: bool = False, users_distinct: bool = False,
              cache_policy: int = ADAM_CACHE_AUTO, loss_acc: Optional[torch.Tensor] = None):
    """pda_adam_step_f32: one reference train step (gradients of the batch + TF-1.14 dense-decay Adam over both tables) in two launches.
    step >= 1 is the step number (the tag the touched rows get); gU / gI must be zero off the rows of the running step (they are, when only
    this function writes them)."""
    lib = _lib.load()
    for t in (U, mU, vU, gU, I, mI, vI, gI):
        _need(t, torch.float32, "adam state")
    users, pos, neg = (_need(t, torch.int32, n) for t, n in ((users, "users"), (pos, "pos"), (neg, "neg")))
    tagU, tagI = _need(tagU, torch.int32, "tagU"), _need(tagI, torch.int32, "tagI")
    pos_pop = _need(pos_pop, torch.float32, "pos_pop", optional=True)
    neg_pop = _need(neg_pop, torch.float32, "neg_pop", optional=True)
    B, d = users.numel(), U.shape[1]
    if pos.numel() != B or neg.numel() != B:
        raise ValueError("users/pos/neg must have the same length")
    if tagU.numel() != U.shape[0] or tagI.numel() != I.shape[0]:
        raise ValueError("tagU / tagI hold one int32 per table row")
    loss_acc = _need(loss_acc, torch.float32, "loss_acc", optional=True)
    check(lib.pda_adam_step_f32(ptr(U), ptr(mU), ptr(vU), ptr(gU), ptr(tagU), U.shape[0], ptr(I), ptr(mI), ptr(vI), ptr(gI), ptr(tagI), I.shape[0],
                                ptr(users), ptr(pos), ptr(neg), ptr(pos_pop), ptr(neg_pop), B, d, float(regs), float(reg_div), int(step), float(lr_t),
                                beta1, beta2, eps, (0 if grouped else UPD_ANY_ORDER) | (UPD_USERS_DISTINCT if users_distinct else 0),
                                int(cache_policy), ptr(loss_acc), stream_ptr()), "pda_adam_step_f32")
    mark_modified(U, I)


def adam_dense_sweep4(var_a, m_a, v_a, g_a, tag_a, var_b, m_b, v_b, g_b, tag_b, tag: int, lr_t: float, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS,
                      cache_policy: int = ADAM_CACHE_AUTO):
    """pda_adam_dense_sweep4_f32: the sweep of adam_step alone (the gradients and the tags came from elsewhere)."""
    lib = _lib.load()
    for t in (var_a, m_a, v_a, g_a, var_b, m_b, v_b, g_b):
        _need(t, torch.float32, "adam state")
    check(lib.pda_adam_dense_sweep4_f32(ptr(var_a), ptr(m_a), ptr(v_a), ptr(g_a), var_a.shape[0], ptr(_need(tag_a, torch.int32, "tag_a")), ptr(var_b), ptr(m_b),
                                        ptr(v_b), ptr(g_b), var_b.shape[0], ptr(_need(tag_b, torch.int32, "tag_b")), var_a.shape[1], int(tag), float(lr_t),
                                        beta1, beta2, eps, int(cache_policy), stream_ptr()), "pda_adam_dense_sweep4_f32")
    mark_modified(var_a)
    mark_modified(var_b)


def _grad_plan_args(U, I, users, pos, neg, pos_pop, neg_pop, plan, scratch):
    """The checks the two planned-gradient entry points share -> (users, pos, neg, pos_pop, neg_pop, plan, scratch, B, d)."""
    lib = _lib.load()
    users, pos, neg = (_need(t, torch.int32, n) for t, n in ((users, "users"), (pos, "pos"), (neg, "neg")))
    pos_pop = _need(pos_pop, torch.float32, "pos_pop", optional=True)
    neg_pop = _need(neg_pop, torch.float32, "neg_pop", optional=True)
    plan = _need(plan, torch.uint8, "plan")
    B, d = users.numel(), U.shape[1]
    if pos.numel() != B or neg.numel() != B:
        raise ValueError("users/pos/neg must have the same length")
    if plan.numel() != lib.pda_triplet_plan_bytes(B):
        raise ValueError("plan does not belong to a batch of %d triplets" % B)
    ns = lib.pda_bpr_grad_plan_scratch_bytes(B, d) // 4
    if scratch is None or scratch.numel() != ns or scratch.dtype != torch.float32:
        scratch = torch.empty(ns, dtype=torch.float32, device=U.device)
    return users, pos, neg, pos_pop, neg_pop, plan, scratch, B, d


def bpr_grad_plan(U, I, users, pos, neg, pos_pop=None, neg_pop=None, *, regs: float, reg_div: float, plan: torch.Tensor, gU, gI, tagU=None, tagI=None,
                  step: int = 0, scratch: Optional[torch.Tensor] = None, loss_acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pda_bpr_grad_plan_f32: the summed gradients of a batch with DISTINCT users into gU / gI, bit-reproducible -- two launches, sums in the
    order of plan = triplet_plan(users, pos, neg)[j], no float atomics.  A drop-in for bpr_step(mode=UPD_DENSE_GRAD); with tagU / tagI the
    touched rows get the tag `step` (adam_dense_sweep4).  A rejected batch (a user occurs twice): loss_acc := NaN, nothing else is written.
    Returns the scratch buffer for reuse."""
    lib = _lib.load()
    for t in (U, I, gU, gI):
        _need(t, torch.float32, "tables / gradient tables")
    if gU.shape != U.shape or gI.shape != I.shape:
        raise ValueError("gU / gI have the shape of the tables")
    if (tagU is None) != (tagI is None):
        raise ValueError("tagU and tagI come together")
    if tagU is not None:
        tagU, tagI = _need(tagU, torch.int32, "tagU"), _need(tagI, torch.int32, "tagI")
        if tagU.numel() != U.shape[0] or tagI.numel() != I.shape[0]:
            raise ValueError("tagU / tagI hold one int32 per table row")
    users, pos, neg, pos_pop, neg_pop, plan, scratch, B, d = _grad_plan_args(U, I, users, pos, neg, pos_pop, neg_pop, plan, scratch)
    loss_acc = _need(loss_acc, torch.float32, "loss_acc", optional=True)
    check(lib.pda_bpr_grad_plan_f32(ptr(U), ptr(I), ptr(users), ptr(pos), ptr(neg), ptr(pos_pop), ptr(neg_pop), B, d, float(regs), float(reg_div),
                                    ptr(plan), ptr(scratch), ptr(gU), ptr(tagU), ptr(gI), ptr(tagI), int(step), ptr(loss_acc), stream_ptr()),
          "pda_bpr_grad_plan_f32")
    return scratch


def adam_step_plan(U, mU, vU, gU, tagU, I, mI, vI, gI, tagI, users, pos, neg, pos_pop=None, neg_pop=None, *, regs: float, reg_div: float, step: int,
                   lr_t: float, plan: torch.Tensor, scratch: Optional[torch.Tensor] = None, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS,
                   cache_policy: int = ADAM_CACHE_AUTO, loss_acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pda_adam_step_plan_f32: adam_step, bit-reproducible -- bpr_grad_plan followed by the tagged sweep (three launches).  The batch's users
    must be distinct (a batch whose plan says otherwise is rejected: loss_acc := NaN, nothing else moves).  Returns the scratch buffer."""
    lib = _lib.load()
    for t in (U, mU, vU, gU, I, mI, vI, gI):
        _need(t, torch.float32, "adam state")
    tagU, tagI = _need(tagU, torch.int32, "tagU"), _need(tagI, torch.int32, "tagI")
    if tagU.numel() != U.shape[0] or tagI.numel() != I.shape[0]:
        raise ValueError("tagU / tagI hold one int32 per table row")
    users, pos, neg, pos_pop, neg_pop, plan, scratch, B, d = _grad_plan_args(U, I, users, pos, neg, pos_pop, neg_pop, plan, scratch)
    loss_acc = _need(loss_acc, torch.float32, "loss_acc", optional=True)
    check(lib.pda_adam_step_plan_f32(ptr(U), ptr(mU), ptr(vU), ptr(gU), ptr(tagU), U.shape[0], ptr(I), ptr(mI), ptr(vI), ptr(gI), ptr(tagI), I.shape[0],
                                     ptr(users), ptr(pos), ptr(neg), ptr(pos_pop), ptr(neg_pop), B, d, float(regs), float(reg_div), int(step),
                                     float(lr_t), beta1, beta2, eps, int(cache_policy), ptr(plan), ptr(scratch), ptr(loss_acc), stream_ptr()),
          "pda_adam_step_plan_f32")
    mark_modified(U, I)
    return scratch


def adam_dense_sweep(var, m, v, g, lr_t: float, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS):
    lib = _lib.load()
    for t, n in ((var, "var"), (m, "m"), (v, "v"), (g, "g")):
        _need(t, torch.float32, n)
    check(lib.pda_adam_dense_sweep_f32(ptr(var), ptr(m), ptr(v), ptr(g), var.numel(), lr_t, beta1, beta2, eps,
                                       stream_ptr()), "pda_adam_dense_sweep_f32")
    mark_modified(var)


def adam_rows(var, m, v, g, rows, lr_t: float, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS):
    lib = _lib.load()
    rows = _need(rows, torch.int32, "rows")
    check(lib.pda_adam_rows_f32(ptr(var), ptr(m), ptr(v), ptr(g), ptr(rows), rows.numel(), var.shape[1], lr_t, beta1,
                                beta2, eps, stream_ptr()), "pda_adam_rows_f32")
    mark_modified(var)


class LazyAdamState:
    """The bookkeeping of the exact lazy dense-decay Adam (pda_adam_lazy_f32): per-row `last` steps and the device table of
    bias-corrected rates lr_tab[k] = float32(adam_lr_t(lr, k)) -- the value the dense sweep receives as its lr_t argument."""

    def __init__(self, n_users: int, n_items: int, lr: float, device, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS, fast: bool = False):
        self.fast = bool(fast)              # PDA_ADAM_REPLAY_FAST: catch-up to 1e-6 instead of bit for bit (see include/pda_hip.h)
        self.lastU = torch.zeros(n_users, dtype=torch.int32, device=device)
        self.lastI = torch.zeros(n_items, dtype=torch.int32, device=device)
        self.lr, self.beta1, self.beta2, self.eps = lr, beta1, beta2, eps
        self.lr_tab = torch.zeros(0, dtype=torch.float32, device=device)
        self.synced = 0                     # the step every row is known to be current for

    def rates(self, t: int) -> torch.Tensor:
        """lr_tab with at least t + 1 entries (grown geometrically; computed in float64 like adam_lr_t, rounded once)."""
        if self.lr_tab.numel() < t + 1:
            # the very doubles the dense path passes as lr_t (adam_lr_t), rounded to float32 once -- as the ctypes call does
            n = max(1024, 2 * (t + 1))
            tab = [0.0] + [adam_lr_t(self.lr, k, self.beta1, self.beta2) for k in range(1, n)]
            self.lr_tab = torch.tensor(tab, dtype=torch.float64).to(torch.float32).to(self.lastU.device)
        return self.lr_tab


def adam_lazy(phase: int, st: LazyAdamState, U, mU, vU, gU, I, mI, vI, gI, users, pos, neg, t: int):
    """pda_adam_lazy_f32: phase 0 = the batch rows up to step t - 1 (before the forward pass of step t), phase 1 = step t on
    the batch rows with their summed gradients (after pda_bpr_step_f32 in PDA_UPD_DENSE_GRAD mode)."""
    lib = _lib.load()
    for x in (U, mU, vU, gU, I, mI, vI, gI):
        _need(x, torch.float32, "adam state")
    for x in (users, pos, neg):
        _need(x, torch.int32, "batch rows")
    tab = st.rates(t)
    check(lib.pda_adam_lazy_f32(phase | (_lib.ADAM_REPLAY_FAST if st.fast else 0), ptr(U), ptr(mU), ptr(vU), ptr(gU), ptr(st.lastU), ptr(I), ptr(mI), ptr(vI), ptr(gI), ptr(st.lastI),
                                ptr(users), ptr(pos), ptr(neg), users.numel(), U.shape[1], t, ptr(tab), st.beta1, st.beta2, st.eps,
                                stream_ptr()), "pda_adam_lazy_f32")
    mark_modified(U)
    mark_modified(I)


def adam_lazy_dev(phase: int, st: LazyAdamState, U, mU, vU, gU, I, mI, vI, gI, users, pos, neg, t_dev: torch.Tensor, parity: int, n_tab: int):
    """pda_adam_lazy_dev_f32: adam_lazy with the step in device memory -- t_dev int32 [2]: slot `parity` is read, phase 1 stores
    t + 1 into slot 1 - parity (the caller alternates the parity from step to step: an even number of steps per captured graph).
    n_tab: steps the rate table must cover (built once, before the capture)."""
    lib = _lib.load()
    for x in (U, mU, vU, gU, I, mI, vI, gI):
        _need(x, torch.float32, "adam state")
    for x in (users, pos, neg):
        _need(x, torch.int32, "batch rows")
    t_dev = _need(t_dev, torch.int32, "t_dev")
    if t_dev.numel() != 2:
        raise ValueError("t_dev must be int32 [2]")
    tab = st.rates(n_tab)
    check(lib.pda_adam_lazy_dev_f32(phase | (_lib.ADAM_REPLAY_FAST if st.fast else 0), ptr(U), ptr(mU), ptr(vU), ptr(gU), ptr(st.lastU), ptr(I), ptr(mI),
                                    ptr(vI), ptr(gI), ptr(st.lastI), ptr(users), ptr(pos), ptr(neg), users.numel(), U.shape[1],
                                    ptr(t_dev[parity:parity + 1]), ptr(t_dev[1 - parity:2 - parity]), ptr(tab), tab.numel(), st.beta1, st.beta2, st.eps,
                                    stream_ptr()), "pda_adam_lazy_dev_f32")
    mark_modified(U)
    mark_modified(I)


def adam_lazy_sync(st: LazyAdamState, U, mU, vU, I, mI, vI, t: int):
    """pda_adam_lazy_sync_f32 on both tables: every row current for step t (a no-op when nothing is behind)."""
    if st.synced >= t:
        return
    lib = _lib.load()
    tab = st.rates(t)
    fn = lib.pda_adam_lazy_sync_fast_f32 if st.fast else lib.pda_adam_lazy_sync_f32
    for var, m, v, last in ((U, mU, vU, st.lastU), (I, mI, vI, st.lastI)):
        check(fn(ptr(var), ptr(m), ptr(v), ptr(last), var.shape[0], var.shape[1], t, ptr(tab), st.beta1, st.beta2,
                                         st.eps, stream_ptr()), "pda_adam_lazy_sync_f32")
        mark_modified(var)
    st.synced = t


def _metrics_targets(tgt_indices):
    """The target entries of a metrics call.  A block in which no row has a target is an empty tensor, whose null pointer the library refuses:
    it gets one entry that no row reads, and the kernel adds the zeros such rows add."""
    tgt_indices = _need(tgt_indices, torch.int32, "tgt_indices")
    return tgt_indices if tgt_indices.numel() else tgt_indices.new_zeros(1)


def metrics_route(k_cols: int, ordered: bool = False):
    """The entry point that reduces lists of k_cols columns: pda_metrics keeps a 64-bit hit mask, so up to _lib.MAX_K columns go to
    metrics_sums / metrics_sums_ordered and longer lists (--topk_max) to the deep pair."""
    if k_cols > _lib.MAX_K:
        return metrics_sums_deep_ordered if ordered else metrics_sums_deep
    return metrics_sums_ordered if ordered else metrics_sums


def metrics_sums(topk, tgt_indptr, tgt_indices, Ks, sums: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pda_metrics: float64 [4, len(Ks)] sums of precision, recall, ndcg, hit over the rows (added to `sums`).  Ks: int32 on the device, every
    one >= 1 (used_metric.check_ks checks them while they are a host list: the kernel divides by min(K, columns))."""
    lib = _lib.load()
    topk = _need(topk, torch.int32, "topk")
    tgt_indptr = _need(tgt_indptr, torch.int64, "tgt_indptr")
    tgt_indices = _metrics_targets(tgt_indices)
    Ks = _need(Ks, torch.int32, "Ks")
    if sums is None:
        sums = torch.zeros((4, Ks.numel()), dtype=torch.float64, device=topk.device)
    check(lib.pda_metrics(ptr(topk), topk.shape[0], topk.shape[1], ptr(tgt_indptr), ptr(tgt_indices), ptr(Ks),
                          Ks.numel(), ptr(sums), stream_ptr()), "pda_metrics")
    return sums


_METRICS_WS = {}


def metrics_sums_ordered(topk, tgt_indptr, tgt_indices, Ks, sums: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pda_metrics_ordered: metrics_sums with the waves' partial sums added in a fixed order (no float atomics): the same bits run after run."""
    lib = _lib.load()
    topk = _need(topk, torch.int32, "topk")
    tgt_indptr = _need(tgt_indptr, torch.int64, "tgt_indptr")
    tgt_indices = _metrics_targets(tgt_indices)
    Ks = _need(Ks, torch.int32, "Ks")
    if sums is None:
        sums = torch.zeros((4, Ks.numel()), dtype=torch.float64, device=topk.device)
    nb = lib.pda_metrics_ordered_workspace_bytes(topk.shape[0], Ks.numel())
    ws = _METRICS_WS.get(topk.device)
    if ws is None or ws.numel() * 8 < nb:
        ws = _METRICS_WS[topk.device] = torch.empty(max(1, nb // 8), dtype=torch.float64, device=topk.device)
    check(lib.pda_metrics_ordered(ptr(topk), topk.shape[0], topk.shape[1], ptr(tgt_indptr), ptr(tgt_indices), ptr(Ks), Ks.numel(), ptr(sums),
                                  ptr(ws), stream_ptr()), "pda_metrics_ordered")
    return sums


def sample_triplets(train_indptr, train_indices, B: int, *, seed: int, step: int, users=None, user_pool=None,
                    n_pool: int = 0, train_slots=None, neg_range=(0, 0), pop_matrix=None, sort_by_pos: bool = False):
    """pda_sample_triplets -> (users, pos, neg, pos_pop|None, neg_pop|None), all on device."""
    lib = _lib.load()
    dev = train_indptr.device
    gen = users is None
    if gen:
        users = torch.empty(B, dtype=torch.int32, device=dev)
    pos = torch.empty(B, dtype=torch.int32, device=dev)
    neg = torch.empty(B, dtype=torch.int32, device=dev)
    pp = pn = None
    n_slots = 0
    if pop_matrix is not None:
        pop_matrix = _need(pop_matrix, torch.float32, "pop_matrix")
        n_slots = pop_matrix.shape[1]
        pp = torch.empty(B, dtype=torch.float32, device=dev)
        pn = torch.empty(B, dtype=torch.float32, device=dev)
    check(lib.pda_sample_triplets(ptr(users), int(gen), ptr(user_pool), int(n_pool), B, ptr(train_indptr),
                                  ptr(train_indices), ptr(train_slots), int(neg_range[0]), int(neg_range[1]),
                                  ptr(pop_matrix), n_slots, seed & (2 ** 64 - 1), step, ptr(pos), ptr(neg), ptr(pp),
                                  ptr(pn), stream_ptr()), "pda_sample_triplets")
    if sort_by_pos:
        group_triplets_by_pos(users, pos, neg, pp, pn)
    return users, pos, neg, pp, pn


def _step_slots(step_dev: torch.Tensor, parity: Optional[int]):
    """-> (the slot of the device step counter a sampler reads, the slot that receives step + 1 or None).  parity None: the counter
    is only read.  parity p on a two-slot counter: slot p is read, slot 1 - p written (never the slot other workgroups still read)."""
    if parity is None:
        return step_dev, None
    if step_dev.numel() != 2:
        raise ValueError("parity mode needs a two-slot step counter")
    return step_dev[parity:parity + 1], step_dev[1 - parity:2 - parity]


def sample_triplets_into(out, train_indptr, train_indices, *, seed: int, step_dev: torch.Tensor, user_pool=None, n_pool: int = 0,
                          train_slots=None, neg_range=(0, 0), pop_matrix=None, sort_by_pos: bool = False, advance: bool = True,
                          parity: Optional[int] = None):
    """Graph-capturable sampler: writes one batch into the preallocated `out` = (users, pos, neg, pos_pop|None, neg_pop|None),
    taking the step from device memory.  step_dev int64[1]: read, and with `advance` incremented by a pda_counter_add launch.
    step_dev int64[2] + parity p: the step is read from slot p and step + 1 stored to slot 1 - p by the sampler itself (no
    extra launch); the caller alternates p from call to call (an even number of calls per captured graph)."""
    lib = _lib.load()
    users, pos, neg, pp, pn = out
    n_slots = pop_matrix.shape[1] if pop_matrix is not None else 0
    src, nxt = _step_slots(step_dev, parity)
    check(lib.pda_sample_triplets_dev(ptr(users), 1, ptr(user_pool), int(n_pool), users.numel(), ptr(train_indptr),
                                      ptr(train_indices), ptr(train_slots), int(neg_range[0]), int(neg_range[1]),
                                      ptr(pop_matrix), n_slots, seed & (2 ** 64 - 1), ptr(src), ptr(nxt) if advance else None,
                                      ptr(pos), ptr(neg), ptr(pp), ptr(pn), stream_ptr()), "pda_sample_triplets_dev")
    if sort_by_pos:
        group_triplets_by_pos(users, pos, neg, pp, pn)
    if advance and parity is None:
        check(lib.pda_counter_add(ptr(step_dev), 1, stream_ptr()), "pda_counter_add")
    return out


def sample_batches_into(out, train_indptr, train_indices, *, seed: int, step_dev: torch.Tensor, parity: int, user_pool=None, n_pool: int = 0,
                        train_slots=None, neg_range=(0, 0), pop_matrix=None, group_by_pos: bool = False):
    """pda_sample_batches_dev: `out` = (users, pos, neg, pos_pop|None, neg_pop|None) as [n, B] tensors; row j receives the batch
    of step step_dev[parity] + j (bit for bit what sample_triplets_into draws for that step); step_dev[1 - parity] receives
    step + n.  Graph-capturable (alternate `parity` from call to call, an even number of calls per captured graph)."""
    lib = _lib.load()
    users, pos, neg, pp, pn = out
    if users.dim() != 2 or step_dev.numel() != 2:
        raise ValueError("sample_batches_into wants [n, B] buffers and the two-slot step counter")
    n, B = users.shape
    n_slots = pop_matrix.shape[1] if pop_matrix is not None else 0
    check(lib.pda_sample_batches_dev(ptr(users), 1, ptr(user_pool), int(n_pool), B, n, ptr(train_indptr), ptr(train_indices), ptr(train_slots),
                                     int(neg_range[0]), int(neg_range[1]), ptr(pop_matrix), n_slots, seed & (2 ** 64 - 1),
                                     ptr(step_dev[parity:parity + 1]), ptr(step_dev[1 - parity:2 - parity]), ptr(pos), ptr(neg), ptr(pp), ptr(pn),
                                     1 if group_by_pos else 0, stream_ptr()), "pda_sample_batches_dev")
    return out


def bpr_step_and_sample(U, I, users, pos, neg, pos_pop, neg_pop, *, regs: float, reg_div: float, lr: float, next_out,
                        train_indptr, train_indices, seed: int, step_dev: torch.Tensor, parity: int, user_pool=None,
                        n_pool: int = 0, train_slots=None, neg_range=(0, 0), pop_matrix=None, mode: int = UPD_SGD_FUSED,
                        loss_acc: Optional[torch.Tensor] = None, grouped: bool = False):
    """pda_bpr_step_sample_f32: the fused SGD step on (users, pos, neg, ...) and, in spare workgroups of the same launch, the
    sampler of the NEXT batch into `next_out` = (users, pos, neg, pos_pop|None, neg_pop|None) -- a second set of batch
    buffers.  step_dev int64[2] + parity as in sample_triplets_into (slot `parity` is read, 1 - parity receives step + 1).
    Graph-capturable; equivalent to bpr_step followed by sample_triplets_into."""
    lib = _lib.load()
    if step_dev.numel() != 2:
        raise ValueError("bpr_step_and_sample needs the two-slot step counter")
    nu, npos, nneg, npp, npn = next_out
    n_slots = pop_matrix.shape[1] if pop_matrix is not None else 0
    job = _lib.SampleJob(ptr(nu), 1, ptr(user_pool), int(n_pool), nu.numel(), ptr(train_indptr), ptr(train_indices), ptr(train_slots),
                         int(neg_range[0]), int(neg_range[1]), ptr(pop_matrix), n_slots, seed & (2 ** 64 - 1),
                         ptr(step_dev[parity:parity + 1]), ptr(step_dev[1 - parity:2 - parity]), ptr(npos), ptr(nneg), ptr(npp), ptr(npn))
    if loss_acc is None:
        loss_acc = torch.zeros(3, dtype=torch.float32, device=U.device)
    m = int(mode) | (0 if grouped else UPD_ANY_ORDER)
    check(lib.pda_bpr_step_sample_f32(ptr(U), ptr(I), ptr(users), ptr(pos), ptr(neg), ptr(pos_pop), ptr(neg_pop), users.numel(),
                                      U.shape[1], float(regs), float(reg_div), float(lr), m, ptr(loss_acc), C.byref(job), stream_ptr()),
          "pda_bpr_step_sample_f32")
    return loss_acc


def bpr_train_steps(U, I, bufs, n_steps: int, *, regs: float, reg_div: float, lr: float, train_indptr, train_indices, seed: int,
                    step_ctr: torch.Tensor, user_pool=None, n_pool: int = 0, train_slots=None, neg_range=(0, 0), pop_matrix=None,
                    loss_acc: Optional[torch.Tensor] = None, loss_steps: Optional[torch.Tensor] = None, grouped: bool = False,
                    barrier_ws: Optional[torch.Tensor] = None):
    """pda_bpr_train_steps_f32: n_steps fused SGD steps in one launch.  bufs = two sets (users, pos, neg, pos_pop|None,
    neg_pop|None) of batch buffers; set 0 holds the first batch, set n_steps & 1 the next one afterwards.  step_ctr int64[1]
    (device): the sampler step of the first batch drawn inside, advanced by n_steps.  Returns (loss tensor, barrier_ws) --
    barrier_ws[1] != 0 (checked by the caller when it next synchronises) means the loop was abandoned."""
    lib = _lib.load()
    n_slots = pop_matrix.shape[1] if pop_matrix is not None else 0
    jobs = []
    for (nu, npos, nneg, npp, npn) in bufs:
        jobs.append(_lib.SampleJob(ptr(nu), 1, ptr(user_pool), int(n_pool), nu.numel(), ptr(train_indptr), ptr(train_indices), ptr(train_slots),
                                   int(neg_range[0]), int(neg_range[1]), ptr(pop_matrix), n_slots, seed & (2 ** 64 - 1), None, None,
                                   ptr(npos), ptr(nneg), ptr(npp), ptr(npn)))
    if loss_acc is None and loss_steps is None:
        loss_acc = torch.zeros(3, dtype=torch.float32, device=U.device)
    if barrier_ws is None:
        barrier_ws = torch.zeros(2, dtype=torch.int32, device=U.device)
    if step_ctr.dtype != torch.int64 or step_ctr.numel() != 1:
        raise ValueError("step_ctr must be int64[1] on the device")
    m = int(UPD_SGD_FUSED) | (0 if grouped else UPD_ANY_ORDER)
    check(lib.pda_bpr_train_steps_f32(ptr(U), ptr(I), U.shape[1], float(regs), float(reg_div), float(lr), m, C.byref(jobs[0]), C.byref(jobs[1]),
                                      ptr(step_ctr), int(n_steps), ptr(loss_acc), ptr(loss_steps), ptr(barrier_ws), stream_ptr()),
          "pda_bpr_train_steps_f32")
    mark_modified(U)
    mark_modified(I)
    return (loss_steps if loss_steps is not None else loss_acc), barrier_ws


def group_triplets_by_pos(users, pos, neg, pos_pop=None, neg_pop=None):
    """pda_group_triplets_by_pos (in place): equal positives become contiguous.  Batches above 4096 triplets are left alone."""
    lib = _lib.load()
    if users.numel() > 4096:
        return
    check(lib.pda_group_triplets_by_pos(ptr(users), ptr(pos), ptr(neg), ptr(pos_pop), ptr(neg_pop), users.numel(), stream_ptr()),
          "pda_group_triplets_by_pos")


def sort_triplets_by_pos(users, pos, neg, pos_pop=None, neg_pop=None):
    """pda_sort_triplets_by_pos (in place).  Batches above 4096 triplets are left as they are."""
    lib = _lib.load()
    if users.numel() > 4096:
        return
    check(lib.pda_sort_triplets_by_pos(ptr(users), ptr(pos), ptr(neg), ptr(pos_pop), ptr(neg_pop), users.numel(), stream_ptr()),
          "pda_sort_triplets_by_pos")


def measured_peaks(device=None, mfma_iters: int = 4000, copy_mb: int = 1024) -> dict:
    """pda_peak_mfma_bf16 / pda_peak_copy timed with HIP events (best of 3): the roofs of THIS box, beside the datasheet's."""
    lib = _lib.load()
    dev = device or torch.device("cuda")
    sink = torch.zeros(4, dtype=torch.float32, device=dev)
    n = copy_mb * (1 << 20) // 4
    src, dst = torch.ones(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    best_mfma = best_copy = float("inf")
    for _ in range(4):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        check(lib.pda_peak_mfma_bf16(ptr(sink), mfma_iters, stream_ptr()), "pda_peak_mfma_bf16")
        e[1].record()
        check(lib.pda_peak_copy(ptr(src), ptr(dst), n, stream_ptr()), "pda_peak_copy")
        e[2].record()
        torch.cuda.synchronize()
        best_mfma, best_copy = min(best_mfma, e[0].elapsed_time(e[1])), min(best_copy, e[1].elapsed_time(e[2]))
    # the same register-operand loop with every operand 1.0, and the sweep's own kind of loop (B from the LDS, tiles by LDS-DMA)
    # on random and on constant bf16 rows: the second data points behind `peak_measured`
    best_const = best_lds = best_lds_const = float("inf")
    n_blk = 3000
    nb = (n_blk + 1024) * 19456
    rows = torch.randint(-(1 << 15), (1 << 15) - 1, (nb // 2,), dtype=torch.int16, device=dev)
    rows = ((rows & 0x7F) | ((0x3B + (torch.arange(nb // 2, device=dev, dtype=torch.int16) & 3)) << 7) | (rows & -0x8000)).contiguous()   # |x| ~ 0.1 .. 1
    rows_c = torch.full_like(rows, 0x3C00)
    scratch = torch.zeros(4, dtype=torch.int32, device=dev)
    for _ in range(3):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        check(lib.pda_peak_mfma_bf16_const(ptr(sink), mfma_iters, stream_ptr()), "pda_peak_mfma_bf16_const")
        e[1].record()
        check(lib.pda_peak_mfma_lds_bf16(ptr(rows), nb, ptr(scratch), n_blk, stream_ptr()), "pda_peak_mfma_lds_bf16")
        e[2].record()
        check(lib.pda_peak_mfma_lds_bf16(ptr(rows_c), nb, ptr(scratch), n_blk, stream_ptr()), "pda_peak_mfma_lds_bf16")
        e[3].record()
        torch.cuda.synchronize()
        best_const = min(best_const, e[0].elapsed_time(e[1]))
        best_lds, best_lds_const = min(best_lds, e[1].elapsed_time(e[2])), min(best_lds_const, e[2].elapsed_time(e[3]))
    lds_fl = lib.pda_peak_mfma_lds_flops_per_launch(n_blk)
    return {"bf16_mfma_TFLOPs": lib.pda_peak_mfma_flops_per_launch(mfma_iters) / (best_mfma * 1e-3) / 1e12,
            "bf16_mfma_constant_operands_TFLOPs": lib.pda_peak_mfma_flops_per_launch(mfma_iters) / (best_const * 1e-3) / 1e12,
            "bf16_mfma_lds_fed_TFLOPs": lds_fl / (best_lds * 1e-3) / 1e12,
            "bf16_mfma_lds_fed_constant_rows_TFLOPs": lds_fl / (best_lds_const * 1e-3) / 1e12,
            "hbm_copy_GBs": 2.0 * 4.0 * n / (best_copy * 1e-3) / 1e9,
            "note": "bf16 MFMA: 2 waves per SIMD x 4 accumulator chains, register operands, random mantissas (power-limited clock) / every operand "
                    "1.0; lds_fed: the sweep's own block statement -- B from the LDS, one ds_read_b128 per MFMA, four LDS-DMA loader waves streaming "
                    "tiles, no hand-over (executed flops: 18 MFMAs per block, of which 16 algorithmic) on random / constant bf16 rows; "
                    "HBM: float4 copy of %d MiB, read + write bytes" % copy_mb}


def unpack_keys(keys: torch.Tensor):
    """Host-side helper for tests: packed int64 keys -> (idx int64, val float32); empty (0) -> (-1, -inf)."""
    k = keys.cpu().numpy().view("uint64")
    import numpy as np
    hi = (k >> np.uint64(32)).astype(np.uint32)
    lo = (k & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    bits = np.where(hi & np.uint32(0x80000000), hi ^ np.uint32(0x80000000), ~hi).astype(np.uint32)
    val = bits.view(np.float32).copy()
    idx = (np.uint32(0xFFFFFFFF) - lo).astype(np.int64)
    empty = k == 0
    idx[empty] = -1
    val[empty] = -np.inf
    return idx, val


# ---- BPRMF(t)-pop (include/pda_hip_temp_pop.h) ----------------------------------------------------------------------------------------------
HEAD_BIAS = _lib.HEAD_BIAS


class TempPopState:
    """Adam state of the four BPRMF(t)-pop tables: m, v and the dense gradient accumulator of each, and the per-row step tags (a user tag
    covers U and bu, an item tag covers I and C)."""

    def __init__(self, U, I, bu, C):
        z = torch.zeros_like
        self.m = [z(U), z(I), z(bu), z(C)]
        self.v = [z(U), z(I), z(bu), z(C)]
        self.g = [z(U), z(I), z(bu), z(C)]
        self.tagU = torch.zeros(U.shape[0], dtype=torch.int32, device=U.device)
        self.tagI = torch.zeros(I.shape[0], dtype=torch.int32, device=U.device)


def _temp_pop_tables(U, I, bu, C):
    for t, n in ((U, "U"), (I, "I"), (bu, "bu"), (C, "C")):
        _need(t, torch.float32, n)
    if bu.numel() != U.shape[0] or C.dim() != 2 or C.shape[0] != I.shape[0] or C.shape[1] < 2 or U.shape[1] != I.shape[1]:
        raise ValueError("temp_pop tables: U [n_users, d], I [n_items, d], bu [n_users(, 1)], C [n_items, T + 1] with T >= 1")
    return U.shape[1], C.shape[1] - 1


def _temp_pop_batch(users, pos, neg, temps):
    users, pos, neg = (_need(t, torch.int32, n) for t, n in ((users, "users"), (pos, "pos"), (neg, "neg")))
    temps = _need(temps, torch.float32, "temps")
    B = users.numel()
    if pos.numel() != B or neg.numel() != B or temps.numel() != B:
        raise ValueError("users/pos/neg/temps must have the same length")
    return users, pos, neg, temps, B


def temp_pop_grads(U, I, bu, C, users, pos, neg, temps, st: TempPopState, *, regs: float, reg_div: float, step: int,
                   loss_acc: Optional[torch.Tensor] = None):
    """pda_temp_pop_step_f32: the batch's gradients summed into st.g (and the rows tagged with `step`), no update."""
    d, T = _temp_pop_tables(U, I, bu, C)
    users, pos, neg, temps, B = _temp_pop_batch(users, pos, neg, temps)
    loss_acc = _need(loss_acc, torch.float32, "loss_acc", optional=True)
    g = st.g
    check(_lib.load().pda_temp_pop_step_f32(ptr(U), ptr(I), ptr(bu), ptr(C), ptr(users), ptr(pos), ptr(neg), ptr(temps), B, d, T, float(regs),
                                            float(reg_div), ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]), ptr(st.tagU), ptr(st.tagI), int(step),
                                            ptr(loss_acc), stream_ptr()), "pda_temp_pop_step_f32")


def temp_pop_sweep(U, I, bu, C, st: TempPopState, *, step: int, lr_t: float, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS):
    """pda_temp_pop_sweep_f32: TF-1.14 dense-decay Adam over the four tables (g read on the rows tagged `step`, cleared behind)."""
    d, T = _temp_pop_tables(U, I, bu, C)
    m, v, g = st.m, st.v, st.g
    check(_lib.load().pda_temp_pop_sweep_f32(ptr(U), ptr(m[0]), ptr(v[0]), ptr(g[0]), ptr(st.tagU), U.shape[0], ptr(I), ptr(m[1]), ptr(v[1]),
                                             ptr(g[1]), ptr(st.tagI), I.shape[0], ptr(bu), ptr(m[2]), ptr(v[2]), ptr(g[2]), ptr(C), ptr(m[3]),
                                             ptr(v[3]), ptr(g[3]), d, T, int(step), float(lr_t), beta1, beta2, eps, stream_ptr()),
          "pda_temp_pop_sweep_f32")
    mark_modified(U, I, bu, C)


def temp_pop_adam_step(U, I, bu, C, users, pos, neg, temps, st: TempPopState, *, regs: float, reg_div: float, step: int, lr_t: float,
                       beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS, loss_acc: Optional[torch.Tensor] = None):
    """pda_temp_pop_adam_step_f32: one reference BPRMF(t)-pop step (gradients + Adam over the four tables) in two launches."""
    d, T = _temp_pop_tables(U, I, bu, C)
    users, pos, neg, temps, B = _temp_pop_batch(users, pos, neg, temps)
    loss_acc = _need(loss_acc, torch.float32, "loss_acc", optional=True)
    m, v, g = st.m, st.v, st.g
    check(_lib.load().pda_temp_pop_adam_step_f32(ptr(U), ptr(m[0]), ptr(v[0]), ptr(g[0]), ptr(st.tagU), U.shape[0], ptr(I), ptr(m[1]), ptr(v[1]),
                                                 ptr(g[1]), ptr(st.tagI), I.shape[0], ptr(bu), ptr(m[2]), ptr(v[2]), ptr(g[2]), ptr(C), ptr(m[3]),
                                                 ptr(v[3]), ptr(g[3]), ptr(users), ptr(pos), ptr(neg), ptr(temps), B, d, T, float(regs),
                                                 float(reg_div), int(step), float(lr_t), beta1, beta2, eps, ptr(loss_acc), stream_ptr()),
          "pda_temp_pop_adam_step_f32")
    mark_modified(U, I, bu, C)


def score_topk_bias_keys(U, I_shard, users, alpha, beta, K=50, hist: Optional[HistoryCSR] = None, item_offset=0, n_splits=0,
                         stats: Optional[dict] = None) -> torch.Tensor:
    """pda_temp_pop_score_topk_f32: the bias head h = fl(s + fl(alpha_u beta_i)) -> packed keys int64 [n_splits, Bu, K].
    alpha float32 [Bu] per block row, beta float32 [n_items_local].  The library picks the kernel (the pre-filtered one, given the item
    prep, wherever it can run; PDA_TEMP_POP_KERNEL=exact | prefiltered forces one); stats["kernel_id"]: bias_kernel_identity()."""
    lib = _lib.load()
    U, I_shard = _need(U, torch.float32, "U"), _need(I_shard, torch.float32, "I_shard")
    users = _need(users, torch.int32, "users")
    alpha, beta = _need(alpha, torch.float32, "alpha"), _need(beta, torch.float32, "beta")
    nu, nloc, d = users.numel(), I_shard.shape[0], I_shard.shape[1]
    if alpha.numel() != nu or beta.numel() != nloc or U.shape[1] != d:
        raise ValueError("alpha: one value per block row, beta: one per local item row; U and I_shard share the embed dim")
    if hist is not None and hist.indices.numel() == 0:
        hist = None
    if n_splits <= 0:
        n_splits = lib.pda_score_topk_auto_splits(nu, nloc)
    out = torch.empty((n_splits, nu, K), dtype=torch.int64, device=U.device)
    ws = torch.empty(lib.pda_temp_pop_score_workspace_bytes(nu), dtype=torch.uint8, device=U.device)
    prep = item_prep(I_shard)
    check(lib.pda_temp_pop_score_topk_f32(ptr(U), ptr(I_shard), ptr(prep), ptr(alpha), ptr(beta), ptr(users), nu, item_offset, nloc, d,
                                          ptr(hist.indptr) if hist else None, ptr(hist.indices) if hist else None, hist.mode if hist else 0,
                                          K, n_splits, ptr(out), ptr(ws), stream_ptr()), "pda_temp_pop_score_topk_f32")
    if stats is not None:
        stats["kernel_id"] = ws[16:20].view(torch.int32)
    return out


def bias_kernel_identity(word) -> dict:
    """Decodes the identity word of a bias-head score call (stats["kernel_id"] of score_topk_bias_keys)."""
    w = int(word) & 0xFFFFFFFF
    return {"generation": w >> 28, "bias_head": bool((w >> 15) & 1), "d": (w & 15) * 64}


def recommend_topk_bias(U, I_shard, users, alpha, beta, K=50, hist: Optional[HistoryCSR] = None, stats: Optional[dict] = None):
    """Bias-head score + mask + top-K, merged -> (int32 [Bu, K] item ids, float32 [Bu, K] head values)."""
    keys = score_topk_bias_keys(U, I_shard, users, alpha, beta, K, hist, stats=stats)
    return topk_merge(keys, users, hist)


# ---- BPR-PC (include/pda_hip_pc.h) ------------------------------------------------------------------------------------------------------
HEAD_PC = _lib.HEAD_PC
PC_MAX_K = _lib.PC_MAX_K


def _pc_check(I, pop):
    if I is not None and I.dtype == torch.bfloat16:
        raise TypeError("BPR-PC runs on fp32 tables only (bf16 tables are not supported)")
    I = _need(I, torch.float32, "I")
    d = I.shape[1]
    if d not in (64, 128, 256):
        raise ValueError(f"BPR-PC supports embed sizes 64, 128 and 256, not {d}")
    pop = _need(pop, torch.float32, "pop")
    if pop.numel() != I.shape[0]:
        raise ValueError("pop: one value per item of the full catalogue")
    if not bool(torch.isfinite(pop).all()) or not bool((pop > 0).all()):
        raise ValueError("pop must be finite and > 0 (p_i = 1 / pop_i)")
    return I, pop, d


def _pc_finite(name, x):
    if not math.isfinite(float(x)):
        raise ValueError(f"{name} must be finite, got {x}")
    return float(x)


def pc_item_moments(I, pop) -> torch.Tensor:
    """pda_pc_item_moments_f32: float64 [2 d^2 + d + 1] = G (sum v v^T), H (sum p^2 v v^T), h (sum p^2 v), P (sum p^2), p = RN32(1 / pop)."""
    lib = _lib.load()
    I, pop, d = _pc_check(I, pop)
    n = I.shape[0]
    out = torch.empty(2 * d * d + d + 1, dtype=torch.float64, device=I.device)
    ws = torch.empty(lib.pda_pc_moments_workspace_bytes(n, d), dtype=torch.uint8, device=I.device)
    check(lib.pda_pc_item_moments_f32(ptr(I), ptr(pop), n, d, ptr(out), ptr(ws), stream_ptr()), "pda_pc_item_moments_f32")
    return out


def split_moments(mom: torch.Tensor, d: int):
    """-> (G [d, d], H [d, d], h [d], P) views of a pc_item_moments vector."""
    return (mom[:d * d].view(d, d), mom[d * d:2 * d * d].view(d, d), mom[2 * d * d:2 * d * d + d], mom[2 * d * d + d])


def pc_user_stats(U, I, users, pop, beta, hist: Optional[HistoryCSR] = None, moments: Optional[torch.Tensor] = None):
    """pda_pc_user_stats_f32 -> (U_n, U_c, k) float32 [Bu] each: the per-row norms of BPR-PC and k_u = U_n / U_c (0 where n_u or U_c is 0)."""
    lib = _lib.load()
    I, pop, d = _pc_check(I, pop)
    if U is not None and U.dtype == torch.bfloat16:
        raise TypeError("BPR-PC runs on fp32 tables only (bf16 tables are not supported)")
    U = _need(U, torch.float32, "U")
    users = _need(users, torch.int32, "users")
    if U.shape[1] != d:
        raise ValueError("U and I must share the embed dim")
    beta = _pc_finite("beta", beta)
    if moments is None:
        moments = pc_item_moments(I, pop)
    moments = _need(moments, torch.float64, "moments")
    nu = users.numel()
    out = torch.empty((3, nu), dtype=torch.float32, device=U.device)
    if hist is not None and hist.indices.numel() == 0:
        hist = None
    check(lib.pda_pc_user_stats_f32(ptr(U), ptr(I), ptr(pop), ptr(moments), ptr(users), nu, I.shape[0], d,
                                    ptr(hist.indptr) if hist else None, ptr(hist.indices) if hist else None, hist.mode if hist else 0,
                                    beta, ptr(out[0]), ptr(out[1]), ptr(out[2]), stream_ptr()), "pda_pc_user_stats_f32")
    return out[0], out[1], out[2]


def pc_kernel_identity(word) -> dict:
    """Decodes the identity word of a BPR-PC score call (stats["kernel_id"] of recommend_topk_pc)."""
    w = int(word) & 0xFFFFFFFF
    return {"generation": w >> 28, "pc_head": bool((w >> 16) & 1), "d": (w & 15) * 64}


def recommend_topk_pc(U, I, users, pop, scale, alpha, beta, K=50, hist: Optional[HistoryCSR] = None, rows_per_min: int = 2048,
                      stats: Optional[dict] = None):
    """pda_pc_score_topk_f32: BPR-PC's ranking of a block of users over the full catalogue -> (idx int32 [Bu, K], val float32 [Bu, K] = g).
    scale float32 [Bu]: k_u of each row (pc_user_stats); m is the minimum of r over each group of rows_per_min rows.  stats (optional)
    receives "kernel_id" (pc_kernel_identity) and "pc_fallback_rows" (rows the ranking by r could not settle, swept again by g)."""
    lib = _lib.load()
    I, pop, d = _pc_check(I, pop)
    if U is not None and U.dtype == torch.bfloat16:
        raise TypeError("BPR-PC runs on fp32 tables only (bf16 tables are not supported)")
    U = _need(U, torch.float32, "U")
    users = _need(users, torch.int32, "users")
    scale = _need(scale, torch.float32, "scale")
    nu, n = users.numel(), I.shape[0]
    if U.shape[1] != d or scale.numel() != nu:
        raise ValueError("U and I share the embed dim; scale has one value per block row")
    if not 1 <= K <= PC_MAX_K:
        raise ValueError(f"BPR-PC needs 1 <= K <= {PC_MAX_K}, got {K}")
    if K > n:
        raise ValueError(f"K = {K} exceeds the catalogue ({n} items)")
    alpha, beta = _pc_finite("alpha", alpha), _pc_finite("beta", beta)
    if int(rows_per_min) < 1:
        raise ValueError("rows_per_min must be >= 1")
    if hist is not None and hist.indices.numel() == 0:
        hist = None
    idx = torch.empty((nu, K), dtype=torch.int32, device=U.device)
    val = torch.empty((nu, K), dtype=torch.float32, device=U.device)
    nbytes = lib.pda_pc_score_workspace_bytes(nu, n, d, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=U.device)        # exactly the reported size (the caching allocator aligns to 512 bytes)
    if ws.data_ptr() % 256:
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=U.device)
    off = (-ws.data_ptr()) % 256
    wsa = ws[off:]
    check(lib.pda_pc_score_topk_f32(ptr(U), ptr(I), ptr(pop), ptr(scale), ptr(users), nu, n, d, ptr(hist.indptr) if hist else None,
                                    ptr(hist.indices) if hist else None, hist.mode if hist else 0, alpha, beta, int(rows_per_min), K,
                                    ptr(idx), ptr(val), ptr(wsa), stream_ptr()), "pda_pc_score_topk_f32")
    if stats is not None:
        stats["kernel_id"] = wsa[16:20].view(torch.int32)
        stats["pc_fallback_rows"] = int(wsa[20:24].view(torch.int32).item())
    return idx, val


# ---- deep lists (include/pda_hip_deep.h) ------------------------------------------------------------------------------------------------
DEEP_MAX_K = _lib.DEEP_MAX_K
DEEP_GENERATION = 8                      # generation tag of the deep path in its identity word
DEEP_WORKSPACE_BUDGET = 1 << 30          # bytes of workspace a recommend_topk_deep call may hold at a time: the users are chunked to stay within it
_DEEP_WS = {}                            # device -> the workspace of the last call (kept: a 1 GiB allocation per evaluation block is not free)


def deep_workspace_bytes(n_users_blk: int, n_items_local: int, d: int, K: int) -> int:
    return int(_lib.load().pda_deep_topk_workspace_bytes(n_users_blk, n_items_local, d, K))


def deep_kernel_identity(word) -> dict:
    """Decodes the identity word of a deep call (stats["kernel_id"] of recommend_topk_deep): generation 8 = the deep path."""
    w = int(word) & 0xFFFFFFFF
    return {"generation": w >> 28, "head": (w >> 13) & 1, "bf16": bool((w >> 14) & 1), "d": (w & 15) * 64 or 32}


def deep_chunk_users(n_users: int, n_items_local: int, d: int, K: int, budget: Optional[int] = None) -> int:
    """Users per pda_deep_topk_* call so that its workspace stays within `budget` bytes (whole 128-user tiles; at least one tile)."""
    budget = DEEP_WORKSPACE_BUDGET if budget is None else int(budget)
    if deep_workspace_bytes(n_users, n_items_local, d, K) <= budget:
        return n_users
    lo, hi = 1, -(-n_users // 128)        # tiles: the size is non-decreasing in the users
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if deep_workspace_bytes(mid * 128, n_items_local, d, K) <= budget:
            lo = mid
        else:
            hi = mid - 1
    return lo * 128


def recommend_topk_deep(U, I_shard, users, K, head=HEAD_RAW, pop_shard=None, hist: Optional[HistoryCSR] = None, item_offset=0,
                        stats: Optional[dict] = None, want="idx_val", workspace_budget: Optional[int] = None):
    """pda_deep_topk_f32 / _bf16: exact score + mask + top-K for 1 <= K <= 1 024 without the rating matrix -> (idx int32 [Bu, K], val float32
    [Bu, K]), or packed keys int64 [Bu, K] with want="keys".  The users are chunked so that the workspace stays within DEEP_WORKSPACE_BUDGET
    (or workspace_budget) bytes; a history by block row is re-based per chunk.  stats["kernel_id"]: deep_kernel_identity()."""
    lib = _lib.load()
    bf = U is not None and U.dtype == torch.bfloat16
    tdt = torch.bfloat16 if bf else torch.float32
    U, I_shard = _need(U, tdt, "U"), _need(I_shard, tdt, "I_shard")
    users = _need(users, torch.int32, "users")
    pop_shard = _need(pop_shard, torch.float32, "pop_shard", optional=True)
    nu, nloc, d = users.numel(), I_shard.shape[0], I_shard.shape[1]
    K = int(K)
    if U.shape[1] != d:
        raise ValueError("U and I_shard must share the embed dim")
    if d not in (32, 64, 128, 256):
        raise ValueError(f"deep lists support embed sizes 32, 64, 128 and 256, not {d}")
    if not 1 <= K <= DEEP_MAX_K:
        raise ValueError(f"deep lists need 1 <= K <= {DEEP_MAX_K}, got {K}")
    if K > nloc:
        raise ValueError(f"K = {K} exceeds the item shard ({nloc} items)")
    if head not in (HEAD_RAW, HEAD_POP):
        raise ValueError("deep lists rank by the raw head or the popularity head")
    if head == HEAD_POP:
        if pop_shard is None or pop_shard.numel() != nloc:
            raise ValueError("pop_shard must hold one value per local item row")
        _check_pop(pop_shard)
    if nu == 0:
        raise ValueError("empty user block")
    if hist is not None and hist.indices.numel() == 0:
        hist = None
    dev = U.device
    out_keys = out_idx = out_val = None
    if want == "keys":
        out_keys = torch.empty((nu, K), dtype=torch.int64, device=dev)
    else:
        out_idx = torch.empty((nu, K), dtype=torch.int32, device=dev)
        out_val = torch.empty((nu, K), dtype=torch.float32, device=dev)
    chunk = deep_chunk_users(nu, nloc, d, K, workspace_budget)
    nbytes = deep_workspace_bytes(min(chunk, nu), nloc, d, K)
    ws = _DEEP_WS.get(dev)
    if ws is None or ws.numel() < nbytes:
        ws = None
        _DEEP_WS.pop(dev, None)            # (released before the larger one is taken)
        ws = _DEEP_WS[dev] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    fn = lib.pda_deep_topk_bf16 if bf else lib.pda_deep_topk_f32
    for lo in range(0, nu, chunk):
        hi = min(nu, lo + chunk)
        ip = None
        if hist is not None:     # rows by user id: the whole CSR; by block row: the chunk's rows (indptr keeps its absolute offsets)
            ip = hist.indptr if hist.mode == HIST_BY_USER_ID else hist.indptr[lo:hi + 1]
        check(fn(ptr(U), ptr(I_shard), ptr(pop_shard), ptr(users[lo:hi]), hi - lo, int(item_offset), nloc, d, ptr(ip),
                 ptr(hist.indices) if hist else None, hist.mode if hist else 0, K, int(head),
                 ptr(out_keys[lo:hi]) if out_keys is not None else None, ptr(out_idx[lo:hi]) if out_idx is not None else None,
                 ptr(out_val[lo:hi]) if out_val is not None else None, ptr(ws), ws.numel(), stream_ptr()),
              "pda_deep_topk_bf16" if bf else "pda_deep_topk_f32")
    if stats is not None:
        stats["kernel_id"] = ws[16:20].view(torch.int32).clone()
        stats["workspace_bytes"] = nbytes
        stats["chunk_users"] = chunk
    return out_keys if want == "keys" else (out_idx, out_val)


DEEP_MERGE_MAX_KEYS = _lib.DEEP_MERGE_MAX_KEYS      # keys of a row that one pda_deep_merge launch holds in LDS (R * K)


def deep_merge(keys: torch.Tensor, users=None, hist: Optional[HistoryCSR] = None, want="idx_val"):
    """pda_deep_merge: topk_merge for lists of 1 .. 1 024 columns.  keys int64 [R, Bu, K], every list best first, zeros behind its keys, the
    keys of a row distinct across its lists.  want: 'keys' -> int64 [Bu, K]; 'idx_val' -> (int32, float32), a short row completed from the
    user's history row.  More than DEEP_MERGE_MAX_KEYS keys per row are folded: groups of at most 8192 // K lists are merged to keys until
    one launch is left (the order is total: the fold is exact)."""
    lib = _lib.load()
    keys = _need(keys, torch.int64, "keys")
    if keys.dim() != 3:
        raise ValueError("keys must be [R, Bu, K]")
    R, nu, K = keys.shape
    if not 1 <= K <= DEEP_MAX_K:
        raise ValueError(f"deep lists need 1 <= K <= {DEEP_MAX_K}, got {K}")
    if R < 1 or nu < 1:
        raise ValueError("deep_merge needs at least one list and one user")
    dev = keys.device
    if users is not None:
        users = _need(users, torch.int32, "users")
    if hist is not None and hist.indices.numel() == 0:
        hist = None

    def launch(src, out_keys, out_idx, out_val, h):
        check(lib.pda_deep_merge(ptr(src), src.shape[0], nu, K, ptr(out_keys), ptr(out_idx), ptr(out_val), ptr(users),
                                 ptr(h.indptr) if h else None, ptr(h.indices) if h else None, h.mode if h else 0, stream_ptr()),
              "pda_deep_merge")

    group = max(2, DEEP_MERGE_MAX_KEYS // K)           # lists per launch (K > 4 096 does not occur: two lists always fit)
    while keys.shape[0] > group:
        n_groups = -(-keys.shape[0] // group)
        folded = torch.empty((n_groups, nu, K), dtype=torch.int64, device=dev)
        for g in range(n_groups):
            launch(keys[g * group:(g + 1) * group], folded[g], None, None, None)
        keys = folded
    if want == "keys":
        out = torch.empty((nu, K), dtype=torch.int64, device=dev)
        launch(keys, out, None, None, None)
        return out
    out_idx = torch.empty((nu, K), dtype=torch.int32, device=dev)
    out_val = torch.empty((nu, K), dtype=torch.float32, device=dev)
    launch(keys, None, out_idx, out_val, hist)
    return out_idx, out_val


def deep_shard_keys(U, I_shard, users, K, head=HEAD_RAW, pop_shard=None, hist: Optional[HistoryCSR] = None, item_offset=0) -> torch.Tensor:
    """One item shard's share of a deep ranking: packed keys int64 [Bu, K] of the shard's best min(K, n_items_local) unlisted items per user
    (recommend_topk_deep, want="keys"), zeros behind them -- one list of deep_merge.  An empty shard returns all zeros."""
    users = _need(users, torch.int32, "users")
    K = int(K)
    if not 1 <= K <= DEEP_MAX_K:
        raise ValueError(f"deep lists need 1 <= K <= {DEEP_MAX_K}, got {K}")
    nloc = I_shard.shape[0]
    if nloc >= K:
        return recommend_topk_deep(U, I_shard, users, K, head, pop_shard, hist, item_offset, want="keys")
    out = torch.zeros((users.numel(), K), dtype=torch.int64, device=users.device)
    if nloc > 0:
        out[:, :nloc] = recommend_topk_deep(U, I_shard, users, nloc, head, pop_shard, hist, item_offset, want="keys")
    return out


def _metrics_deep(topk, tgt_indptr, tgt_indices, Ks, sums, ordered: bool):
    lib = _lib.load()
    topk = _need(topk, torch.int32, "topk")
    tgt_indptr = _need(tgt_indptr, torch.int64, "tgt_indptr")
    tgt_indices = _metrics_targets(tgt_indices)
    Ks = _need(Ks, torch.int32, "Ks")
    if not 1 <= topk.shape[1] <= DEEP_MAX_K:
        raise ValueError(f"deep metrics take lists of 1 .. {DEEP_MAX_K} columns, got {topk.shape[1]}")
    if sums is None:
        sums = torch.zeros((4, Ks.numel()), dtype=torch.float64, device=topk.device)
    ws = None
    if ordered:
        nb = lib.pda_metrics_deep_workspace_bytes(topk.shape[0], Ks.numel())
        ws = _METRICS_WS.get(topk.device)
        if ws is None or ws.numel() * 8 < nb:
            ws = _METRICS_WS[topk.device] = torch.empty(max(1, nb // 8), dtype=torch.float64, device=topk.device)
    check(lib.pda_metrics_deep(ptr(topk), topk.shape[0], topk.shape[1], ptr(tgt_indptr), ptr(tgt_indices), ptr(Ks), Ks.numel(), ptr(sums),
                               ptr(ws), stream_ptr()), "pda_metrics_deep")
    return sums


def metrics_sums_deep(topk, tgt_indptr, tgt_indices, Ks, sums: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pda_metrics_deep: metrics_sums on lists of up to 1 024 columns (float atomics)."""
    return _metrics_deep(topk, tgt_indptr, tgt_indices, Ks, sums, ordered=False)


def metrics_sums_deep_ordered(topk, tgt_indptr, tgt_indices, Ks, sums: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pda_metrics_deep with a workspace: the ordered reduction of metrics_sums_ordered (the same bits run after run)."""
    return _metrics_deep(topk, tgt_indptr, tgt_indices, Ks, sums, ordered=True)


# ---- xQuAD (include/pda_hip_xquad.h) ----------------------------------------------------------------------------------------------------
XQUAD_MAX_K = _lib.XQUAD_MAX_K
XQUAD_MAX_N = _lib.XQUAD_MAX_N
XQUAD_VARIANTS = {"binary": _lib.XQUAD_BINARY, "smooth": _lib.XQUAD_SMOOTH}


def xquad_rerank(cand_idx, cand_val, item_is_head, lam, K=50, variant="smooth", users=None, hist: Optional[HistoryCSR] = None):
    """pda_xquad_rerank: xQuAD's greedy selection of K out of each row's N candidates -> (idx int32 [Bu, K], val float32 [Bu, K] = x at the pick).
    cand_idx int32 [Bu, N], cand_val float32 [Bu, N]: what every recommend_* call returns (best first; -1 / -inf behind a short row).
    item_is_head uint8 [n_items]: non-zero = short head.  hist: the users' profiles (by user id: `users` int32 [Bu] is needed; by block row:
    row r of the CSR is row r of the candidates); None = no profile, which leaves the candidates' order."""
    lib = _lib.load()
    cand_idx = _need(cand_idx, torch.int32, "cand_idx")
    cand_val = _need(cand_val, torch.float32, "cand_val")
    item_is_head = _need(item_is_head, torch.uint8, "item_is_head")
    users = _need(users, torch.int32, "users", optional=True)
    if cand_idx.dim() != 2 or cand_idx.shape != cand_val.shape:
        raise ValueError("cand_idx and cand_val must be [Bu, N], the same shape")
    if item_is_head.dim() != 1 or item_is_head.numel() < 1:
        raise ValueError("item_is_head holds one byte per item of the catalogue")
    if cand_val.device != cand_idx.device or item_is_head.device != cand_idx.device:
        raise ValueError("cand_idx, cand_val and item_is_head must live on one device")
    nu, N = cand_idx.shape
    K = int(K)
    if nu < 1:
        raise ValueError("empty user block")
    if not 1 <= N <= XQUAD_MAX_N:
        raise ValueError(f"xQuAD takes 1 .. {XQUAD_MAX_N} candidates per user, got {N}")
    if not 1 <= K <= min(XQUAD_MAX_K, N):
        raise ValueError(f"xQuAD needs 1 <= K <= min({XQUAD_MAX_K}, N = {N}), got {K}")
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"lambda must lie in [0, 1], got {lam}")
    if variant not in XQUAD_VARIANTS:
        raise ValueError(f"variant must be 'smooth' or 'binary', not {variant!r}")
    if users is not None and users.numel() != nu:
        raise ValueError("users holds one id per candidate row")
    if hist is not None and hist.indices.numel() == 0:
        hist = None
    if hist is not None:
        if hist.mode == HIST_BY_USER_ID and users is None:
            raise ValueError("a history by user id needs `users`")
        if hist.mode == HIST_BY_BLOCK_ROW and hist.indptr.numel() < nu + 1:
            raise ValueError("a history by block row holds one row per candidate row")
    idx = torch.empty((nu, K), dtype=torch.int32, device=cand_idx.device)
    val = torch.empty((nu, K), dtype=torch.float32, device=cand_idx.device)
    check(lib.pda_xquad_rerank(ptr(cand_idx), ptr(cand_val), nu, N, ptr(item_is_head), item_is_head.numel(), ptr(users),
                               ptr(hist.indptr) if hist else None, ptr(hist.indices) if hist else None, hist.mode if hist else 0,
                               lam, XQUAD_VARIANTS[variant], K, ptr(idx), ptr(val), stream_ptr()), "pda_xquad_rerank")
    return idx, val


# ---- calibrated popularity (include/pda_hip_calib.h) ------------------------------------------------------------------------------------
CALIB_MAX_G = _lib.CALIB_MAX_G
CALIB_MAX_K = _lib.CALIB_MAX_K
CALIB_MAX_N = _lib.CALIB_MAX_N
CALIB_MAX_KS = _lib.CALIB_MAX_KS
CALIB_DIVERGENCES = {"js": _lib.CALIB_JS, "kl": _lib.CALIB_KL}


def _calib_groups(item_group, G, like=None):
    item_group = _need(item_group, torch.uint8, "item_group")
    if item_group.dim() != 1 or item_group.numel() < 1:
        raise ValueError("item_group holds one byte per item of the catalogue")
    if like is not None and item_group.device != like.device:
        raise ValueError("item_group must live on the device of the lists")
    if int(G) != G or not 2 <= int(G) <= CALIB_MAX_G:
        raise ValueError(f"calibration takes 2 .. {CALIB_MAX_G} popularity groups, got {G}")
    return item_group, int(G)


def calib_profile(item_group, G, n_rows, users=None, hist: Optional[HistoryCSR] = None) -> torch.Tensor:
    """pda_calib_profile -> int32 [n_rows, G]: the distinct history entries of each row per popularity group.  item_group uint8 [n_items]
    (0 = the most popular; a byte >= G: no group).  hist by user id: `users` int32 [n_rows] is needed; by block row: row r of the CSR is row r;
    None (or an empty history): all zeros."""
    lib = _lib.load()
    item_group, G = _calib_groups(item_group, G)
    users = _need(users, torch.int32, "users", optional=True)
    n_rows = int(n_rows)
    if n_rows < 1:
        raise ValueError("empty user block")
    if users is not None and users.numel() != n_rows:
        raise ValueError("users holds one id per row")
    if hist is not None and hist.indices.numel() == 0:
        hist = None
    if hist is not None:
        if hist.mode == HIST_BY_USER_ID and users is None:
            raise ValueError("a history by user id needs `users`")
        if hist.mode == HIST_BY_BLOCK_ROW and hist.indptr.numel() < n_rows + 1:
            raise ValueError("a history by block row holds one row per profile row")
    prof = torch.zeros((n_rows, G), dtype=torch.int32, device=item_group.device)
    check(lib.pda_calib_profile(ptr(users), ptr(hist.indptr) if hist else None, ptr(hist.indices) if hist else None, hist.mode if hist else 0,
                                n_rows, ptr(item_group), item_group.numel(), G, ptr(prof), stream_ptr()), "pda_calib_profile")
    return prof


def calib_ks(Ks, K) -> Tuple[int, ...]:
    """The cut-offs of pda_calib_list_counts, checked: 1 .. CALIB_MAX_KS integers, strictly ascending inside 1 .. K."""
    ks = tuple(int(k) for k in Ks)
    if not 1 <= len(ks) <= CALIB_MAX_KS:
        raise ValueError(f"list counts take 1 .. {CALIB_MAX_KS} cut-offs, got {len(ks)}")
    if ks[0] < 1 or ks[-1] > int(K) or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"the cut-offs must ascend strictly inside 1 .. {int(K)} (the columns of the lists), got {list(ks)}")
    return ks


def calib_list_counts(idx, item_group, G, Ks) -> torch.Tensor:
    """pda_calib_list_counts -> int32 [n_rows, len(Ks), G]: the entries of each group among the first Ks[j] columns of idx int32 [n_rows, K]
    (an empty slot, an id outside the catalogue and an item of no group count nowhere)."""
    lib = _lib.load()
    idx = _need(idx, torch.int32, "idx")
    if idx.dim() != 2 or idx.shape[0] < 1 or not 1 <= idx.shape[1] <= CALIB_MAX_N:
        raise ValueError(f"idx must be int32 [n_rows >= 1, 1 .. {CALIB_MAX_N}], got {tuple(idx.shape)}")
    item_group, G = _calib_groups(item_group, G, idx)
    ks = calib_ks(Ks, idx.shape[1])
    cnt = torch.zeros((idx.shape[0], len(ks), G), dtype=torch.int32, device=idx.device)
    check(lib.pda_calib_list_counts(ptr(idx), idx.shape[0], idx.shape[1], ptr(item_group), item_group.numel(), G, (C.c_int32 * len(ks))(*ks),
                                    len(ks), ptr(cnt), stream_ptr()), "pda_calib_list_counts")
    return cnt


def calib_rerank(cand_idx, cand_val, prof, item_group, G, lam, K=50, div="js", alpha=0.01):
    """pda_calib_rerank: the calibrated greedy selection of K out of each row's N candidates -> (idx int32 [Bu, K], val float32 [Bu, K] = x at
    the pick, div float32 [Bu, K] = the divergence of the list's first t + 1 items from the profile, on the 2^-20 grid).  cand_idx int32
    [Bu, N], cand_val float32 [Bu, N]: what every recommend_* call returns (best first; -1 / -inf behind a short row).  prof int32 [Bu, G]:
    calib_profile (all zeros: the candidates' order stays).  div: 'js' (log2) or 'kl' (the list smoothed by alpha)."""
    lib = _lib.load()
    cand_idx = _need(cand_idx, torch.int32, "cand_idx")
    cand_val = _need(cand_val, torch.float32, "cand_val")
    prof = _need(prof, torch.int32, "prof")
    if cand_idx.dim() != 2 or cand_idx.shape != cand_val.shape:
        raise ValueError("cand_idx and cand_val must be [Bu, N], the same shape")
    item_group, G = _calib_groups(item_group, G, cand_idx)
    if cand_val.device != cand_idx.device or prof.device != cand_idx.device:
        raise ValueError("cand_idx, cand_val, prof and item_group must live on one device")
    nu, N = cand_idx.shape
    K = int(K)
    if nu < 1:
        raise ValueError("empty user block")
    if tuple(prof.shape) != (nu, G):
        raise ValueError(f"prof must be int32 [Bu = {nu}, G = {G}], got {tuple(prof.shape)}")
    if not 1 <= N <= CALIB_MAX_N:
        raise ValueError(f"calibration takes 1 .. {CALIB_MAX_N} candidates per user, got {N}")
    if not 1 <= K <= min(CALIB_MAX_K, N):
        raise ValueError(f"calibration needs 1 <= K <= min({CALIB_MAX_K}, N = {N}), got {K}")
    lam, alpha = float(lam), float(alpha)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"lambda must lie in [0, 1], got {lam}")
    if div not in CALIB_DIVERGENCES:
        raise ValueError(f"div must be 'js' or 'kl', not {div!r}")
    if div == "kl" and not 0.0 < alpha < 1.0:
        raise ValueError(f"alpha must lie strictly inside 0 .. 1, got {alpha}")
    idx = torch.full((nu, K), -1, dtype=torch.int32, device=cand_idx.device)
    val = torch.full((nu, K), float("-inf"), dtype=torch.float32, device=cand_idx.device)
    dv = torch.full((nu, K), float("-inf"), dtype=torch.float32, device=cand_idx.device)
    check(lib.pda_calib_rerank(ptr(cand_idx), ptr(cand_val), nu, N, ptr(prof), ptr(item_group), item_group.numel(), G, lam,
                               CALIB_DIVERGENCES[div], alpha, K, ptr(idx), ptr(val), ptr(dv), stream_ptr()), "pda_calib_rerank")
    return idx, val, dv


# ---- item exposure of the lists (include/pda_hip_exposure.h) ------------------------------------------------------------------------------
EXPOSURE_MAX_KS = _lib.EXPOSURE_MAX_KS
EXPOSURE_MAX_COLS = _lib.EXPOSURE_MAX_COLS
_EXPOSURE_KS = {}                        # (Ks, device) -> the cut-offs on the device: one copy per list of cut-offs, not one per block


def exposure_ks(Ks) -> Tuple[int, ...]:
    """The cut-offs of pda_list_exposure, checked: 1 .. EXPOSURE_MAX_KS integers, strictly ascending, the first >= 1."""
    ks = tuple(int(k) for k in Ks)
    if any(k != k0 for k, k0 in zip(ks, Ks)):
        raise ValueError("Ks must be integers, got %r" % (list(Ks),))
    if not 1 <= len(ks) <= EXPOSURE_MAX_KS:
        raise ValueError("pda_list_exposure takes 1 .. %d cut-offs, got %d" % (EXPOSURE_MAX_KS, len(ks)))
    if ks[0] < 1 or any(b <= a for a, b in zip(ks, ks[1:])) or ks[-1] > 0x7FFFFFFF:
        raise ValueError("Ks must be strictly ascending and >= 1, got %r" % (list(ks),))
    return ks


def list_exposure(topk, Ks, n_items, tgt_indptr=None, tgt_indices=None, shown=None, hit=None, plain: bool = False):
    """pda_list_exposure: shown[b][i] += the entries of topk int32 [n, k] in the columns Ks[b-1] <= j < Ks[b] that hold item i, hit[b][i] += those
    that are also in the row's targets (CSR tgt_indptr int64 [n + 1], tgt_indices int32; both None: no hit counts, hit is None)
    -> (shown, hit) int32 [len(Ks), n_items], zeroed here when none are given.  Ks: a host list, strictly ascending.  Ids outside [0, n_items) are
    ignored.  plain: pda_list_exposure_plain, the same result with one global atomic per entry (the measurement's baseline)."""
    lib = _lib.load()
    topk = _need(topk, torch.int32, "topk")
    ks = exposure_ks(Ks)
    n_items = int(n_items)
    if topk.dim() != 2 or topk.shape[0] < 1:
        raise ValueError("topk must be [n_rows >= 1, k_cols]")
    n, k = topk.shape
    if not 1 <= k <= EXPOSURE_MAX_COLS:
        raise ValueError(f"pda_list_exposure takes lists of 1 .. {EXPOSURE_MAX_COLS} columns, got {k}")
    if not 1 <= n_items <= 0x7FFFFFFF:
        raise ValueError(f"n_items must lie in 1 .. 2^31 - 1, got {n_items}")
    if (tgt_indptr is None) != (tgt_indices is None):
        raise ValueError("the targets are tgt_indptr and tgt_indices together, or neither")
    with_hits = tgt_indptr is not None
    if with_hits:
        tgt_indptr = _need(tgt_indptr, torch.int64, "tgt_indptr")
        tgt_indices = _need(tgt_indices, torch.int32, "tgt_indices")
        if tgt_indptr.numel() != n + 1:
            raise ValueError("tgt_indptr holds one row per list (n_rows + 1 entries)")
        if tgt_indices.numel() == 0:            # (every target row empty: the C ABI wants a pointer, and reads nothing through it)
            tgt_indices = tgt_indices.new_zeros(1)
    elif hit is not None:
        raise ValueError("a hit buffer needs the targets")
    dev = topk.device
    for name, buf in (("shown", shown), ("hit", hit)):
        if buf is not None:
            _need(buf, torch.int32, name)
            if tuple(buf.shape) != (len(ks), n_items) or buf.device != dev:
                raise ValueError(f"{name} must be int32 [len(Ks), n_items] on the lists' device")
    if shown is None:
        shown = torch.zeros((len(ks), n_items), dtype=torch.int32, device=dev)
    if with_hits and hit is None:
        hit = torch.zeros((len(ks), n_items), dtype=torch.int32, device=dev)
    ks_dev = _EXPOSURE_KS.get((ks, dev))
    if ks_dev is None:
        ks_dev = _EXPOSURE_KS[(ks, dev)] = torch.as_tensor(ks, dtype=torch.int32, device=dev)
    fn, what = (lib.pda_list_exposure_plain, "pda_list_exposure_plain") if plain else (lib.pda_list_exposure, "pda_list_exposure")
    check(fn(ptr(topk), n, k, n_items, ptr(tgt_indptr), ptr(tgt_indices), ptr(ks_dev), len(ks), ptr(shown), ptr(hit), stream_ptr()), what)
    return shown, hit


# ---- what the checks of the tagged step kernels (DICE, IPS, MACR) repeat ---------------------------------------------------------------------
def _triplet_shapes(method: str, tables: str, sizes, U, I, users, pos, neg, *, halves: int = 1, width_note: str = "", mask=None):
    """fp32 2-D tables of equal width (rows of `halves` embeddings of d floats), d in `sizes`, int32 users/pos/neg (and a uint8 mask, where given)
    of one non-zero length -> (d, B).  `method` stands in front of the messages, `tables` describes the tables."""
    U, I = _need(U, torch.float32, "U"), _need(I, torch.float32, "I")
    if U.dim() != 2 or I.dim() != 2 or U.shape[1] != I.shape[1] or U.shape[1] % halves:
        raise ValueError(f"{method} tables: {tables}")
    d = U.shape[1] // halves
    if d not in sizes:
        raise ValueError(f"{method}: the embedding width d must be one of {sizes}{width_note}, got {d}")
    users, pos, neg = (_need(t, torch.int32, n) for t, n in ((users, "users"), (pos, "pos"), (neg, "neg")))
    names, lens = "users/pos/neg", (pos.numel(), neg.numel())
    if mask is not None:
        names, lens = names + "/mask", lens + (_need(mask, torch.uint8, "mask").numel(),)
    B = users.numel()
    if B < 1 or any(n != B for n in lens):
        raise ValueError(f"{names} must have the same, non-zero length")
    return d, B


def _triplet_ids(method: str, U, I, users, pos, neg, check_ids: bool):
    if check_ids:          # (a host synchronisation: the debugging entry points ask for it, the training loop does not)
        lo = min(int(users.min()), int(pos.min()), int(neg.min()))
        if lo < 0 or int(users.max()) >= U.shape[0] or max(int(pos.max()), int(neg.max())) >= I.shape[0]:
            raise ValueError(f"{method} batch: a user or item id lies outside the tables")


# ---- DICE (include/pda_hip_dice.h) ------------------------------------------------------------------------------------------------------
DICE_EMBED_SIZES = (32, 64, 128)          # d, the width of ONE embedding: the tables' rows are 2 d wide
DICE_DIS_KINDS = {"l1": _lib.DICE_DIS_L1, "l2": _lib.DICE_DIS_L2}
DICE_LOSS_TERMS = 6                       # loss_acc: loss, mf_loss, reg_loss, L_int, L_con, L_dis


def dice_rows_ws(B: int, device) -> torch.Tensor:
    """The row-list workspace of one batch size (pda_dice_rows_ws_words): int32, private to one stream.  Handed over as it comes: pda_dice_step_f32
    clears the counts itself and lists a row before pda_dice_dis_f32 reads it."""
    return torch.empty(int(_lib.load().pda_dice_rows_ws_words(int(B))), dtype=torch.int32, device=device)


class DiceState:
    """Adam state of the two concatenated DICE tables: m, v, the dense gradient accumulators, the per-row step tags and the row lists."""

    def __init__(self, U, I):
        z = torch.zeros_like
        self.mU, self.vU, self.gU, self.mI, self.vI, self.gI = z(U), z(U), z(U), z(I), z(I), z(I)
        self.tagU, self.tagI = adam_row_tags(U.shape[0], I.shape[0], U.device)
        self.rows_ws = None

    def ws(self, B: int) -> torch.Tensor:
        if self.rows_ws is None or self.rows_ws.numel() < 4 + 3 * B:
            self.rows_ws = dice_rows_ws(B, self.gU.device)
        return self.rows_ws


def _dice_check(U, I, users, pos, neg, mask, check_ids: bool):
    d, B = _triplet_shapes("DICE", "U [n_users, 2d] and I [n_items, 2d] (interest columns, then conformity columns)", DICE_EMBED_SIZES, U, I, users,
                           pos, neg, halves=2, width_note=" (rows of 2d floats)", mask=mask)
    _triplet_ids("DICE", U, I, users, pos, neg, check_ids)
    return d, B


def dice_grads(U, I, users, pos, neg, mask, st: DiceState, *, w_int: float, w_con: float, dis_pen: float, dis_loss: str = "l1", regs: float,
               reg_div: float, step: int, loss_acc: Optional[torch.Tensor] = None, check_ids: bool = True):
    """pda_dice_step_f32 + pda_dice_dis_f32: the batch's whole gradient summed into st.gU / st.gI (rows tagged `step`), no update.
    loss_acc float32 [6] += (loss, mf_loss, reg_loss, L_int, L_con, L_dis)."""
    d, B = _dice_check(U, I, users, pos, neg, mask, check_ids)
    if dis_loss not in DICE_DIS_KINDS:
        raise ValueError(f"dis_loss must be 'l1' or 'l2', not {dis_loss!r}")
    loss_acc = _need(loss_acc, torch.float32, "loss_acc", optional=True)
    if loss_acc is not None and loss_acc.numel() < DICE_LOSS_TERMS:
        raise ValueError("DICE loss_acc holds six float32")
    lib, ws = _lib.load(), st.ws(B)
    check(lib.pda_dice_step_f32(ptr(U), ptr(I), U.shape[0], I.shape[0], ptr(users), ptr(pos), ptr(neg), ptr(mask), B, d, float(w_int), float(w_con),
                                float(regs), float(reg_div), ptr(st.gU), ptr(st.gI), ptr(st.tagU), ptr(st.tagI), int(step), ptr(ws), ptr(loss_acc),
                                stream_ptr()), "pda_dice_step_f32")
    check(lib.pda_dice_dis_f32(ptr(U), ptr(I), U.shape[0], I.shape[0], B, d, DICE_DIS_KINDS[dis_loss], float(dis_pen), ptr(st.gU), ptr(st.gI), ptr(ws), ptr(loss_acc),
                               stream_ptr()), "pda_dice_dis_f32")


def dice_adam_step(U, I, users, pos, neg, mask, st: DiceState, *, w_int: float, w_con: float, dis_pen: float, dis_loss: str = "l1", regs: float,
                   reg_div: float, step: int, lr_t: float, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS, cache_policy: int = ADAM_CACHE_AUTO,
                   loss_acc: Optional[torch.Tensor] = None, check_ids: bool = False):
    """pda_dice_adam_step_f32: one DICE train step (gradients, L_dis, TF-1.14 dense-decay Adam over both tables); graph-capturable."""
    d, B = _dice_check(U, I, users, pos, neg, mask, check_ids)
    if dis_loss not in DICE_DIS_KINDS:
        raise ValueError(f"dis_loss must be 'l1' or 'l2', not {dis_loss!r}")
    loss_acc = _need(loss_acc, torch.float32, "loss_acc", optional=True)
    if loss_acc is not None and loss_acc.numel() < DICE_LOSS_TERMS:
        raise ValueError("DICE loss_acc holds six float32")
    check(_lib.load().pda_dice_adam_step_f32(ptr(U), ptr(st.mU), ptr(st.vU), ptr(st.gU), ptr(st.tagU), U.shape[0], ptr(I), ptr(st.mI), ptr(st.vI),
                                             ptr(st.gI), ptr(st.tagI), I.shape[0], ptr(users), ptr(pos), ptr(neg), ptr(mask), B, d, float(w_int),
                                             float(w_con), DICE_DIS_KINDS[dis_loss], float(dis_pen), float(regs), float(reg_div), int(step),
                                             float(lr_t), beta1, beta2, eps, int(cache_policy), ptr(st.ws(B)), ptr(loss_acc), stream_ptr()),
          "pda_dice_adam_step_f32")
    mark_modified(U, I)


class DicePop:
    """What PNSM reads besides the train CSR: pop int32 [n_items] (train interactions per item), order (items ascending by (pop, id)) and
    sorted_pop = pop[order], built once on the host from the CSR's column ids."""

    def __init__(self, train_indices: torch.Tensor, n_items: int):
        import numpy as np
        idx = train_indices.detach().cpu().numpy().astype(np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= n_items):
            raise ValueError("a train item id lies outside the catalogue")
        pop = np.bincount(idx, minlength=int(n_items)).astype(np.int32)
        order = np.lexsort((np.arange(n_items), pop)).astype(np.int32)
        dev = train_indices.device
        self.n_items = int(n_items)
        self.pop, self.order = torch.from_numpy(pop).to(dev), torch.from_numpy(order).to(dev)
        self.sorted_pop = torch.from_numpy(np.ascontiguousarray(pop[order])).to(dev)


def _dice_sample_out(B, dev, out):
    if out is None:
        return tuple(torch.empty(B, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.int32, torch.uint8))
    users, pos, neg, mask = out
    for t, dt, n in ((users, torch.int32, "users"), (pos, torch.int32, "pos"), (neg, torch.int32, "neg"), (mask, torch.uint8, "mask")):
        if _need(t, dt, n).numel() != B:
            raise ValueError("PNSM output buffers hold one entry per triplet")
    return out


def dice_sample(train_indptr, train_indices, dp: DicePop, B: int, *, margin: float, seed: int, step: int, users=None, user_pool=None,
                n_pool: int = 0):
    """pda_dice_sample -> (users, pos, neg, mask) on the device: PNSM with the users and positives of sample_triplets(seed, step)."""
    if not float(margin) >= 0.0:
        raise ValueError("the PNSM margin must be >= 0")
    gen = users is None
    out = _dice_sample_out(int(B), train_indptr.device, None)
    if not gen:
        out = (_need(users, torch.int32, "users"),) + out[1:]
    check(_lib.load().pda_dice_sample(ptr(out[0]), int(gen), ptr(user_pool), int(n_pool), int(B), ptr(_need(train_indptr, torch.int64, "train_indptr")),
                                      ptr(_need(train_indices, torch.int32, "train_indices")), dp.n_items, ptr(dp.order), ptr(dp.sorted_pop),
                                      ptr(dp.pop), float(margin), seed & (2 ** 64 - 1), int(step), ptr(out[1]), ptr(out[2]), ptr(out[3]),
                                      stream_ptr()), "pda_dice_sample")
    return out


def dice_sample_into(out, train_indptr, train_indices, dp: DicePop, *, margin_dev: torch.Tensor, seed: int, step_dev: torch.Tensor,
                     parity: Optional[int] = None, user_pool=None, n_pool: int = 0):
    """pda_dice_sample_dev: one batch into out = (users, pos, neg, mask), step and margin read from device memory (graph-capturable).
    step_dev int64 [1]: read only.  step_dev int64 [2] + parity p: read from slot p, step + 1 stored to slot 1 - p (sample_triplets_into)."""
    out = _dice_sample_out(out[0].numel(), train_indptr.device, out)
    margin_dev = _need(margin_dev, torch.float32, "margin_dev")
    src, nxt = _step_slots(_need(step_dev, torch.int64, "step_dev"), parity)
    check(_lib.load().pda_dice_sample_dev(ptr(out[0]), 1, ptr(user_pool), int(n_pool), out[0].numel(), ptr(_need(train_indptr, torch.int64, "train_indptr")),
                                          ptr(_need(train_indices, torch.int32, "train_indices")), dp.n_items, ptr(dp.order), ptr(dp.sorted_pop),
                                          ptr(dp.pop), ptr(margin_dev), seed & (2 ** 64 - 1), ptr(src), ptr(nxt), ptr(out[1]), ptr(out[2]),
                                          ptr(out[3]), stream_ptr()), "pda_dice_sample_dev")
    return out


# ---- IPS, IPS-C, IPS-CN (include/pda_hip_ips.h) ---------------------------------------------------------------------------------------------
IPS_EMBED_SIZES = (32, 64, 128, 256)


class IpsWeights:
    """The inverse propensity weight of every item as a positive, built once per data set on the host: with n_i the train interactions of item i,
    p_i = max(n_i, 1) / max_j n_j and w_i = 1 / p_i in float64, w_i = min(w_i, clip) when clip > 0, then cast: ipw float32 [n_items] on the
    device of train_indices.  counts: the int64 numpy vector n_i."""

    def __init__(self, train_indices: torch.Tensor, n_items: int, clip: float = 0.0):
        import numpy as np
        idx = train_indices.detach().cpu().numpy().astype(np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= n_items):
            raise ValueError("a train item id lies outside the catalogue")
        self._build(np.bincount(idx, minlength=int(n_items)), clip, train_indices.device)

    @classmethod
    def from_counts(cls, counts, clip: float = 0.0, device="cpu"):
        """The same from the vector of train interactions per item."""
        import numpy as np
        counts = np.asarray(counts)
        if counts.ndim != 1 or counts.size == 0 or (counts < 0).any():
            raise ValueError("counts: one non-negative number of train interactions per item")
        self = cls.__new__(cls)
        self._build(counts.astype(np.int64), clip, device)
        return self

    def _build(self, counts, clip, device):
        import numpy as np
        clip = float(clip)
        if not clip >= 0.0:
            raise ValueError("--ips_clip must be >= 0 (0: no clip)")
        n = np.maximum(counts, 1).astype(np.float64)
        w = 1.0 / (n / float(max(int(counts.max()) if counts.size else 1, 1)))
        if clip > 0.0:
            w = np.minimum(w, clip)
        self.n_items, self.clip, self.counts = int(counts.size), clip, counts
        self.ipw = torch.from_numpy(w.astype(np.float32)).to(device)


def _ips_check(U, I, users, pos, neg, ipw, tagU, tagI, wsum, loss_acc, check_ids: bool):
    d, B = _triplet_shapes("IPS", "U [n_users, d] and I [n_items, d]", IPS_EMBED_SIZES, U, I, users, pos, neg)
    if _need(ipw, torch.float32, "ipw").numel() != I.shape[0]:
        raise ValueError("ipw holds one float32 per item")
    if _need(tagU, torch.int32, "tagU").numel() != U.shape[0] or _need(tagI, torch.int32, "tagI").numel() != I.shape[0]:
        raise ValueError("tagU / tagI hold one int32 per table row")
    if _need(wsum, torch.float32, "wsum", optional=True) is not None and wsum.numel() < 1:
        raise ValueError("wsum holds one float32")
    if _need(loss_acc, torch.float32, "loss_acc", optional=True) is not None and loss_acc.numel() < 3:
        raise ValueError("IPS loss_acc holds three float32")
    _triplet_ids("IPS", U, I, users, pos, neg, check_ids)
    return d, B


def _ips_flags(grouped: bool, users_distinct: bool) -> int:
    return (0 if grouped else UPD_ANY_ORDER) | (UPD_USERS_DISTINCT if users_distinct else 0)


def ips_weight_sum(ipw, users, pos, neg, n_users: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pda_ips_weight_sum -> float32 [1] on the device: the sum of ipw[pos] over the batch's valid triplets (one workgroup, a fixed order)."""
    ipw = _need(ipw, torch.float32, "ipw")
    users, pos, neg = (_need(t, torch.int32, n) for t, n in ((users, "users"), (pos, "pos"), (neg, "neg")))
    B = users.numel()
    if B < 1 or pos.numel() != B or neg.numel() != B:
        raise ValueError("users/pos/neg must have the same, non-zero length")
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=ipw.device)
    if _need(out, torch.float32, "out").numel() < 1:
        raise ValueError("out holds one float32")
    check(_lib.load().pda_ips_weight_sum(ptr(ipw), int(n_users), ipw.numel(), ptr(users), ptr(pos), ptr(neg), B, ptr(out), stream_ptr()),
          "pda_ips_weight_sum")
    return out


def ips_grads(U, I, users, pos, neg, ipw, gU, gI, tagU, tagI, *, wsum: Optional[torch.Tensor] = None, regs: float, reg_div: float, step: int,
              grouped: bool = False, users_distinct: bool = False, loss_acc: Optional[torch.Tensor] = None, check_ids: bool = True):
    """[pda_ips_weight_sum +] pda_ips_step_f32: the batch's gradient summed into gU / gI (rows tagged `step`), no update.  wsum float32 [1]: the
    self-normalised form (IPS-CN) -- the batch's weight sum is written there first and the triplets are scaled by w_t / wsum; None: by w_t / B.
    loss_acc float32 [3] += (loss, mf_loss, reg_loss)."""
    d, B = _ips_check(U, I, users, pos, neg, ipw, tagU, tagI, wsum, loss_acc, check_ids)
    gU, gI = _need(gU, torch.float32, "gU"), _need(gI, torch.float32, "gI")
    if gU.shape != U.shape or gI.shape != I.shape:
        raise ValueError("gU / gI have the shapes of the tables")
    lib = _lib.load()
    if wsum is not None:
        check(lib.pda_ips_weight_sum(ptr(ipw), U.shape[0], I.shape[0], ptr(users), ptr(pos), ptr(neg), B, ptr(wsum), stream_ptr()),
              "pda_ips_weight_sum")
    check(lib.pda_ips_step_f32(ptr(U), ptr(I), U.shape[0], I.shape[0], ptr(users), ptr(pos), ptr(neg), ptr(ipw), ptr(wsum), B, d, float(regs),
                               float(reg_div), ptr(gU), ptr(gI), ptr(tagU), ptr(tagI), int(step), _ips_flags(grouped, users_distinct), ptr(loss_acc),
                               stream_ptr()), "pda_ips_step_f32")


def ips_adam_step(U, mU, vU, gU, tagU, I, mI, vI, gI, tagI, users, pos, neg, ipw, *, wsum: Optional[torch.Tensor] = None, regs: float,
                  reg_div: float, step: int, lr_t: float, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS, grouped: bool = False,
                  users_distinct: bool = False, cache_policy: int = ADAM_CACHE_AUTO, loss_acc: Optional[torch.Tensor] = None,
                  check_ids: bool = False):
    """pda_ips_adam_step_f32: one IPS train step ([the weight sum,] the weighted gradients, TF-1.14 dense-decay Adam over both tables) in two or
    three launches; graph-capturable.  The arguments of adam_step with ipw float32 [n_items] in place of the popularities; wsum float32 [1]
    (workspace) selects the self-normalised form."""
    d, B = _ips_check(U, I, users, pos, neg, ipw, tagU, tagI, wsum, loss_acc, check_ids)
    for t in (mU, vU, gU, mI, vI, gI):
        _need(t, torch.float32, "adam state")
    if not (mU.shape == vU.shape == gU.shape == U.shape and mI.shape == vI.shape == gI.shape == I.shape):
        raise ValueError("the Adam state tables have the shapes of U and I")
    check(_lib.load().pda_ips_adam_step_f32(ptr(U), ptr(mU), ptr(vU), ptr(gU), ptr(tagU), U.shape[0], ptr(I), ptr(mI), ptr(vI), ptr(gI), ptr(tagI),
                                            I.shape[0], ptr(users), ptr(pos), ptr(neg), ptr(ipw), ptr(wsum), B, d, float(regs), float(reg_div),
                                            int(step), float(lr_t), beta1, beta2, eps, _ips_flags(grouped, users_distinct), int(cache_policy),
                                            ptr(loss_acc), stream_ptr()), "pda_ips_adam_step_f32")
    mark_modified(U, I)


# ---- the popularity-correlation regulariser (include/pda_hip_pcc.h) -------------------------------------------------------------------------
PCC_EMBED_SIZES = (32, 64, 128, 256)
PCC_ON = {"pos": _lib.PCC_ON_POS, "margin": _lib.PCC_ON_MARGIN}
PCC_POP_MODES = ("count", "log")


class PccPop:
    """The popularity of every item, built once per data set on the host from n_i, the train interactions of item i: mode "count": (float)n_i;
    "log": log1p(n_i) in float64, then cast.  pop float32 [n_items] on `device`.  (Pearson's r is invariant to positive affine maps, so counts,
    shares and propensities give the same model.)"""

    @classmethod
    def from_counts(cls, counts, mode: str = "count", device="cpu"):
        import numpy as np
        counts = np.asarray(counts)
        if counts.ndim != 1 or counts.size == 0 or (counts < 0).any():
            raise ValueError("counts: one non-negative number of train interactions per item")
        if mode not in PCC_POP_MODES:
            raise ValueError("--pcc_pop must be one of %s, got %r" % (" | ".join(PCC_POP_MODES), mode))
        counts = counts.astype(np.int64)
        pop = counts.astype(np.float32) if mode == "count" else np.log1p(counts.astype(np.float64)).astype(np.float32)
        self = cls.__new__(cls)
        self.n_items, self.mode, self.counts = int(counts.size), mode, counts
        self.pop = torch.from_numpy(pop).to(device)
        return self


def pcc_workspace(B: int, device):
    """(z_ws float32 [B], stat float64 [8]): the workspace of one batch size, private to one stream."""
    # (z_ws as it comes: the score pass of pda_pcc_stats_f32 writes every one of its B elements before the moments pass reads them)
    return torch.empty(int(B), dtype=torch.float32, device=device), torch.zeros(_lib.PCC_STAT_WORDS, dtype=torch.float64, device=device)


def _pcc_on(on: str) -> int:
    if on not in PCC_ON:
        raise ValueError("--pcc_on must be one of pos | margin, got %r" % (on,))
    return PCC_ON[on]


def _pcc_check(U, I, users, pos, neg, pop, z_ws, stat, check_ids: bool):
    d, B = _triplet_shapes("PCC", "U [n_users, d] and I [n_items, d]", PCC_EMBED_SIZES, U, I, users, pos, neg)
    if _need(pop, torch.float32, "pop").numel() != I.shape[0]:
        raise ValueError("pop holds one float32 per item")
    if _need(z_ws, torch.float32, "z_ws").numel() < B:
        raise ValueError("z_ws holds one float32 per triplet")
    if _need(stat, torch.float64, "stat").numel() < _lib.PCC_STAT_WORDS:
        raise ValueError("stat holds eight float64")
    _triplet_ids("PCC", U, I, users, pos, neg, check_ids)
    return d, B


def _pcc_step_check(U, I, tagU, tagI, gamma, loss_acc, pcc_acc):
    if not float(gamma) >= 0.0:
        raise ValueError("--pcc_gamma must be >= 0, got %s" % (gamma,))
    if _need(tagU, torch.int32, "tagU").numel() != U.shape[0] or _need(tagI, torch.int32, "tagI").numel() != I.shape[0]:
        raise ValueError("tagU / tagI hold one int32 per table row")
    if _need(loss_acc, torch.float32, "loss_acc", optional=True) is not None and loss_acc.numel() < 3:
        raise ValueError("PCC loss_acc holds three float32")
    if _need(pcc_acc, torch.float32, "pcc_acc", optional=True) is not None and pcc_acc.numel() < 2:
        raise ValueError("pcc_acc holds two float32")


def pcc_stats(U, I, users, pos, neg, pop, *, on: str = "pos", z_ws: Optional[torch.Tensor] = None, stat: Optional[torch.Tensor] = None,
              check_ids: bool = True):
    """pda_pcc_stats_f32 -> (z_ws float32 [B], stat float64 [8]) on the device: z_t of every triplet (0 for a refused one) and the batch's
    statistic (n_v, zbar, qbar, Szz, Sqq, Szq, r, 0): centred float64 moments in a fixed order, the same bits run after run."""
    if z_ws is None or stat is None:
        ws = pcc_workspace(_need(users, torch.int32, "users").numel(), users.device)
        z_ws, stat = (ws[0] if z_ws is None else z_ws), (ws[1] if stat is None else stat)
    d, B = _pcc_check(U, I, users, pos, neg, pop, z_ws, stat, check_ids)
    check(_lib.load().pda_pcc_stats_f32(ptr(U), ptr(I), U.shape[0], I.shape[0], ptr(users), ptr(pos), ptr(neg), ptr(pop), B, d, _pcc_on(on),
                                        ptr(z_ws), ptr(stat), stream_ptr()), "pda_pcc_stats_f32")
    return z_ws, stat


def pcc_grads(U, I, users, pos, neg, pop, gU, gI, tagU, tagI, *, gamma: float, on: str = "pos", regs: float, reg_div: float, step: int,
              grouped: bool = False, users_distinct: bool = False, z_ws: Optional[torch.Tensor] = None, stat: Optional[torch.Tensor] = None,
              loss_acc: Optional[torch.Tensor] = None, pcc_acc: Optional[torch.Tensor] = None, check_ids: bool = True):
    """pda_pcc_stats_f32 + pda_pcc_step_f32: the batch's gradient summed into gU / gI (rows tagged `step`), no update.  loss_acc float32 [3] +=
    (loss, mf_loss, reg_loss), pcc_acc float32 [2] += (r, r^2).  Returns (z_ws, stat) as pcc_stats does."""
    if z_ws is None or stat is None:
        ws = pcc_workspace(_need(users, torch.int32, "users").numel(), users.device)
        z_ws, stat = (ws[0] if z_ws is None else z_ws), (ws[1] if stat is None else stat)
    d, B = _pcc_check(U, I, users, pos, neg, pop, z_ws, stat, check_ids)
    _pcc_step_check(U, I, tagU, tagI, gamma, loss_acc, pcc_acc)
    gU, gI = _need(gU, torch.float32, "gU"), _need(gI, torch.float32, "gI")
    if gU.shape != U.shape or gI.shape != I.shape:
        raise ValueError("gU / gI have the shapes of the tables")
    lib, code = _lib.load(), _pcc_on(on)
    check(lib.pda_pcc_stats_f32(ptr(U), ptr(I), U.shape[0], I.shape[0], ptr(users), ptr(pos), ptr(neg), ptr(pop), B, d, code, ptr(z_ws), ptr(stat),
                                stream_ptr()), "pda_pcc_stats_f32")
    check(lib.pda_pcc_step_f32(ptr(U), ptr(I), U.shape[0], I.shape[0], ptr(users), ptr(pos), ptr(neg), ptr(pop), ptr(z_ws), ptr(stat), B, d,
                               float(gamma), code, float(regs), float(reg_div), ptr(gU), ptr(gI), ptr(tagU), ptr(tagI), int(step),
                               _ips_flags(grouped, users_distinct), ptr(loss_acc), ptr(pcc_acc), stream_ptr()), "pda_pcc_step_f32")
    return z_ws, stat


def pcc_adam_step(U, mU, vU, gU, tagU, I, mI, vI, gI, tagI, users, pos, neg, pop, z_ws, stat, *, gamma: float, on: str = "pos", regs: float,
                  reg_div: float, step: int, lr_t: float, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS, grouped: bool = False,
                  users_distinct: bool = False, cache_policy: int = ADAM_CACHE_AUTO, loss_acc: Optional[torch.Tensor] = None,
                  pcc_acc: Optional[torch.Tensor] = None, check_ids: bool = False):
    """pda_pcc_adam_step_f32: one PCC train step (the scores, their moments, the gradients, TF-1.14 dense-decay Adam over both tables) in four
    launches; graph-capturable.  The arguments of adam_step with pop float32 [n_items] in place of the popularities and the workspace
    (z_ws, stat) of pcc_workspace."""
    d, B = _pcc_check(U, I, users, pos, neg, pop, z_ws, stat, check_ids)
    _pcc_step_check(U, I, tagU, tagI, gamma, loss_acc, pcc_acc)
    for t in (mU, vU, gU, mI, vI, gI):
        _need(t, torch.float32, "adam state")
    if not (mU.shape == vU.shape == gU.shape == U.shape and mI.shape == vI.shape == gI.shape == I.shape):
        raise ValueError("the Adam state tables have the shapes of U and I")
    check(_lib.load().pda_pcc_adam_step_f32(ptr(U), ptr(mU), ptr(vU), ptr(gU), ptr(tagU), U.shape[0], ptr(I), ptr(mI), ptr(vI), ptr(gI), ptr(tagI),
                                            I.shape[0], ptr(users), ptr(pos), ptr(neg), ptr(pop), ptr(z_ws), ptr(stat), B, d, float(gamma),
                                            _pcc_on(on), float(regs), float(reg_div), int(step), float(lr_t), beta1, beta2, eps,
                                            _ips_flags(grouped, users_distinct), int(cache_policy), ptr(loss_acc), ptr(pcc_acc), stream_ptr()),
          "pda_pcc_adam_step_f32")
    mark_modified(U, I)


# ---- MACR (include/pda_hip_macr.h) ----------------------------------------------------------------------------------------------------------
MACR_EMBED_SIZES = (32, 64, 128, 256)         # the step and the item prep
MACR_EVAL_EMBED_SIZES = (64, 128, 256)        # the lists: the bias head of include/pda_hip_temp_pop.h
MACR_LOSS_TERMS = 5                           # a step's loss row: loss, L_O, L_I, L_U, reg


class MacrState:
    """What a MACR step writes besides the parameters: the Adam moments of both tables and of the two branch vectors (mW / vW float32 [2, d]:
    w_item, w_user), the dense gradient accumulators gU / gI / gW and the per-row step tags."""

    def __init__(self, U, I):
        z = torch.zeros_like
        self.mU, self.vU, self.gU, self.mI, self.vI, self.gI = z(U), z(U), z(U), z(I), z(I), z(I)
        self.tagU, self.tagI = adam_row_tags(U.shape[0], I.shape[0], U.device)
        self.mW, self.vW, self.gW = (torch.zeros((2, U.shape[1]), dtype=torch.float32, device=U.device) for _ in range(3))


def _macr_check(U, I, w_item, w_user, users, pos, neg, st, loss_acc, check_ids: bool):
    d, B = _triplet_shapes("MACR", "U [n_users, d] and I [n_items, d]", MACR_EMBED_SIZES, U, I, users, pos, neg)
    if _need(w_item, torch.float32, "w_item").numel() != d or _need(w_user, torch.float32, "w_user").numel() != d:
        raise ValueError("w_item / w_user hold d float32 each")
    if not isinstance(st, MacrState) or st.gU.shape != U.shape or st.gI.shape != I.shape:
        raise ValueError("st: the MacrState of these tables")
    if _need(loss_acc, torch.float32, "loss_acc", optional=True) is not None and loss_acc.numel() < MACR_LOSS_TERMS:
        raise ValueError("MACR loss_acc holds five float32")
    _triplet_ids("MACR", U, I, users, pos, neg, check_ids)
    return d, B


def macr_grads(U, I, w_item, w_user, users, pos, neg, st: MacrState, *, alpha: float, beta: float, regs: float, reg_div: float, step: int,
               grouped: bool = False, users_distinct: bool = False, loss_acc: Optional[torch.Tensor] = None, check_ids: bool = True):
    """pda_macr_step_f32: the batch's gradients summed into st.gU / st.gI (rows tagged `step`) and st.gW (row 0: w_item, row 1: w_user), no
    update.  loss_acc float32 [5] += (loss, L_O, L_I, L_U, reg)."""
    d, B = _macr_check(U, I, w_item, w_user, users, pos, neg, st, loss_acc, check_ids)
    check(_lib.load().pda_macr_step_f32(ptr(U), ptr(I), ptr(w_item), ptr(w_user), U.shape[0], I.shape[0], ptr(users), ptr(pos), ptr(neg), B, d,
                                        float(alpha), float(beta), float(regs), float(reg_div), ptr(st.gU), ptr(st.gI), ptr(st.gW), ptr(st.tagU),
                                        ptr(st.tagI), int(step), (0 if grouped else UPD_ANY_ORDER) | (UPD_USERS_DISTINCT if users_distinct else 0),
                                        ptr(loss_acc), stream_ptr()), "pda_macr_step_f32")


def macr_adam_step(U, I, w_item, w_user, users, pos, neg, st: MacrState, *, alpha: float, beta: float, regs: float, reg_div: float, step: int,
                   lr_t: float, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS, grouped: bool = False, users_distinct: bool = False,
                   cache_policy: int = ADAM_CACHE_AUTO, loss_acc: Optional[torch.Tensor] = None, check_ids: bool = False):
    """pda_macr_adam_step_f32: one MACR train step (the gradients, TF-1.14 dense-decay Adam over both tables, the same Adam over the two branch
    vectors) in three launches; graph-capturable."""
    d, B = _macr_check(U, I, w_item, w_user, users, pos, neg, st, loss_acc, check_ids)
    check(_lib.load().pda_macr_adam_step_f32(ptr(U), ptr(st.mU), ptr(st.vU), ptr(st.gU), ptr(st.tagU), U.shape[0], ptr(I), ptr(st.mI), ptr(st.vI),
                                             ptr(st.gI), ptr(st.tagI), I.shape[0], ptr(w_item), ptr(w_user), ptr(st.mW), ptr(st.vW), ptr(st.gW),
                                             ptr(users), ptr(pos), ptr(neg), B, d, float(alpha), float(beta), float(regs), float(reg_div), int(step),
                                             float(lr_t), beta1, beta2, eps, (0 if grouped else UPD_ANY_ORDER) | (UPD_USERS_DISTINCT if users_distinct else 0),
                                             int(cache_policy), ptr(loss_acc), stream_ptr()), "pda_macr_adam_step_f32")
    mark_modified(U, I, w_item, w_user)


class MacrItemPrep:
    """What MACR's lists read in place of the item table, built once per evaluation: sig float32 [n_items] = sigmoid(I_i . w_item),
    J float32 [n_items, d] = fl(sig_i I_i), and beta float32 [n_items], the bias of the value of c asked for last."""

    def __init__(self, n_items: int, d: int, device):
        self.sig = torch.empty(n_items, dtype=torch.float32, device=device)
        self.J = torch.empty((n_items, d), dtype=torch.float32, device=device)
        self.beta = torch.empty(n_items, dtype=torch.float32, device=device)
        self.c = None

    def bias(self, c: float) -> torch.Tensor:
        if self.c is None or float(c) != self.c:
            macr_item_bias(self.sig, c, self.beta)
            self.c = float(c)
        return self.beta


def macr_item_prep(I, w_item, out: Optional[MacrItemPrep] = None) -> MacrItemPrep:
    """pda_macr_item_prep_f32 -> MacrItemPrep (sig, J): one launch over the item table, the same bits run after run."""
    I, w_item = _need(I, torch.float32, "I"), _need(w_item, torch.float32, "w_item")
    if I.dim() != 2 or I.shape[1] not in MACR_EMBED_SIZES or w_item.numel() != I.shape[1]:
        raise ValueError(f"MACR item prep: I [n_items, d], d one of {MACR_EMBED_SIZES}, and w_item of d float32")
    n, d = I.shape
    if out is None:
        out = MacrItemPrep(n, d, I.device)
    if out.J.shape != I.shape or out.J.device != I.device:
        raise ValueError("out: the MacrItemPrep of a table of this shape")
    check(_lib.load().pda_macr_item_prep_f32(ptr(I), ptr(w_item), n, d, ptr(out.sig), ptr(out.J), stream_ptr()), "pda_macr_item_prep_f32")
    out.c = None
    mark_modified(out.J, out.sig)
    return out


def macr_item_bias(sig, c: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pda_macr_item_bias_f32 -> beta float32 [n]: beta_i = fl(-c sig_i)."""
    sig = _need(sig, torch.float32, "sig")
    if not math.isfinite(float(c)):
        raise ValueError(f"c must be finite, got {c}")
    if out is None:
        out = torch.empty_like(sig)
    if _need(out, torch.float32, "beta").numel() != sig.numel():
        raise ValueError("beta holds one float32 per item")
    check(_lib.load().pda_macr_item_bias_f32(ptr(sig), float(c), ptr(out), sig.numel(), stream_ptr()), "pda_macr_item_bias_f32")
    mark_modified(out)
    return out


def check_macr_lists(d: int, K: int):
    """MACR's lists come from the bias head: d in {64, 128, 256} and K <= 54, like BPRMF(t)-pop's."""
    if int(d) not in MACR_EVAL_EMBED_SIZES:
        raise ValueError(f"MACR lists: the embedding width must be one of {MACR_EVAL_EMBED_SIZES} (the bias-head score kernels), got {d}")
    if not 1 <= int(K) <= TOPK_K_V4:
        raise ValueError(f"MACR lists: K must lie in 1 .. {TOPK_K_V4} (the bias head has no deep lists), got {K}")


def recommend_topk_macr(U, I, w_item, users, c: float, K=50, hist: Optional[HistoryCSR] = None, prep: Optional[MacrItemPrep] = None,
                        stats: Optional[dict] = None):
    """MACR's counterfactual ranking by (y_ui - c) s_i -> (int32 [Bu, K] item ids, float32 [Bu, K] values): the bias head on J = fl(s_i I_i)
    with alpha = 1 and beta_i = fl(-c s_i), so the values are fl(chain(u . J_i) + beta_i).  prep: macr_item_prep(I, w_item) of the evaluation
    (built here when missing); every value of c costs one bias launch and one sweep."""
    U = _need(U, torch.float32, "U")
    users = _need(users, torch.int32, "users")
    check_macr_lists(U.shape[1], K)
    if prep is None:
        prep = macr_item_prep(I, w_item)
    if prep.J.shape[1] != U.shape[1]:
        raise ValueError("U and the item prep share the embed dim")
    ones = torch.ones(users.numel(), dtype=torch.float32, device=U.device)
    return recommend_topk_bias(U, prep.J, users, ones, prep.bias(c), K, hist, stats=stats)


# ---- LightGCN (include/pda_hip_gcn.h) -------------------------------------------------------------------------------------------------------
GCN_EMBED_SIZES = (32, 64, 128, 256)
GCN_CHUNK = _lib.GCN_CHUNK                    # PDA_GCN_CHUNK: a row with more edges is cut into chunks of this many
GCN_MAX_LAYERS = 4


def gcn_graph_arrays(users, items, n_users: int, n_items: int, chunk: int = GCN_CHUNK) -> dict:
    """The train graph of include/pda_hip_gcn.h from the train pairs, on the host (numpy; no GPU needed): the distinct (u, i) edges sorted by
    (u, i), deg_u / deg_i, w = fl32(1 / sqrt(float64(deg_u deg_i))), the symmetric CSR over the n_users + n_items stacked rows (a user row
    lists n_users + i ascending, an item row lists u ascending) and the work list (`work` int64 [n_work, 4] = row, first edge, end edge, slot;
    `long_rows` int64 [n_long, 3] = row, first slot, chunks; `n_slots`).  The entries of `work` are sorted by falling length (stable: rows and
    chunks in rising order among equals), so the lane groups of a wave run about equally long; every sum's order stays that of the CSR.
    Ids outside the tables are an error here, once: the kernels trust the graph."""
    import numpy as np
    n_users, n_items, chunk = int(n_users), int(n_items), int(chunk)
    if n_users < 1 or n_items < 1 or n_users + n_items > 0x7FFFFFFF or chunk < 1:
        raise ValueError("gcn graph: n_users, n_items >= 1 with n_users + n_items < 2^31, chunk >= 1")
    u, i = np.asarray(users, dtype=np.int64).reshape(-1), np.asarray(items, dtype=np.int64).reshape(-1)
    if u.shape != i.shape:
        raise ValueError("gcn graph: users and items hold one id per train pair each")
    if u.size and (u.min() < 0 or u.max() >= n_users or i.min() < 0 or i.max() >= n_items):
        raise ValueError("gcn graph: a train pair has a user or item id outside the tables")
    key = np.unique(u * n_items + i)
    eu, ei = key // n_items, key % n_items
    deg_u, deg_i = np.bincount(eu, minlength=n_users).astype(np.int64), np.bincount(ei, minlength=n_items).astype(np.int64)
    w = (1.0 / np.sqrt((deg_u[eu] * deg_i[ei]).astype(np.float64))).astype(np.float32)
    N = n_users + n_items
    o = np.lexsort((eu, ei))                       # the same edges by (i, u): the item rows
    deg = np.concatenate([deg_u, deg_i])
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = np.concatenate([n_users + ei, eu[o]]).astype(np.int32)
    weights = np.concatenate([w, w[o]])
    nch = np.maximum(1, -(-deg // chunk))
    first = np.cumsum(nch) - nch
    row = np.repeat(np.arange(N, dtype=np.int64), nch)
    j = np.arange(int(nch.sum()), dtype=np.int64) - np.repeat(first, nch)
    e0 = indptr[row] + j * chunk
    e1 = np.minimum(e0 + chunk, indptr[row + 1])
    is_long = nch > 1
    slot0 = np.cumsum(np.where(is_long, nch, 0)) - np.where(is_long, nch, 0)
    slot = np.where(is_long[row], slot0[row] + j, -1)
    order = np.argsort(-(e1 - e0), kind="stable")
    work = np.ascontiguousarray(np.stack([row, e0, e1, slot], axis=1)[order])
    lr = np.flatnonzero(is_long)
    long_rows = np.ascontiguousarray(np.stack([lr, slot0[lr], nch[lr]], axis=1).astype(np.int64))
    return dict(n_users=n_users, n_items=n_items, chunk=chunk, edge_users=eu, edge_items=ei, edge_w=w, deg_u=deg_u, deg_i=deg_i, indptr=indptr,
                indices=indices, w=weights, work=work, long_rows=long_rows, n_slots=int(np.where(is_long, nch, 0).sum()))


class GcnGraph:
    """The train graph on the device, built once per graph (gcn_graph_arrays): the deduplicated edges, the degrees and weights, the symmetric
    CSR and the work list; `host` keeps the numpy arrays.  It also owns what the passes write: the partial-sum workspace, two layer buffers,
    the final tables and the propagated gradient, one set per row width.  What gcn_propagate / gcn_backward return are views of those
    buffers: valid until the next call of the same function on this graph."""

    def __init__(self, users, items, n_users: int, n_items: int, device, chunk: int = GCN_CHUNK):
        if int(chunk) != GCN_CHUNK:
            raise ValueError(f"the kernels are built for chunks of {GCN_CHUNK} edges")
        h = self.host = gcn_graph_arrays(users, items, n_users, n_items, chunk)
        self.n_users, self.n_items, self.n_rows = h["n_users"], h["n_items"], h["n_users"] + h["n_items"]
        self.device = torch.device(device)
        dev = lambda a: torch.from_numpy(a).to(self.device)      # noqa: E731
        self.indptr, self.indices, self.w = dev(h["indptr"]), dev(h["indices"]), dev(h["w"])
        self.work, self.long_rows, self.n_slots = dev(h["work"]), dev(h["long_rows"]), h["n_slots"]
        self.n_edges = int(h["edge_w"].shape[0])
        self._bufs = {}

    @staticmethod
    def from_csr(indptr, indices, n_items: int, device) -> "GcnGraph":
        """From the train CSR (rows: users; int64 indptr, item ids), e.g. Data.train_csr."""
        import numpy as np
        ip = indptr.cpu().numpy() if torch.is_tensor(indptr) else np.asarray(indptr)
        ix = indices.cpu().numpy() if torch.is_tensor(indices) else np.asarray(indices)
        users = np.repeat(np.arange(len(ip) - 1, dtype=np.int64), np.diff(ip))
        return GcnGraph(users, ix, len(ip) - 1, n_items, device)

    def buffers(self, d: int) -> dict:
        if d not in self._bufs:
            mk = lambda: torch.zeros((self.n_rows, d), dtype=torch.float32, device=self.device)      # noqa: E731
            nbytes = _lib.load().pda_gcn_spmm_workspace_bytes(self.n_slots, d)
            b = dict(A=mk(), B=mk(), F=mk(), H=mk(), ws=torch.empty(max(1, nbytes), dtype=torch.uint8, device=self.device))
            b["Fv"], b["Hv"] = self.split(b["F"]), self.split(b["H"])      # (the same view objects call after call: what ops caches per table stays keyed)
            self._bufs[d] = b
        return self._bufs[d]

    def split(self, t):
        return t[:self.n_users], t[self.n_users:]


def _gcn_stacked(graph: GcnGraph, a, b, what: str):
    """(a [n_users, d]; b [n_items, d]) as ONE [n_users + n_items, d] tensor: the storage itself where b starts where a ends (the model's
    tables), a copy otherwise."""
    a, b = _need(a, torch.float32, what + " (users)"), _need(b, torch.float32, what + " (items)")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1] or a.shape[0] != graph.n_users or b.shape[0] != graph.n_items:
        raise ValueError(f"{what}: [n_users, d] and [n_items, d] tables of the graph's {graph.n_users} users and {graph.n_items} items")
    if a.shape[1] not in GCN_EMBED_SIZES:
        raise ValueError(f"LightGCN: the embedding width d must be one of {GCN_EMBED_SIZES}, got {a.shape[1]}")
    if a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr() and a.data_ptr() + a.numel() * 4 == b.data_ptr():
        return a.as_strided((graph.n_rows, a.shape[1]), (a.shape[1], 1), a.storage_offset())
    return torch.cat([a, b], dim=0)


def gcn_spmm(graph: GcnGraph, X, *, add=None, Y=None, sum_in=None, sum_out=None, scale: float = 1.0):
    """pda_gcn_spmm_f32 on stacked [n_users + n_items, d] tensors: y = add + A X;  Y = scale y, or with a running sum Y = y (optional) and
    sum_out = scale (sum_in + y).  Y is allocated when neither Y nor sum_out is given.  Returns (Y, sum_out)."""
    X = _need(X, torch.float32, "X")
    if X.dim() != 2 or X.shape[0] != graph.n_rows or X.shape[1] not in GCN_EMBED_SIZES:
        raise ValueError(f"X: float32 [{graph.n_rows}, d], d one of {GCN_EMBED_SIZES}")
    if (sum_in is None) != (sum_out is None):
        raise ValueError("sum_in and sum_out come together")
    if Y is None and sum_out is None:
        Y = torch.empty_like(X)
    for t, n in ((add, "add"), (Y, "Y"), (sum_in, "sum_in"), (sum_out, "sum_out")):
        if _need(t, torch.float32, n, optional=True) is not None and t.shape != X.shape:
            raise ValueError(f"{n} has the shape of X")
    if not math.isfinite(float(scale)):
        raise ValueError("scale must be finite")
    d = X.shape[1]
    ws = graph.buffers(d)["ws"]
    check(_lib.load().pda_gcn_spmm_f32(ptr(graph.indptr), ptr(graph.indices), ptr(graph.w), graph.n_rows, ptr(graph.work), graph.work.shape[0],
                                       ptr(graph.long_rows) if graph.long_rows.shape[0] else None, graph.long_rows.shape[0], graph.n_slots,
                                       ptr(X), d, ptr(add), ptr(Y), ptr(sum_in), ptr(sum_out), float(scale),
                                       ptr(ws) if graph.n_slots else None, ws.numel() if graph.n_slots else 0, stream_ptr()), "pda_gcn_spmm_f32")
    mark_modified(*(t for t in (Y, sum_out) if t is not None))
    return Y, sum_out


def _gcn_layers(L) -> int:
    L = int(L)
    if not 0 <= L <= GCN_MAX_LAYERS:
        raise ValueError(f"gcn layers must lie in 0 .. {GCN_MAX_LAYERS}, got {L}")
    return L


def gcn_propagate(graph: GcnGraph, U0, I0, L: int):
    """The final tables (F_U, F_I) = (1 / (L + 1)) sum_k A^k (U0; I0): L launches (plus one per layer for cut rows), the layer mean kept as a
    running sum by each row's owner and scaled in the last one.  L = 0: the ego tables themselves.  The result is a pair of views of the
    graph's own buffer."""
    L = _gcn_layers(L)
    E0 = _gcn_stacked(graph, U0, I0, "ego tables")
    if L == 0:
        return U0, I0
    b = graph.buffers(E0.shape[1])
    X, F = E0, b["F"]
    for k in range(1, L + 1):
        last = k == L
        Y = None if last else b["AB"[(k - 1) & 1]]
        gcn_spmm(graph, X, Y=Y, sum_in=E0 if k == 1 else F, sum_out=F, scale=1.0 / (L + 1) if last else 1.0)
        X = Y
    return b["Fv"]


def gcn_backward(graph: GcnGraph, G_U, G_I, L: int):
    """(1 / (L + 1)) sum_{k = 0 .. L} A^k (G_U; G_I) in Horner form: H <- G + A H, L times from H = G, the last one scaled.  L = 0: G itself.
    The result is a pair of views of the graph's own buffer."""
    L = _gcn_layers(L)
    G = _gcn_stacked(graph, G_U, G_I, "gradient tables")
    if L == 0:
        return G_U, G_I
    b = graph.buffers(G.shape[1])
    X = G
    for j in range(1, L + 1):
        last = j == L
        Y = b["H"] if last else b["AB"[(j - 1) & 1]]
        gcn_spmm(graph, X, add=G, Y=Y, scale=1.0 / (L + 1) if last else 1.0)
        X = Y
    return b["Hv"]


def gcn_reg(U0, I0, users, pos, neg, gU, gI, *, regs: float, reg_div: float, loss_acc: Optional[torch.Tensor] = None):
    """pda_gcn_reg_f32: gU / gI += (regs / reg_div) x the batch's ego rows, per occurrence; loss_acc float32 [3]: [0] and [2] += the regulariser."""
    U0, I0, gU, gI = (_need(t, torch.float32, n) for t, n in ((U0, "U0"), (I0, "I0"), (gU, "gU"), (gI, "gI")))
    if U0.dim() != 2 or I0.dim() != 2 or U0.shape[1] != I0.shape[1] or gU.shape != U0.shape or gI.shape != I0.shape:
        raise ValueError("gcn_reg: U0 [n_users, d], I0 [n_items, d] and gradient tables of the same shapes")
    if U0.shape[1] not in GCN_EMBED_SIZES:
        raise ValueError(f"LightGCN: the embedding width d must be one of {GCN_EMBED_SIZES}, got {U0.shape[1]}")
    users, pos, neg = (_need(t, torch.int32, n) for t, n in ((users, "users"), (pos, "pos"), (neg, "neg")))
    B = users.numel()
    if B < 1 or pos.numel() != B or neg.numel() != B:
        raise ValueError("users/pos/neg must have the same, non-zero length")
    if _need(loss_acc, torch.float32, "loss_acc", optional=True) is not None and loss_acc.numel() < 3:
        raise ValueError("loss_acc holds three float32")
    check(_lib.load().pda_gcn_reg_f32(ptr(U0), ptr(I0), U0.shape[0], I0.shape[0], ptr(users), ptr(pos), ptr(neg), B, U0.shape[1], float(regs),
                                      float(reg_div), ptr(gU), ptr(gI), ptr(loss_acc), stream_ptr()), "pda_gcn_reg_f32")
    mark_modified(gU, gI)


# ---- the sampled-softmax loss (include/pda_hip_ssm.h) ------------------------------------------------------------------------------------------
SSM_EMBED_SIZES = (32, 64, 128, 256)
SSM_MAX_NEGS = _lib.SSM_MAX_NEGS


def _ssm_params(tau, norm):
    tau = float(tau)
    if not (tau > 0.0 and math.isfinite(tau)):
        raise ValueError(f"SSM: tau must be a finite number > 0, got {tau}")
    if norm not in (0, 1, False, True):
        raise ValueError(f"SSM: norm must be 0 or 1, got {norm!r}")
    return tau, int(norm)


def _ssm_logq(logq, I):
    """logq of the sampled-softmax steps: None, or float32 [n_items] beside the tables."""
    if logq is not None and (_need(logq, torch.float32, "logq").dim() != 1 or logq.numel() != I.shape[0] or logq.device != I.device):
        raise ValueError(f"SSM logq: float32 [n_items] = [{I.shape[0]}] on the tables' device")
    return logq


def _ssm_check(U, I, users, pos, negs, tagU, tagI, loss_acc, check_ids: bool):
    """The tables and (users, pos) as every tagged step checks them, negs int32 [B, N] with 1 <= N <= SSM_MAX_NEGS -> (d, B, N)."""
    negs = _need(negs, torch.int32, "negs")
    d, B = _triplet_shapes("SSM", "U [n_users, d] and I [n_items, d]", SSM_EMBED_SIZES, U, I, users, pos, pos)
    if negs.dim() != 2 or negs.shape[0] != B or not 1 <= negs.shape[1] <= SSM_MAX_NEGS:
        raise ValueError(f"SSM negs: int32 [B, N] with B = {B} rows and 1 <= N <= {SSM_MAX_NEGS}, got {tuple(negs.shape)}")
    if _need(tagU, torch.int32, "tagU").numel() != U.shape[0] or _need(tagI, torch.int32, "tagI").numel() != I.shape[0]:
        raise ValueError("tagU / tagI hold one int32 per table row")
    if _need(loss_acc, torch.float32, "loss_acc", optional=True) is not None and loss_acc.numel() < 3:
        raise ValueError("SSM loss_acc holds three float32")
    _triplet_ids("SSM", U, I, users, pos, negs, check_ids)
    return d, B, int(negs.shape[1])


def ssm_step(U, I, users, pos, negs, gU, gI, tagU, tagI, *, tau: float, norm: int, regs: float, reg_div: float, step: int, grouped: bool = False,
             users_distinct: bool = False, loss_acc: Optional[torch.Tensor] = None, check_ids: bool = True, logq: Optional[torch.Tensor] = None):
    """pda_ssm_step_f32: the batch's sampled-softmax gradient summed into gU / gI (rows tagged `step`), no update.  negs int32 [B, N].
    loss_acc float32 [3] += (loss, mf_loss, reg_loss).  logq float32 [n_items]: pda_ssm_step_logq_f32, every logit takes - logq[item]."""
    d, B, N = _ssm_check(U, I, users, pos, negs, tagU, tagI, loss_acc, check_ids)
    logq = _ssm_logq(logq, I)
    tau, norm = _ssm_params(tau, norm)
    gU, gI = _need(gU, torch.float32, "gU"), _need(gI, torch.float32, "gI")
    if gU.shape != U.shape or gI.shape != I.shape:
        raise ValueError("gU / gI have the shapes of the tables")
    if logq is None:
        check(_lib.load().pda_ssm_step_f32(ptr(U), ptr(I), U.shape[0], I.shape[0], ptr(users), ptr(pos), ptr(negs), B, N, d, tau, norm, float(regs),
                                           float(reg_div), ptr(gU), ptr(gI), ptr(tagU), ptr(tagI), int(step), _ips_flags(grouped, users_distinct),
                                           ptr(loss_acc), stream_ptr()), "pda_ssm_step_f32")
    else:
        check(_lib.load().pda_ssm_step_logq_f32(ptr(U), ptr(I), U.shape[0], I.shape[0], ptr(users), ptr(pos), ptr(negs), ptr(logq), B, N, d, tau, norm,
                                                float(regs), float(reg_div), ptr(gU), ptr(gI), ptr(tagU), ptr(tagI), int(step),
                                                _ips_flags(grouped, users_distinct), ptr(loss_acc), stream_ptr()), "pda_ssm_step_logq_f32")
    mark_modified(gU, gI)


def ssm_adam_step(U, mU, vU, gU, tagU, I, mI, vI, gI, tagI, users, pos, negs, *, tau: float, norm: int, regs: float, reg_div: float, step: int,
                  lr_t: float, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS, grouped: bool = False, users_distinct: bool = False,
                  cache_policy: int = ADAM_CACHE_AUTO, loss_acc: Optional[torch.Tensor] = None, check_ids: bool = False,
                  logq: Optional[torch.Tensor] = None):
    """pda_ssm_adam_step_f32: one sampled-softmax train step (the gradients, TF-1.14 dense-decay Adam over both tables) in two launches;
    graph-capturable.  The arguments of adam_step with negs int32 [B, N] in place of the negative and the popularities.  logq float32
    [n_items]: pda_ssm_adam_step_logq_f32."""
    d, B, N = _ssm_check(U, I, users, pos, negs, tagU, tagI, loss_acc, check_ids)
    logq = _ssm_logq(logq, I)
    tau, norm = _ssm_params(tau, norm)
    for t in (mU, vU, gU, mI, vI, gI):
        _need(t, torch.float32, "adam state")
    if not (mU.shape == vU.shape == gU.shape == U.shape and mI.shape == vI.shape == gI.shape == I.shape):
        raise ValueError("the Adam state tables have the shapes of U and I")
    if logq is None:
        check(_lib.load().pda_ssm_adam_step_f32(ptr(U), ptr(mU), ptr(vU), ptr(gU), ptr(tagU), U.shape[0], ptr(I), ptr(mI), ptr(vI), ptr(gI), ptr(tagI),
                                                I.shape[0], ptr(users), ptr(pos), ptr(negs), B, N, d, tau, norm, float(regs), float(reg_div), int(step),
                                                float(lr_t), beta1, beta2, eps, _ips_flags(grouped, users_distinct), int(cache_policy), ptr(loss_acc),
                                                stream_ptr()), "pda_ssm_adam_step_f32")
    else:
        check(_lib.load().pda_ssm_adam_step_logq_f32(ptr(U), ptr(mU), ptr(vU), ptr(gU), ptr(tagU), U.shape[0], ptr(I), ptr(mI), ptr(vI), ptr(gI),
                                                     ptr(tagI), I.shape[0], ptr(users), ptr(pos), ptr(negs), ptr(logq), B, N, d, tau, norm, float(regs),
                                                     float(reg_div), int(step), float(lr_t), beta1, beta2, eps, _ips_flags(grouped, users_distinct),
                                                     int(cache_policy), ptr(loss_acc), stream_ptr()), "pda_ssm_adam_step_logq_f32")
    mark_modified(U, I)


def _ssm_sample_args(train_indptr, train_indices, B, N, neg_range, user_pool, n_pool):
    if not 1 <= int(N) <= SSM_MAX_NEGS:
        raise ValueError(f"SSM: the number of negatives per row must lie in 1 .. {SSM_MAX_NEGS}, got {N}")
    if int(B) < 1:
        raise ValueError("SSM sampler: B >= 1")
    if int(neg_range[1]) <= int(neg_range[0]):
        raise ValueError("SSM sampler: neg_range = (lo, hi) with hi > lo")
    _need(train_indptr, torch.int64, "train_indptr"), _need(train_indices, torch.int32, "train_indices")
    if user_pool is not None and _need(user_pool, torch.int32, "user_pool").numel() < int(n_pool):
        raise ValueError("user_pool holds n_pool int32")


def ssm_sample(train_indptr, train_indices, B: int, N: int, *, seed: int, step: int, neg_range, users=None, user_pool=None, n_pool: int = 0):
    """pda_ssm_sample -> (users, pos, negs [B, N]) on the device: the users and positives of sample_triplets(seed, step), N negatives per row
    (column 0: the negative of sample_triplets).  users given: they are kept and only positives and negatives are drawn."""
    _ssm_sample_args(train_indptr, train_indices, B, N, neg_range, user_pool, n_pool)
    dev = train_indptr.device
    gen = users is None
    if gen:
        if int(n_pool) < 1:
            raise ValueError("SSM sampler: drawing users needs n_pool >= 1")
        users = torch.empty(B, dtype=torch.int32, device=dev)
    elif _need(users, torch.int32, "users").numel() != B:
        raise ValueError("users holds B int32")
    pos = torch.empty(B, dtype=torch.int32, device=dev)
    negs = torch.empty((B, N), dtype=torch.int32, device=dev)
    check(_lib.load().pda_ssm_sample(ptr(users), int(gen), ptr(user_pool), int(n_pool), int(B), int(N), ptr(train_indptr), ptr(train_indices),
                                     int(neg_range[0]), int(neg_range[1]), seed & (2 ** 64 - 1), int(step), ptr(pos), ptr(negs), stream_ptr()),
          "pda_ssm_sample")
    return users, pos, negs


def ssm_sample_into(out, train_indptr, train_indices, *, seed: int, step_dev: torch.Tensor, neg_range, parity: Optional[int] = None, user_pool=None,
                    n_pool: int = 0):
    """pda_ssm_sample_dev: one batch into out = (users [B], pos [B], negs [B, N]), the step read from device memory (graph-capturable).
    step_dev int64 [1]: read only.  step_dev int64 [2] + parity p: read from slot p, step + 1 stored to slot 1 - p (sample_triplets_into)."""
    users, pos, negs = out
    users, pos, negs = _need(users, torch.int32, "users"), _need(pos, torch.int32, "pos"), _need(negs, torch.int32, "negs")
    B = users.numel()
    if pos.numel() != B or negs.dim() != 2 or negs.shape[0] != B:
        raise ValueError("SSM sampler output: users [B], pos [B], negs [B, N]")
    _ssm_sample_args(train_indptr, train_indices, B, negs.shape[1], neg_range, user_pool, n_pool)
    if int(n_pool) < 1:
        raise ValueError("SSM sampler: drawing users needs n_pool >= 1")
    src, nxt = _step_slots(_need(step_dev, torch.int64, "step_dev"), parity)
    check(_lib.load().pda_ssm_sample_dev(ptr(users), 1, ptr(user_pool), int(n_pool), B, int(negs.shape[1]), ptr(train_indptr), ptr(train_indices),
                                         int(neg_range[0]), int(neg_range[1]), seed & (2 ** 64 - 1), ptr(src), ptr(nxt), ptr(pos), ptr(negs),
                                         stream_ptr()), "pda_ssm_sample_dev")
    return out


def ssm_normalize_rows(X, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pda_ssm_normalize_rows_f32 -> Y float32 [n_rows, d], Y[r] = X[r] / max(|X[r]|, 1e-12) (the sum of squares in float64, a fixed order):
    the evaluation tables of a norm == 1 model."""
    X = _need(X, torch.float32, "X")
    if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] not in SSM_EMBED_SIZES:
        raise ValueError(f"ssm_normalize_rows: X float32 [n_rows >= 1, d], d one of {SSM_EMBED_SIZES}, got {tuple(X.shape)}")
    if out is None:
        out = torch.empty_like(X)
    if _need(out, torch.float32, "out").shape != X.shape:
        raise ValueError("out has the shape of X")
    check(_lib.load().pda_ssm_normalize_rows_f32(ptr(X), X.shape[0], X.shape[1], ptr(out), stream_ptr()), "pda_ssm_normalize_rows_f32")
    mark_modified(out)
    return out


# ---- the in-batch softmax with logQ correction (include/pda_hip_inbatch.h) ----------------------------------------------------------------------
INBATCH_MAX_B = _lib.INBATCH_MAX_B
INBATCH_ROW_TILE = _lib.INBATCH_ROW_TILE
INBATCH_COL_TILE = _lib.INBATCH_COL_TILE


def inbatch_col_splits(B: int) -> int:
    """pda_inbatch_col_splits: the column ranges the tile passes split a batch of B into."""
    if not 1 <= int(B) <= INBATCH_MAX_B:
        raise ValueError(f"in-batch softmax: the batch size must lie in 1 .. {INBATCH_MAX_B}, got {B}")
    return int(_lib.load().pda_inbatch_col_splits(int(B)))


def inbatch_workspace(B: int, d: int, device) -> torch.Tensor:
    """The workspace of one batch size and width (pda_inbatch_workspace_bytes): uint8, private to one stream."""
    if not 1 <= int(B) <= INBATCH_MAX_B:
        raise ValueError(f"in-batch softmax: the batch size must lie in 1 .. {INBATCH_MAX_B}, got {B}")
    if d not in SSM_EMBED_SIZES:
        raise ValueError(f"in-batch softmax: the embedding width d must be one of {SSM_EMBED_SIZES}, got {d}")
    return torch.empty(int(_lib.load().pda_inbatch_workspace_bytes(int(B), int(d))), dtype=torch.uint8, device=device)


def inbatch_mask_words(B: int) -> int:
    return (int(B) + 31) // 32


def inbatch_logq(train_indptr, train_indices, n_items: int, user_pool=None):
    """log q_i of the device sampler's columns, on the host -> numpy float32 [n_items].  The sampler draws a user uniformly from its pool (all
    users without one) and then one of that user's train items uniformly: q_i = (1 / n_pool) sum_{u in pool, i in I_u} 1 / |I_u|, summed in
    float64 and rounded once.  An item that never appears as a column (q_i = 0) takes the log of the smallest positive q: the table stays finite."""
    import numpy as np
    to_np = lambda t: t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)      # noqa: E731
    indptr, indices = to_np(train_indptr).astype(np.int64), to_np(train_indices).astype(np.int64)
    pool = np.arange(len(indptr) - 1, dtype=np.int64) if user_pool is None else to_np(user_pool).astype(np.int64)
    if pool.size < 1:
        raise ValueError("inbatch_logq: an empty user pool")
    lens = (indptr[1:] - indptr[:-1])[pool]
    # a user without train items puts item 0 into its column (the sampler's convention); such users are not in a trainer's pool
    q = np.zeros(int(n_items), dtype=np.float64)
    has = lens > 0
    starts = indptr[pool[has]]
    flat = np.concatenate([indices[s:s + n] for s, n in zip(starts, lens[has])]) if has.any() else np.zeros(0, np.int64)
    np.add.at(q, flat, np.repeat(1.0 / lens[has], lens[has]))
    q[0] += float((~has).sum())
    q /= float(pool.size)
    if not (q > 0).any():
        raise ValueError("inbatch_logq: no item occurs")
    q[q == 0] = q[q > 0].min()
    return np.log(q).astype(np.float32)


def inbatch_mask(users, pos, train_indptr, train_indices, n_users: int, n_items: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pda_inbatch_mask -> int32 [B, ceil(B / 32)] (the words are the kernel's uint32): bit (r, c) set iff c != r and pos[c] is a train item of
    users[r]."""
    users, pos = _need(users, torch.int32, "users"), _need(pos, torch.int32, "pos")
    _need(train_indptr, torch.int64, "train_indptr"), _need(train_indices, torch.int32, "train_indices")
    B = users.numel()
    if not 1 <= B <= INBATCH_MAX_B or pos.numel() != B:
        raise ValueError(f"in-batch softmax: users / pos of one length in 1 .. {INBATCH_MAX_B}")
    if train_indptr.numel() != int(n_users) + 1:
        raise ValueError("train_indptr holds n_users + 1 int64")
    W = inbatch_mask_words(B)
    if out is None:
        out = torch.empty((B, W), dtype=torch.int32, device=users.device)
    if _need(out, torch.int32, "mask").numel() != B * W:
        raise ValueError(f"mask: int32 [B, ceil(B / 32)] = [{B}, {W}]")
    check(_lib.load().pda_inbatch_mask(ptr(users), ptr(pos), B, ptr(train_indptr), ptr(train_indices), int(n_users), int(n_items), ptr(out),
                                       stream_ptr()), "pda_inbatch_mask")
    mark_modified(out)
    return out


def _inbatch_check(U, I, users, pos, logq, mask, tagU, tagI, ws, loss_acc, check_ids: bool):
    """The tables and (users, pos) as every tagged step checks them, the optional logq float32 [n_items] and mask int32 [B, ceil(B / 32)], the
    workspace -> (d, B)."""
    d, B = _triplet_shapes("in-batch softmax", "U [n_users, d] and I [n_items, d]", SSM_EMBED_SIZES, U, I, users, pos, pos)
    if B > INBATCH_MAX_B:
        raise ValueError(f"in-batch softmax: the batch size must lie in 1 .. {INBATCH_MAX_B}, got {B}")
    if _need(logq, torch.float32, "logq", optional=True) is not None and logq.numel() != I.shape[0]:
        raise ValueError("logq holds one float32 per item")
    if _need(mask, torch.int32, "mask", optional=True) is not None and mask.numel() != B * inbatch_mask_words(B):
        raise ValueError(f"mask: int32 [B, ceil(B / 32)] = [{B}, {inbatch_mask_words(B)}]")
    if _need(tagU, torch.int32, "tagU").numel() != U.shape[0] or _need(tagI, torch.int32, "tagI").numel() != I.shape[0]:
        raise ValueError("tagU / tagI hold one int32 per table row")
    if _need(ws, torch.uint8, "ws").numel() < int(_lib.load().pda_inbatch_workspace_bytes(B, d)):
        raise ValueError("ws: the workspace of inbatch_workspace(B, d)")
    if _need(loss_acc, torch.float32, "loss_acc", optional=True) is not None and loss_acc.numel() < 3:
        raise ValueError("in-batch softmax loss_acc holds three float32")
    _triplet_ids("in-batch softmax", U, I, users, pos, pos, check_ids)
    return d, B


def inbatch_step(U, I, users, pos, gU, gI, tagU, tagI, ws, *, tau: float, norm: int, regs: float, reg_div: float, step: int, logq=None, mask=None,
                 grouped: bool = False, users_distinct: bool = False, loss_acc: Optional[torch.Tensor] = None, check_ids: bool = True):
    """pda_inbatch_step_f32: the batch's in-batch softmax gradient summed into gU / gI (rows tagged `step`), no update.
    loss_acc float32 [3] += (loss, mf_loss, reg_loss)."""
    d, B = _inbatch_check(U, I, users, pos, logq, mask, tagU, tagI, ws, loss_acc, check_ids)
    tau, norm = _ssm_params(tau, norm)
    gU, gI = _need(gU, torch.float32, "gU"), _need(gI, torch.float32, "gI")
    if gU.shape != U.shape or gI.shape != I.shape:
        raise ValueError("gU / gI have the shapes of the tables")
    check(_lib.load().pda_inbatch_step_f32(ptr(U), ptr(I), U.shape[0], I.shape[0], ptr(users), ptr(pos), B, d, tau, norm, ptr(logq), ptr(mask),
                                           float(regs), float(reg_div), ptr(gU), ptr(gI), ptr(tagU), ptr(tagI), int(step),
                                           _ips_flags(grouped, users_distinct), ptr(ws), ws.numel(), ptr(loss_acc), stream_ptr()),
          "pda_inbatch_step_f32")
    mark_modified(gU, gI)


def inbatch_adam_step(U, mU, vU, gU, tagU, I, mI, vI, gI, tagI, users, pos, ws, *, tau: float, norm: int, regs: float, reg_div: float, step: int,
                      lr_t: float, logq=None, mask=None, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS, grouped: bool = False,
                      users_distinct: bool = False, cache_policy: int = ADAM_CACHE_AUTO, loss_acc: Optional[torch.Tensor] = None,
                      check_ids: bool = False):
    """pda_inbatch_adam_step_f32: one in-batch softmax train step (the gradients, TF-1.14 dense-decay Adam over both tables) in five launches;
    graph-capturable.  The arguments of ssm_adam_step without the block of negatives, with the workspace and the optional logq and mask."""
    d, B = _inbatch_check(U, I, users, pos, logq, mask, tagU, tagI, ws, loss_acc, check_ids)
    tau, norm = _ssm_params(tau, norm)
    for t in (mU, vU, gU, mI, vI, gI):
        _need(t, torch.float32, "adam state")
    if not (mU.shape == vU.shape == gU.shape == U.shape and mI.shape == vI.shape == gI.shape == I.shape):
        raise ValueError("the Adam state tables have the shapes of U and I")
    check(_lib.load().pda_inbatch_adam_step_f32(ptr(U), ptr(mU), ptr(vU), ptr(gU), ptr(tagU), U.shape[0], ptr(I), ptr(mI), ptr(vI), ptr(gI),
                                                ptr(tagI), I.shape[0], ptr(users), ptr(pos), B, d, tau, norm, ptr(logq), ptr(mask), float(regs),
                                                float(reg_div), int(step), float(lr_t), beta1, beta2, eps, _ips_flags(grouped, users_distinct),
                                                int(cache_policy), ptr(ws), ws.numel(), ptr(loss_acc), stream_ptr()),
          "pda_inbatch_adam_step_f32")
    mark_modified(U, I)


# ---- the DirectAU loss (include/pda_hip_dau.h) ---------------------------------------------------------------------------------------------------------
DAU_MAX_B = _lib.DAU_MAX_B
DAU_MAX_T = _lib.DAU_MAX_T
DAU_TILE = _lib.DAU_TILE
DAU_EMBED_SIZES = (32, 64, 128, 256)
DAU_SAME = {"keep": _lib.DAU_SAME_KEEP, "drop": _lib.DAU_SAME_DROP}
DAU_STAT_WORDS = _lib.DAU_STAT_WORDS


def dau_col_splits(B: int) -> int:
    """pda_dau_col_splits: the column ranges the pass over the Gram tiles splits a batch of B into."""
    if not 1 <= int(B) <= DAU_MAX_B:
        raise ValueError(f"DirectAU: the batch size must lie in 1 .. {DAU_MAX_B}, got {B}")
    return int(_lib.load().pda_dau_col_splits(int(B)))


def dau_workspace(B: int, d: int, device) -> torch.Tensor:
    """The workspace of one batch size and width (pda_dau_workspace_bytes): uint8, private to one stream."""
    if not 1 <= int(B) <= DAU_MAX_B:
        raise ValueError(f"DirectAU: the batch size must lie in 1 .. {DAU_MAX_B}, got {B}")
    if d not in DAU_EMBED_SIZES:
        raise ValueError(f"DirectAU: the embedding width d must be one of {DAU_EMBED_SIZES}, got {d}")
    return torch.empty(int(_lib.load().pda_dau_workspace_bytes(int(B), int(d))), dtype=torch.uint8, device=device)


def _dau_params(t, gamma, same):
    t, gamma = float(t), float(gamma)
    if not 0.0 < t <= DAU_MAX_T:
        raise ValueError(f"DirectAU: t must lie in (0, {DAU_MAX_T:g}], got {t}")
    if not (gamma >= 0.0 and math.isfinite(gamma)):
        raise ValueError(f"DirectAU: gamma must be a finite number >= 0, got {gamma}")
    if same not in DAU_SAME:
        raise ValueError(f"DirectAU: same must be one of {sorted(DAU_SAME)}, got {same!r}")
    return t, gamma, DAU_SAME[same]


def _dau_check(U, I, users, pos, tagU, tagI, ws, stat, loss_acc, check_ids: bool):
    """The tables and (users, pos) as every tagged step checks them, the workspace, the optional stat float32 [4] and loss_acc float32 [3]
    -> (d, B)."""
    d, B = _triplet_shapes("DirectAU", "U [n_users, d] and I [n_items, d]", DAU_EMBED_SIZES, U, I, users, pos, pos)
    if B > DAU_MAX_B:
        raise ValueError(f"DirectAU: the batch size must lie in 1 .. {DAU_MAX_B}, got {B}")
    if _need(tagU, torch.int32, "tagU").numel() != U.shape[0] or _need(tagI, torch.int32, "tagI").numel() != I.shape[0]:
        raise ValueError("tagU / tagI hold one int32 per table row")
    if _need(ws, torch.uint8, "ws").numel() < int(_lib.load().pda_dau_workspace_bytes(B, d)):
        raise ValueError("ws: the workspace of dau_workspace(B, d)")
    if _need(stat, torch.float32, "stat", optional=True) is not None and stat.numel() < DAU_STAT_WORDS:
        raise ValueError(f"DirectAU stat holds {DAU_STAT_WORDS} float32")
    if _need(loss_acc, torch.float32, "loss_acc", optional=True) is not None and loss_acc.numel() < 3:
        raise ValueError("DirectAU loss_acc holds three float32")
    _triplet_ids("DirectAU", U, I, users, pos, pos, check_ids)
    return d, B


def dau_step(U, I, users, pos, gU, gI, tagU, tagI, ws, *, t: float, gamma: float, same: str = "keep", regs: float, reg_div: float, step: int,
             grouped: bool = False, users_distinct: bool = False, stat: Optional[torch.Tensor] = None, loss_acc: Optional[torch.Tensor] = None,
             check_ids: bool = True):
    """pda_dau_step_f32: the batch's DirectAU gradient summed into gU / gI (rows tagged `step`), no update.
    loss_acc float32 [3] += (loss, mf_loss, reg_loss); stat float32 [4] += (align, uni_U, uni_I, 1)."""
    d, B = _dau_check(U, I, users, pos, tagU, tagI, ws, stat, loss_acc, check_ids)
    t, gamma, same = _dau_params(t, gamma, same)
    gU, gI = _need(gU, torch.float32, "gU"), _need(gI, torch.float32, "gI")
    if gU.shape != U.shape or gI.shape != I.shape:
        raise ValueError("gU / gI have the shapes of the tables")
    check(_lib.load().pda_dau_step_f32(ptr(U), ptr(I), U.shape[0], I.shape[0], ptr(users), ptr(pos), B, d, t, gamma, same, float(regs),
                                       float(reg_div), ptr(gU), ptr(gI), ptr(tagU), ptr(tagI), int(step), _ips_flags(grouped, users_distinct),
                                       ptr(ws), ws.numel(), ptr(stat), ptr(loss_acc), stream_ptr()), "pda_dau_step_f32")
    mark_modified(gU, gI)


def dau_adam_step(U, mU, vU, gU, tagU, I, mI, vI, gI, tagI, users, pos, ws, *, t: float, gamma: float, same: str = "keep", regs: float,
                  reg_div: float, step: int, lr_t: float, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS, grouped: bool = False,
                  users_distinct: bool = False, cache_policy: int = ADAM_CACHE_AUTO, stat: Optional[torch.Tensor] = None,
                  loss_acc: Optional[torch.Tensor] = None, check_ids: bool = False):
    """pda_dau_adam_step_f32: one DirectAU train step (the gradients, TF-1.14 dense-decay Adam over both tables) in five launches;
    graph-capturable.  The arguments of inbatch_adam_step with (t, gamma, same) in place of (tau, norm, logq, mask), and the optional stat."""
    d, B = _dau_check(U, I, users, pos, tagU, tagI, ws, stat, loss_acc, check_ids)
    t, gamma, same = _dau_params(t, gamma, same)
    for x in (mU, vU, gU, mI, vI, gI):
        _need(x, torch.float32, "adam state")
    if not (mU.shape == vU.shape == gU.shape == U.shape and mI.shape == vI.shape == gI.shape == I.shape):
        raise ValueError("the Adam state tables have the shapes of U and I")
    check(_lib.load().pda_dau_adam_step_f32(ptr(U), ptr(mU), ptr(vU), ptr(gU), ptr(tagU), U.shape[0], ptr(I), ptr(mI), ptr(vI), ptr(gI),
                                            ptr(tagI), I.shape[0], ptr(users), ptr(pos), B, d, t, gamma, same, float(regs), float(reg_div),
                                            int(step), float(lr_t), beta1, beta2, eps, _ips_flags(grouped, users_distinct), int(cache_policy),
                                            ptr(ws), ws.numel(), ptr(stat), ptr(loss_acc), stream_ptr()), "pda_dau_adam_step_f32")
    mark_modified(U, I)


# ---- the full-catalogue softmax (include/pda_hip_fullsm.h) -----------------------------------------------------------------------------------------
FULLSM_MAX_B = _lib.FULLSM_MAX_B
FULLSM_ROW_TILE = _lib.FULLSM_ROW_TILE
FULLSM_COL_TILE = _lib.FULLSM_COL_TILE


def _fullsm_sizes(B, n_items):
    if not 1 <= int(B) <= FULLSM_MAX_B:
        raise ValueError(f"full softmax: the batch size must lie in 1 .. {FULLSM_MAX_B}, got {B}")
    if not 1 <= int(n_items) <= 2 ** 31 - 1:
        raise ValueError(f"full softmax: n_items must lie in 1 .. 2^31 - 1, got {n_items}")


def fullsm_col_splits(n_items: int, B: int) -> int:
    """pda_fullsm_col_splits: the column ranges the row-statistics pass and the user-side pass split the n_items columns into."""
    _fullsm_sizes(B, n_items)
    return int(_lib.load().pda_fullsm_col_splits(int(n_items), int(B)))


def fullsm_workspace(B: int, n_items: int, d: int, device) -> torch.Tensor:
    """The workspace of one batch size, catalogue and width (pda_fullsm_workspace_bytes): uint8, private to one stream."""
    _fullsm_sizes(B, n_items)
    if d not in SSM_EMBED_SIZES:
        raise ValueError(f"full softmax: the embedding width d must be one of {SSM_EMBED_SIZES}, got {d}")
    return torch.empty(int(_lib.load().pda_fullsm_workspace_bytes(int(B), int(n_items), int(d))), dtype=torch.uint8, device=device)


def _fullsm_check(U, I, users, pos, train_indptr, train_indices, tagU, tagI, ws, loss_acc, row_stats, check_ids: bool):
    """The tables and (users, pos) as every tagged step checks them (the checks of _inbatch_check), the optional train CSR (int64 [n_users + 1],
    int32, both or neither), the workspace and the optional row_stats float32 [B, 2] -> (d, B)."""
    d, B = _triplet_shapes("full softmax", "U [n_users, d] and I [n_items, d]", SSM_EMBED_SIZES, U, I, users, pos, pos)
    if B > FULLSM_MAX_B:
        raise ValueError(f"full softmax: the batch size must lie in 1 .. {FULLSM_MAX_B}, got {B}")
    if (train_indptr is None) != (train_indices is None):
        raise ValueError("full softmax: train_indptr and train_indices go together (both None: no item is excluded)")
    if _need(train_indptr, torch.int64, "train_indptr", optional=True) is not None:
        _need(train_indices, torch.int32, "train_indices")
        if train_indptr.numel() != U.shape[0] + 1:
            raise ValueError("train_indptr holds n_users + 1 int64")
    if _need(tagU, torch.int32, "tagU").numel() != U.shape[0] or _need(tagI, torch.int32, "tagI").numel() != I.shape[0]:
        raise ValueError("tagU / tagI hold one int32 per table row")
    if _need(ws, torch.uint8, "ws").numel() < int(_lib.load().pda_fullsm_workspace_bytes(B, I.shape[0], d)):
        raise ValueError("ws: the workspace of fullsm_workspace(B, n_items, d)")
    if _need(loss_acc, torch.float32, "loss_acc", optional=True) is not None and loss_acc.numel() < 3:
        raise ValueError("full softmax loss_acc holds three float32")
    if _need(row_stats, torch.float32, "row_stats", optional=True) is not None and row_stats.numel() != 2 * B:
        raise ValueError(f"row_stats: float32 [B, 2] = [{B}, 2]")
    _triplet_ids("full softmax", U, I, users, pos, pos, check_ids)
    return d, B


def fullsm_step(U, I, users, pos, gU, gI, tagU, tagI, ws, *, tau: float, norm: int, regs: float, reg_div: float, step: int, train_indptr=None,
                train_indices=None, users_distinct: bool = False, loss_acc: Optional[torch.Tensor] = None,
                row_stats: Optional[torch.Tensor] = None, check_ids: bool = True):
    """pda_fullsm_step_f32: the batch's full-catalogue softmax gradient summed into gU / gI (the users' rows and EVERY item row tagged `step`), no
    update.  loss_acc float32 [3] += (loss, mf_loss, reg_loss); row_stats float32 [B, 2] = (m_r, log se_r)."""
    d, B = _fullsm_check(U, I, users, pos, train_indptr, train_indices, tagU, tagI, ws, loss_acc, row_stats, check_ids)
    tau, norm = _ssm_params(tau, norm)
    gU, gI = _need(gU, torch.float32, "gU"), _need(gI, torch.float32, "gI")
    if gU.shape != U.shape or gI.shape != I.shape:
        raise ValueError("gU / gI have the shapes of the tables")
    check(_lib.load().pda_fullsm_step_f32(ptr(U), ptr(I), U.shape[0], I.shape[0], ptr(users), ptr(pos), B, d, tau, norm, ptr(train_indptr),
                                          ptr(train_indices), float(regs), float(reg_div), ptr(gU), ptr(gI), ptr(tagU), ptr(tagI), int(step),
                                          _ips_flags(False, users_distinct), ptr(ws), ws.numel(), ptr(loss_acc), ptr(row_stats), stream_ptr()),
          "pda_fullsm_step_f32")
    mark_modified(gU, gI)


def fullsm_adam_step(U, mU, vU, gU, tagU, I, mI, vI, gI, tagI, users, pos, ws, *, tau: float, norm: int, regs: float, reg_div: float, step: int,
                     lr_t: float, train_indptr=None, train_indices=None, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS,
                     users_distinct: bool = False, cache_policy: int = ADAM_CACHE_AUTO, loss_acc: Optional[torch.Tensor] = None,
                     row_stats: Optional[torch.Tensor] = None, check_ids: bool = False):
    """pda_fullsm_adam_step_f32: one full-catalogue softmax train step (the gradients, TF-1.14 dense-decay Adam over both tables);
    graph-capturable.  The arguments of inbatch_adam_step with the train CSR in place of logq and mask."""
    d, B = _fullsm_check(U, I, users, pos, train_indptr, train_indices, tagU, tagI, ws, loss_acc, row_stats, check_ids)
    tau, norm = _ssm_params(tau, norm)
    for t in (mU, vU, gU, mI, vI, gI):
        _need(t, torch.float32, "adam state")
    if not (mU.shape == vU.shape == gU.shape == U.shape and mI.shape == vI.shape == gI.shape == I.shape):
        raise ValueError("the Adam state tables have the shapes of U and I")
    check(_lib.load().pda_fullsm_adam_step_f32(ptr(U), ptr(mU), ptr(vU), ptr(gU), ptr(tagU), U.shape[0], ptr(I), ptr(mI), ptr(vI), ptr(gI),
                                               ptr(tagI), I.shape[0], ptr(users), ptr(pos), B, d, tau, norm, ptr(train_indptr), ptr(train_indices),
                                               float(regs), float(reg_div), int(step), float(lr_t), beta1, beta2, eps,
                                               _ips_flags(False, users_distinct), int(cache_policy), ptr(ws), ws.numel(), ptr(loss_acc),
                                               ptr(row_stats), stream_ptr()),
          "pda_fullsm_adam_step_f32")
    mark_modified(U, I)


# ---- dynamic hard-negative sampling (include/pda_hip_dns.h) -----------------------------------------------------------------------------------------
DNS_MAX_CANDIDATES = _lib.DNS_MAX_CANDIDATES
DNS_EMBED_SIZES = (32, 64, 128, 256)


def check_dns_sizes(n_cands, topn, what: str = "DNS"):
    """1 <= n_cands <= DNS_MAX_CANDIDATES, 1 <= topn <= n_cands, both whole numbers (the library's own limits, met before the device is touched)."""
    if int(n_cands) != n_cands or not 1 <= int(n_cands) <= DNS_MAX_CANDIDATES:
        raise ValueError(f"{what}: n_cands, the candidates per row, must be an integer in 1 .. {DNS_MAX_CANDIDATES}, got {n_cands}")
    if int(topn) != topn or not 1 <= int(topn) <= int(n_cands):
        raise ValueError(f"{what}: topn must be an integer in 1 .. n_cands = {int(n_cands)}, got {topn}")


def _dns_args(U, I, train_indptr, train_indices, train_slots, B, M, topn, head, neg_range, pop_matrix, user_pool, n_pool):
    """The host-side checks of both DNS front-ends -> (n_slots, lo, hi)."""
    U, I = _need(U, torch.float32, "U"), _need(I, torch.float32, "I")
    if U.dim() != 2 or I.dim() != 2 or U.shape[1] != I.shape[1] or U.shape[1] not in DNS_EMBED_SIZES or U.shape[0] < 1 or I.shape[0] < 1:
        raise ValueError(f"DNS sampler: U float32 [n_users, d], I float32 [n_items, d], d one of {DNS_EMBED_SIZES}, got {tuple(U.shape)}, {tuple(I.shape)}")
    check_dns_sizes(M, topn, "DNS sampler")
    if int(B) < 1 or int(B) > (1 << 22):
        raise ValueError("DNS sampler: B in 1 .. 2^22")
    lo, hi = int(neg_range[0]), int(neg_range[1])
    if not 0 <= lo < hi <= I.shape[0]:
        raise ValueError(f"DNS sampler: neg_range = (lo, hi) with 0 <= lo < hi <= n_items = {I.shape[0]}, got ({lo}, {hi})")
    if head not in (HEAD_RAW, HEAD_POP):
        raise ValueError("DNS sampler: head is HEAD_RAW or HEAD_POP")
    _need(train_indptr, torch.int64, "train_indptr"), _need(train_indices, torch.int32, "train_indices")
    if train_indptr.numel() != U.shape[0] + 1:
        raise ValueError("DNS sampler: train_indptr holds n_users + 1 offsets")
    _need(train_slots, torch.int32, "train_slots", optional=True)
    if user_pool is not None and _need(user_pool, torch.int32, "user_pool").numel() < int(n_pool):
        raise ValueError("user_pool holds n_pool int32")
    n_slots = 0
    if pop_matrix is not None:
        pop_matrix = _need(pop_matrix, torch.float32, "pop_matrix")
        if pop_matrix.dim() != 2 or pop_matrix.shape[0] != I.shape[0] or pop_matrix.shape[1] < 1:
            raise ValueError("DNS sampler: pop_matrix float32 [n_items, n_slots >= 1]")
        n_slots = pop_matrix.shape[1]
    elif head == HEAD_POP:
        raise ValueError("DNS sampler: HEAD_POP scores (elu(u . i) + 1) * pop and needs pop_matrix")
    return n_slots, lo, hi


def dns_sample(U, I, train_indptr, train_indices, B: int, *, n_cands: int, topn: int = 1, head: int = HEAD_RAW, seed: int, step: int, neg_range,
               users=None, user_pool=None, n_pool: int = 0, train_slots=None, pop_matrix=None, want_cands: bool = False, check_ids: bool = True):
    """pda_dns_sample_f32 -> (users, pos, neg, pos_pop|None, neg_pop|None) on the device: the users, positives and slots of
    sample_triplets(seed, step); neg is one of the topn best-scoring (head, on the tables as they are NOW) of the n_cands candidates a row draws
    as ssm_sample draws its columns.  want_cands: (.., cand i32 [B, M], cand_score f32 [B, M], pick_col i32 [B]) behind the five.
    users given: they are kept (check_ids: refused unless all lie in [0, n_users); costs a host sync)."""
    n_slots, lo, hi = _dns_args(U, I, train_indptr, train_indices, train_slots, B, n_cands, topn, head, neg_range, pop_matrix, user_pool, n_pool)
    dev = U.device
    gen = users is None
    if gen:
        if int(n_pool) < 1:
            raise ValueError("DNS sampler: drawing users needs n_pool >= 1")
        users = torch.empty(B, dtype=torch.int32, device=dev)
    else:
        if _need(users, torch.int32, "users").numel() != B:
            raise ValueError("users holds B int32")
        if check_ids and B > 0 and not bool(((users >= 0) & (users < U.shape[0])).all()):
            raise ValueError("DNS sampler: a user id lies outside [0, n_users)")
    M = int(n_cands)
    pos = torch.empty(B, dtype=torch.int32, device=dev)
    neg = torch.empty(B, dtype=torch.int32, device=dev)
    pp = pn = cand = score = col = None
    if pop_matrix is not None:
        pp, pn = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev)
    if want_cands:
        cand, score = torch.empty((B, M), dtype=torch.int32, device=dev), torch.empty((B, M), dtype=torch.float32, device=dev)
        col = torch.empty(B, dtype=torch.int32, device=dev)
    check(_lib.load().pda_dns_sample_f32(ptr(U), ptr(I), U.shape[0], I.shape[0], U.shape[1], ptr(users), int(gen), ptr(user_pool), int(n_pool), int(B),
                                         ptr(train_indptr), ptr(train_indices), ptr(train_slots), ptr(pop_matrix), n_slots, lo, hi, M, int(topn),
                                         int(head), seed & (2 ** 64 - 1), int(step), ptr(pos), ptr(neg), ptr(pp), ptr(pn), ptr(cand), ptr(score),
                                         ptr(col), stream_ptr()), "pda_dns_sample_f32")
    return (users, pos, neg, pp, pn) + ((cand, score, col) if want_cands else ())


def dns_sample_into(out, U, I, train_indptr, train_indices, *, n_cands: int, topn: int = 1, head: int = HEAD_RAW, seed: int, step_dev: torch.Tensor,
                    neg_range, parity: Optional[int] = None, user_pool=None, n_pool: int = 0, train_slots=None, pop_matrix=None, cands=None):
    """pda_dns_sample_f32_dev: one batch into out = (users, pos, neg, pos_pop|None, neg_pop|None), the step read from device memory
    (graph-capturable; the users are drawn).  step_dev int64 [1]: read only.  step_dev int64 [2] + parity p: read from slot p, step + 1 stored
    to slot 1 - p (sample_triplets_into).  cands: optional (cand i32 [B, M], cand_score f32 [B, M], pick_col i32 [B]) to fill as well."""
    users, pos, neg, pp, pn = out
    users, pos, neg = _need(users, torch.int32, "users"), _need(pos, torch.int32, "pos"), _need(neg, torch.int32, "neg")
    B, M = users.numel(), int(n_cands)
    if pos.numel() != B or neg.numel() != B:
        raise ValueError("DNS sampler output: users [B], pos [B], neg [B]")
    n_slots, lo, hi = _dns_args(U, I, train_indptr, train_indices, train_slots, B, n_cands, topn, head, neg_range, pop_matrix, user_pool, n_pool)
    if int(n_pool) < 1:
        raise ValueError("DNS sampler: drawing users needs n_pool >= 1")
    if (pp is None) != (pn is None) or (pp is not None and pop_matrix is None):
        raise ValueError("DNS sampler output: pos_pop and neg_pop come together, and with a pop_matrix")
    for t, name in ((pp, "pos_pop"), (pn, "neg_pop")):
        if t is not None and _need(t, torch.float32, name).numel() != B:
            raise ValueError(f"{name} holds B float32")
    cand = score = col = None
    if cands is not None:
        cand, score, col = cands
        cand, score, col = _need(cand, torch.int32, "cand"), _need(score, torch.float32, "cand_score"), _need(col, torch.int32, "pick_col")
        if tuple(cand.shape) != (B, M) or tuple(score.shape) != (B, M) or col.numel() != B:
            raise ValueError("DNS sampler output: cand [B, M], cand_score [B, M], pick_col [B]")
    src, nxt = _step_slots(_need(step_dev, torch.int64, "step_dev"), parity)
    check(_lib.load().pda_dns_sample_f32_dev(ptr(U), ptr(I), U.shape[0], I.shape[0], U.shape[1], ptr(users), 1, ptr(user_pool), int(n_pool), B,
                                             ptr(train_indptr), ptr(train_indices), ptr(train_slots), ptr(pop_matrix), n_slots, lo, hi, M, int(topn),
                                             int(head), seed & (2 ** 64 - 1), ptr(src), ptr(nxt), ptr(pos), ptr(neg), ptr(pp), ptr(pn), ptr(cand),
                                             ptr(score), ptr(col), stream_ptr()), "pda_dns_sample_f32_dev")
    return out


# ---- the WARP loss (include/pda_hip_warp.h) ------------------------------------------------------------------------------------------------------
WARP_MAX_TRIALS = _lib.WARP_MAX_TRIALS
WARP_EMBED_SIZES = (32, 64, 128, 256)
WARP_WEIGHT_KINDS = ("harmonic", "log", "none")


def check_warp_sizes(max_trials, margin, what: str = "WARP"):
    """1 <= max_trials <= WARP_MAX_TRIALS, a whole number; margin not NaN (+-inf are the library's to take: +inf makes every candidate a violator)."""
    if int(max_trials) != max_trials or not 1 <= int(max_trials) <= WARP_MAX_TRIALS:
        raise ValueError(f"{what}: max_trials, the candidates a row may try, must be an integer in 1 .. {WARP_MAX_TRIALS}, got {max_trials}")
    if float(margin) != float(margin):
        raise ValueError(f"{what}: the margin is NaN")


class WarpWeights:
    """wtab of pda_warp_sample_f32: the weight of a triplet whose first violator was its N-th candidate, N = 1 .. T, built on the host in float64
    and rounded once to fp32.  rank(N) = floor((n_eligible - 1) / N) estimates the positive's rank among the n_eligible = neg_hi - neg_lo items
    the candidates are drawn from.  kind "harmonic": sum_{k = 1 .. rank} 1 / k (WSABIE) | "log": log(max(1, rank)) (LightFM's form: its weight
    is 0 at rank 1, so a triplet whose estimated rank is 1 -- or 0 -- does not train) | "none": 1 (the plain hinge on the first violator).
    wtab[0] = 0: a row without a violator.  table64: the float64 values, wtab: float32 [T + 1] on `device`."""

    def __init__(self, table64, kind, n_eligible, device):
        import numpy as np
        self.kind, self.n_eligible, self.T = kind, int(n_eligible), len(table64) - 1
        self.table64 = np.asarray(table64, dtype=np.float64)
        self.wtab = torch.from_numpy(self.table64.astype(np.float32)).to(device)
        self.max_weight = float(self.table64.astype(np.float32).max())

    @classmethod
    def build(cls, n_eligible, T, kind="harmonic", device="cpu"):
        import numpy as np
        if kind not in WARP_WEIGHT_KINDS:
            raise ValueError(f"WARP weights: kind must be one of {WARP_WEIGHT_KINDS}, got {kind!r}")
        if int(n_eligible) != n_eligible or int(n_eligible) < 1:
            raise ValueError(f"WARP weights: n_eligible, the items a candidate is drawn from, must be an integer >= 1, got {n_eligible}")
        if int(T) != T or not 1 <= int(T) <= WARP_MAX_TRIALS:
            raise ValueError(f"WARP weights: T must be an integer in 1 .. {WARP_MAX_TRIALS}, got {T}")
        n, T = int(n_eligible), int(T)
        rank = (n - 1) // np.arange(1, T + 1, dtype=np.int64)
        tab = np.zeros(T + 1, dtype=np.float64)
        if kind == "harmonic":
            h = np.concatenate([[0.0], np.cumsum(1.0 / np.arange(1, max(n, 2), dtype=np.float64))])      # h[k] = 1 + 1/2 + .. + 1/k
            tab[1:] = h[rank]
        elif kind == "log":
            tab[1:] = np.log(np.maximum(1, rank).astype(np.float64))
        else:
            tab[1:] = 1.0
        return cls(tab, kind, n, device)


def _warp_args(U, I, train_indptr, train_indices, train_slots, B, T, margin, wtab, neg_range, pop_matrix, user_pool, n_pool):
    """The host-side checks of both WARP sampler front-ends -> (n_slots, lo, hi)."""
    U, I = _need(U, torch.float32, "U"), _need(I, torch.float32, "I")
    if U.dim() != 2 or I.dim() != 2 or U.shape[1] != I.shape[1] or U.shape[1] not in WARP_EMBED_SIZES or U.shape[0] < 1 or I.shape[0] < 1:
        raise ValueError(f"WARP sampler: U float32 [n_users, d], I float32 [n_items, d], d one of {WARP_EMBED_SIZES}, got {tuple(U.shape)}, {tuple(I.shape)}")
    check_warp_sizes(T, margin, "WARP sampler")
    if _need(wtab, torch.float32, "wtab").numel() != int(T) + 1:
        raise ValueError(f"WARP sampler: wtab holds max_trials + 1 = {int(T) + 1} float32, got {wtab.numel()}")
    if int(B) < 1 or int(B) > (1 << 22):
        raise ValueError("WARP sampler: B in 1 .. 2^22")
    lo, hi = int(neg_range[0]), int(neg_range[1])
    if not 0 <= lo < hi <= I.shape[0]:
        raise ValueError(f"WARP sampler: neg_range = (lo, hi) with 0 <= lo < hi <= n_items = {I.shape[0]}, got ({lo}, {hi})")
    _need(train_indptr, torch.int64, "train_indptr"), _need(train_indices, torch.int32, "train_indices")
    if train_indptr.numel() != U.shape[0] + 1:
        raise ValueError("WARP sampler: train_indptr holds n_users + 1 offsets")
    _need(train_slots, torch.int32, "train_slots", optional=True)
    if user_pool is not None and _need(user_pool, torch.int32, "user_pool").numel() < int(n_pool):
        raise ValueError("user_pool holds n_pool int32")
    n_slots = 0
    if pop_matrix is not None:
        pop_matrix = _need(pop_matrix, torch.float32, "pop_matrix")
        if pop_matrix.dim() != 2 or pop_matrix.shape[0] != I.shape[0] or pop_matrix.shape[1] < 1:
            raise ValueError("WARP sampler: pop_matrix float32 [n_items, n_slots >= 1]")
        n_slots = pop_matrix.shape[1]
    return n_slots, lo, hi


def warp_sample(U, I, train_indptr, train_indices, B: int, *, max_trials: int, margin: float, wtab, seed: int, step: int, neg_range, users=None,
                user_pool=None, n_pool: int = 0, train_slots=None, pop_matrix=None, want_cands: bool = False, stat=None, check_ids: bool = True):
    """pda_warp_sample_f32 -> (users, pos, neg, coef, trials, pos_pop|None, neg_pop|None) on the device: the users, positives and slots of
    sample_triplets(seed, step); neg is the first of the max_trials candidates a row draws as ssm_sample draws its columns that violates the
    margin on the tables as they are NOW (margin - (u.pos - u.cand) > 0), trials its 1-based column (0: none, neg is the last candidate) and
    coef = wtab[trials].  want_cands: (.., cand i32 [B, T], cand_score f32 [B, T], pos_score f32 [B]) behind the seven.  stat int64 [2] +=
    (sum of trials over the rows with a violator, rows without one).  users given: they are kept (check_ids: refused unless all lie in
    [0, n_users); costs a host sync).  The outputs of a call are rows of one zeroed block (one fill per call, no uninitialised memory)."""
    n_slots, lo, hi = _warp_args(U, I, train_indptr, train_indices, train_slots, B, max_trials, margin, wtab, neg_range, pop_matrix, user_pool, n_pool)
    dev = U.device
    gen = users is None
    if gen:
        if int(n_pool) < 1:
            raise ValueError("WARP sampler: drawing users needs n_pool >= 1")
    else:
        if _need(users, torch.int32, "users").numel() != B:
            raise ValueError("users holds B int32")
        if check_ids and B > 0 and not bool(((users >= 0) & (users < U.shape[0])).all()):
            raise ValueError("WARP sampler: a user id lies outside [0, n_users)")
    if stat is not None and _need(stat, torch.int64, "stat").numel() < 2:
        raise ValueError("WARP sampler: stat holds two int64")
    T = int(max_trials)
    block = torch.zeros((7, int(B)), dtype=torch.int32, device=dev)      # users, pos, neg, trials | coef, pos_pop, neg_pop (as float32)
    pos, neg, trials, coef = block[1], block[2], block[3], block[4].view(torch.float32)
    if gen:
        users = block[0]
    pp = pn = cand = score = ps = None
    if pop_matrix is not None:
        pp, pn = block[5].view(torch.float32), block[6].view(torch.float32)
    if want_cands:
        wide = torch.zeros((2 * T + 1, int(B)), dtype=torch.int32, device=dev)
        cand, score = wide[:T].view(int(B), T), wide[T:2 * T].view(torch.float32).view(int(B), T)
        ps = wide[2 * T].view(torch.float32)
    check(_lib.load().pda_warp_sample_f32(ptr(U), ptr(I), U.shape[0], I.shape[0], U.shape[1], ptr(users), int(gen), ptr(user_pool), int(n_pool), int(B),
                                          ptr(train_indptr), ptr(train_indices), ptr(train_slots), ptr(pop_matrix), n_slots, lo, hi, T, float(margin),
                                          ptr(wtab), seed & (2 ** 64 - 1), int(step), ptr(pos), ptr(neg), ptr(trials), ptr(coef), ptr(pp), ptr(pn),
                                          ptr(cand), ptr(score), ptr(ps), ptr(stat), stream_ptr()), "pda_warp_sample_f32")
    return (users, pos, neg, coef, trials, pp, pn) + ((cand, score, ps) if want_cands else ())


def warp_sample_into(out, U, I, train_indptr, train_indices, *, max_trials: int, margin: float, wtab, seed: int, step_dev: torch.Tensor, neg_range,
                     parity: Optional[int] = None, user_pool=None, n_pool: int = 0, train_slots=None, pop_matrix=None, cands=None, stat=None):
    """pda_warp_sample_f32_dev: one batch into out = (users, pos, neg, coef, trials, pos_pop|None, neg_pop|None), the step read from device memory
    (graph-capturable; the users are drawn).  step_dev int64 [1]: read only.  step_dev int64 [2] + parity p: read from slot p, step + 1 stored
    to slot 1 - p (sample_triplets_into).  cands: optional (cand i32 [B, T], cand_score f32 [B, T], pos_score f32 [B]) to fill as well."""
    users, pos, neg, coef, trials, pp, pn = out
    users, pos, neg, trials = (_need(t, torch.int32, n) for t, n in ((users, "users"), (pos, "pos"), (neg, "neg"), (trials, "trials")))
    coef = _need(coef, torch.float32, "coef")
    B, T = users.numel(), int(max_trials)
    if pos.numel() != B or neg.numel() != B or trials.numel() != B or coef.numel() != B:
        raise ValueError("WARP sampler output: users [B], pos [B], neg [B], coef [B], trials [B]")
    n_slots, lo, hi = _warp_args(U, I, train_indptr, train_indices, train_slots, B, max_trials, margin, wtab, neg_range, pop_matrix, user_pool, n_pool)
    if int(n_pool) < 1:
        raise ValueError("WARP sampler: drawing users needs n_pool >= 1")
    if (pp is None) != (pn is None) or (pp is not None and pop_matrix is None):
        raise ValueError("WARP sampler output: pos_pop and neg_pop come together, and with a pop_matrix")
    for t, name in ((pp, "pos_pop"), (pn, "neg_pop")):
        if t is not None and _need(t, torch.float32, name).numel() != B:
            raise ValueError(f"{name} holds B float32")
    cand = score = ps = None
    if cands is not None:
        cand, score, ps = cands
        cand, score, ps = _need(cand, torch.int32, "cand"), _need(score, torch.float32, "cand_score"), _need(ps, torch.float32, "pos_score")
        if tuple(cand.shape) != (B, T) or tuple(score.shape) != (B, T) or ps.numel() != B:
            raise ValueError("WARP sampler output: cand [B, T], cand_score [B, T], pos_score [B]")
    if stat is not None and _need(stat, torch.int64, "stat").numel() < 2:
        raise ValueError("WARP sampler: stat holds two int64")
    src, nxt = _step_slots(_need(step_dev, torch.int64, "step_dev"), parity)
    check(_lib.load().pda_warp_sample_f32_dev(ptr(U), ptr(I), U.shape[0], I.shape[0], U.shape[1], ptr(users), 1, ptr(user_pool), int(n_pool), B,
                                              ptr(train_indptr), ptr(train_indices), ptr(train_slots), ptr(pop_matrix), n_slots, lo, hi, T,
                                              float(margin), ptr(wtab), seed & (2 ** 64 - 1), ptr(src), ptr(nxt), ptr(pos), ptr(neg), ptr(trials),
                                              ptr(coef), ptr(pp), ptr(pn), ptr(cand), ptr(score), ptr(ps), ptr(stat), stream_ptr()),
          "pda_warp_sample_f32_dev")
    return out


def _warp_check(U, I, users, pos, neg, coef, margin, tagU, tagI, loss_acc, check_ids: bool):
    d, B = _triplet_shapes("WARP", "U [n_users, d] and I [n_items, d]", WARP_EMBED_SIZES, U, I, users, pos, neg)
    if _need(coef, torch.float32, "coef").numel() != B:
        raise ValueError("coef holds one float32 per triplet")
    if float(margin) != float(margin):
        raise ValueError("WARP: the margin is NaN")
    if _need(tagU, torch.int32, "tagU").numel() != U.shape[0] or _need(tagI, torch.int32, "tagI").numel() != I.shape[0]:
        raise ValueError("tagU / tagI hold one int32 per table row")
    if _need(loss_acc, torch.float32, "loss_acc", optional=True) is not None and loss_acc.numel() < 3:
        raise ValueError("WARP loss_acc holds three float32")
    _triplet_ids("WARP", U, I, users, pos, neg, check_ids)
    return d, B


def warp_step(U, I, users, pos, neg, coef, gU, gI, tagU, tagI, *, margin: float, regs: float, reg_div: float, step: int, grouped: bool = False,
              users_distinct: bool = False, loss_acc: Optional[torch.Tensor] = None, check_ids: bool = True):
    """pda_warp_step_f32: the batch's gradient of (1 / B) sum coef_t max(0, margin - (u.p - u.n)) over the triplets with coef_t > 0, plus the L2
    term of every valid triplet, summed into gU / gI (rows tagged `step`), no update.  loss_acc float32 [3] += (loss, mf_loss, reg_loss)."""
    d, B = _warp_check(U, I, users, pos, neg, coef, margin, tagU, tagI, loss_acc, check_ids)
    gU, gI = _need(gU, torch.float32, "gU"), _need(gI, torch.float32, "gI")
    if gU.shape != U.shape or gI.shape != I.shape:
        raise ValueError("gU / gI have the shapes of the tables")
    check(_lib.load().pda_warp_step_f32(ptr(U), ptr(I), U.shape[0], I.shape[0], ptr(users), ptr(pos), ptr(neg), ptr(coef), float(margin), B, d,
                                        float(regs), float(reg_div), ptr(gU), ptr(gI), ptr(tagU), ptr(tagI), int(step),
                                        _ips_flags(grouped, users_distinct), ptr(loss_acc), stream_ptr()), "pda_warp_step_f32")


def warp_adam_step(U, mU, vU, gU, tagU, I, mI, vI, gI, tagI, users, pos, neg, coef, *, margin: float, regs: float, reg_div: float, step: int,
                   lr_t: float, beta1=ADAM_BETA1, beta2=ADAM_BETA2, eps=ADAM_EPS, grouped: bool = False, users_distinct: bool = False,
                   cache_policy: int = ADAM_CACHE_AUTO, loss_acc: Optional[torch.Tensor] = None, check_ids: bool = False):
    """pda_warp_adam_step_f32: one WARP train step (the weighted hinge gradients, TF-1.14 dense-decay Adam over both tables) in two launches;
    graph-capturable.  The arguments of adam_step with coef float32 [B] and the margin in place of the popularities."""
    d, B = _warp_check(U, I, users, pos, neg, coef, margin, tagU, tagI, loss_acc, check_ids)
    for t in (mU, vU, gU, mI, vI, gI):
        _need(t, torch.float32, "adam state")
    if not (mU.shape == vU.shape == gU.shape == U.shape and mI.shape == vI.shape == gI.shape == I.shape):
        raise ValueError("the Adam state tables have the shapes of U and I")
    check(_lib.load().pda_warp_adam_step_f32(ptr(U), ptr(mU), ptr(vU), ptr(gU), ptr(tagU), U.shape[0], ptr(I), ptr(mI), ptr(vI), ptr(gI), ptr(tagI),
                                             I.shape[0], ptr(users), ptr(pos), ptr(neg), ptr(coef), float(margin), B, d, float(regs), float(reg_div),
                                             int(step), float(lr_t), beta1, beta2, eps, _ips_flags(grouped, users_distinct), int(cache_policy),
                                             ptr(loss_acc), stream_ptr()), "pda_warp_adam_step_f32")
    mark_modified(U, I)


# ---- popularity-weighted negative sampling (include/pda_hip_negpop.h) -------------------------------------------------------------------------
NEGPOP_MAX_POWER = 4.0


def negpop_weights(counts, power: float):
    """w_i = (c_i + 1)^power in float64: the + 1 keeps an item without train pairs drawable, power 0 is exactly uniform (every w is 1.0)."""
    import numpy as np
    power = float(power)
    if not (math.isfinite(power) and 0.0 <= power <= NEGPOP_MAX_POWER):
        raise ValueError(f"negative sampler: the popularity power must be a finite number in [0, {NEGPOP_MAX_POWER:g}], got {power}")
    return (np.asarray(counts, dtype=np.float64) + 1.0) ** power


def negpop_alias(w):
    """Vose's alias method on weights w > 0 (float64 [n]) -> (thr uint32 [n], alias uint32 [n]).  p = w n / sum(w); while both work lists
    hold slots, a slot with p < 1 takes thr = min(rint(p 2^32), 2^32 - 1) and the slot with p >= 1 whose turn it is as its alias, which keeps
    (p_large + p_small) - 1.  Whatever is left when one list runs dry is full: alias == slot (thr 2^32 - 1, never looked at)."""
    import numpy as np
    w = np.asarray(w, dtype=np.float64)
    n = w.size
    if n < 1 or not np.isfinite(w).all() or not (w > 0).all():
        raise ValueError("negpop_alias: finite weights > 0, at least one")
    p = w * n / w.sum()
    thr = np.full(n, 2 ** 32 - 1, dtype=np.uint64)
    alias = np.arange(n, dtype=np.uint64)
    small = np.flatnonzero(p < 1.0).tolist()
    large = np.flatnonzero(p >= 1.0).tolist()
    p = p.tolist()
    while small and large:
        s, l = small.pop(), large.pop()
        thr[s] = min(int(np.rint(p[s] * 4294967296.0)), 2 ** 32 - 1)
        alias[s] = l
        p[l] = (p[l] + p[s]) - 1.0
        (large if p[l] >= 1.0 else small).append(l)
    return thr.astype(np.uint32), alias.astype(np.uint32)


class NegPopTable:
    """The proposal of `--neg_sampler pop` over the sampler's range [neg_lo, neg_hi): q_i ~ (c_i + 1)^power, c_i the number of entries of the
    train CSR that hold item i.  Built once per run on the host in float64.
        table   uint64 [n] on `device` (held as int64): low word thr, high word alias (a slot of [0, n)); alias == slot: the slot is full
        q       numpy float64 [n_items], zero outside the range
        logq    numpy float32 [n_items]; an item with q = 0 takes the log of the smallest positive q (as inbatch_logq does)
    from_slots builds one from hand-made (thr, alias).  Every table is refused unless alias < n: the kernels index with it."""

    def __init__(self, train_indices, n_items: int, power: float, neg_range, device):
        import numpy as np
        idx = train_indices.cpu().numpy() if torch.is_tensor(train_indices) else np.asarray(train_indices)
        n_items = int(n_items)
        lo, hi = int(neg_range[0]), int(neg_range[1])
        if not 0 <= lo < hi <= n_items:
            raise ValueError(f"NegPopTable: neg_range = (lo, hi) with 0 <= lo < hi <= n_items = {n_items}, got ({lo}, {hi})")
        if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= n_items):
            raise ValueError("NegPopTable: a train item lies outside [0, n_items)")
        counts = np.bincount(idx.astype(np.int64), minlength=n_items)
        w = negpop_weights(counts[lo:hi], power)
        thr, alias = negpop_alias(w)
        q = np.zeros(n_items, dtype=np.float64)
        q[lo:hi] = w / w.sum()
        self.power = float(power)
        self._finish(thr, alias, lo, hi, n_items, q, device)

    @classmethod
    def from_slots(cls, thr, alias, neg_range, n_items: int, device, q=None):
        """A table from its slots as they are (thr, alias: n integers below 2^32 each); q: its distribution where the caller has one."""
        import numpy as np
        self = cls.__new__(cls)
        self.power = None
        lo, hi = int(neg_range[0]), int(neg_range[1])
        if not 0 <= lo < hi <= int(n_items):
            raise ValueError(f"NegPopTable: neg_range = (lo, hi) with 0 <= lo < hi <= n_items = {n_items}, got ({lo}, {hi})")
        thr, alias = np.asarray(thr, dtype=np.uint64), np.asarray(alias, dtype=np.uint64)
        if (thr >= 2 ** 32).any():
            raise ValueError("NegPopTable: a threshold does not fit 32 bits")
        self._finish(thr, alias, lo, hi, int(n_items), None if q is None else np.asarray(q, dtype=np.float64), device)
        return self

    def _finish(self, thr, alias, lo, hi, n_items, q, device):
        import numpy as np
        n = hi - lo
        if thr.shape != (n,) or alias.shape != (n,):
            raise ValueError(f"NegPopTable: thr and alias hold one word per item of the range, {n}")
        if (alias.astype(np.uint64) >= n).any():
            raise ValueError(f"NegPopTable: an alias lies outside the table's slots [0, {n})")
        self.neg_range, self.n, self.n_items = (lo, hi), n, n_items
        self.thr, self.alias = thr.astype(np.uint32), alias.astype(np.uint32)
        words = (self.alias.astype(np.uint64) << np.uint64(32)) | self.thr.astype(np.uint64)
        self.table = torch.from_numpy(words.view(np.int64).copy()).to(device)
        self.q = q
        self.logq = None
        if q is not None:
            if q.shape != (n_items,) or not (q > 0).any():
                raise ValueError("NegPopTable: q holds one float64 per item, some of them positive")
            filled = np.where(q > 0, q, q[q > 0].min())
            self.logq = np.log(filled).astype(np.float32)

    def all_full(self) -> bool:
        import numpy as np
        return bool((self.alias == np.arange(self.n, dtype=np.uint32)).all())

    def stats(self):
        """-> (max q, entropy of q in nats, entropy of the uniform distribution over the range)."""
        import numpy as np
        q = self.q[self.q > 0]
        return float(q.max()), float(-(q * np.log(q)).sum()), math.log(self.n)


def _negpop_table(table, train_indptr, pop_matrix=None):
    if not isinstance(table, NegPopTable):
        raise ValueError("negative sampler: table is an ops.NegPopTable")
    if table.table.device != train_indptr.device:
        raise ValueError("negative sampler: the table lives on the device of the train CSR")
    if pop_matrix is not None and (_need(pop_matrix, torch.float32, "pop_matrix").dim() != 2 or pop_matrix.shape[0] < table.neg_range[1]
                                   or pop_matrix.shape[1] < 1):
        raise ValueError("negative sampler: pop_matrix float32 [n_items, n_slots >= 1] covering the table's range")
    return table.neg_range


def negpop_sample_triplets(table, train_indptr, train_indices, B: int, *, seed: int, step: int, users=None, user_pool=None, n_pool: int = 0,
                           train_slots=None, pop_matrix=None):
    """pda_negpop_sample_triplets -> (users, pos, neg, pos_pop|None, neg_pop|None) on the device: sample_triplets with the negative drawn from
    `table` (an ops.NegPopTable; its range is the neg_range).  The outputs are allocated zeroed -- the call writes every element, so this is
    for the reader of a failed call only; the trainer's path is the _into calls on buffers of its own."""
    lo, hi = _negpop_table(table, train_indptr, pop_matrix)
    _need(train_indptr, torch.int64, "train_indptr"), _need(train_indices, torch.int32, "train_indices")
    _need(train_slots, torch.int32, "train_slots", optional=True)
    if int(B) < 1:
        raise ValueError("negative sampler: B >= 1")
    if user_pool is not None and _need(user_pool, torch.int32, "user_pool").numel() < int(n_pool):
        raise ValueError("user_pool holds n_pool int32")
    dev = train_indptr.device
    gen = users is None
    if gen:
        if int(n_pool) < 1:
            raise ValueError("negative sampler: drawing users needs n_pool >= 1")
        users = torch.zeros(B, dtype=torch.int32, device=dev)
    elif _need(users, torch.int32, "users").numel() != B:
        raise ValueError("users holds B int32")
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    neg = torch.zeros(B, dtype=torch.int32, device=dev)
    pp = pn = None
    n_slots = 0
    if pop_matrix is not None:
        n_slots = pop_matrix.shape[1]
        pp, pn = torch.zeros(B, dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.float32, device=dev)
    check(_lib.load().pda_negpop_sample_triplets(ptr(users), int(gen), ptr(user_pool), int(n_pool), int(B), ptr(train_indptr), ptr(train_indices),
                                                 ptr(train_slots), lo, hi, ptr(table.table), ptr(pop_matrix), n_slots, seed & (2 ** 64 - 1),
                                                 int(step) & (2 ** 64 - 1), ptr(pos), ptr(neg), ptr(pp), ptr(pn), stream_ptr()),
          "pda_negpop_sample_triplets")
    return users, pos, neg, pp, pn


def _negpop_out(out, table, train_indptr, pop_matrix, dims: int):
    """The (users, pos, neg, pos_pop|None, neg_pop|None) buffers of the _into calls, [B] (dims 1) or [n, B] (dims 2) each -> n_slots."""
    users, pos, neg, pp, pn = out
    users, pos, neg = _need(users, torch.int32, "users"), _need(pos, torch.int32, "pos"), _need(neg, torch.int32, "neg")
    if users.dim() != dims or pos.shape != users.shape or neg.shape != users.shape or users.numel() < 1:
        raise ValueError("negative sampler output: users, pos and neg of one shape")
    if (pp is None) != (pn is None) or (pp is not None and pop_matrix is None):
        raise ValueError("negative sampler output: pos_pop and neg_pop come together, and with a pop_matrix")
    for t, name in ((pp, "pos_pop"), (pn, "neg_pop")):
        if t is not None and _need(t, torch.float32, name).shape != users.shape:
            raise ValueError(f"{name} has the shape of users")
    if pop_matrix is not None and pp is None:
        raise ValueError("negative sampler output: a pop_matrix needs pos_pop and neg_pop")
    return pop_matrix.shape[1] if pop_matrix is not None else 0


def negpop_sample_triplets_into(out, table, train_indptr, train_indices, *, seed: int, step_dev: torch.Tensor, parity: Optional[int] = None,
                                user_pool=None, n_pool: int = 0, train_slots=None, pop_matrix=None):
    """pda_negpop_sample_triplets_dev: one batch into out = (users, pos, neg, pos_pop|None, neg_pop|None), the step read from device memory
    (graph-capturable; the users are drawn).  step_dev int64 [1]: read only; int64 [2] + parity p: slot p read, step + 1 stored to 1 - p."""
    lo, hi = _negpop_table(table, train_indptr, pop_matrix)
    n_slots = _negpop_out(out, table, train_indptr, pop_matrix, 1)
    if int(n_pool) < 1:
        raise ValueError("negative sampler: drawing users needs n_pool >= 1")
    users, pos, neg, pp, pn = out
    src, nxt = _step_slots(_need(step_dev, torch.int64, "step_dev"), parity)
    check(_lib.load().pda_negpop_sample_triplets_dev(ptr(users), 1, ptr(user_pool), int(n_pool), users.numel(), ptr(train_indptr),
                                                     ptr(train_indices), ptr(train_slots), lo, hi, ptr(table.table), ptr(pop_matrix), n_slots,
                                                     seed & (2 ** 64 - 1), ptr(src), ptr(nxt), ptr(pos), ptr(neg), ptr(pp), ptr(pn), stream_ptr()),
          "pda_negpop_sample_triplets_dev")
    return out


def negpop_sample_batches_into(out, table, train_indptr, train_indices, *, seed: int, step_dev: torch.Tensor, parity: int, user_pool=None,
                               n_pool: int = 0, train_slots=None, pop_matrix=None):
    """pda_negpop_sample_batches_dev: sample_batches_into with the negatives drawn from `table`; out as [n, B] tensors, row j the batch of step
    step_dev[parity] + j, step_dev[1 - parity] receives step + n."""
    lo, hi = _negpop_table(table, train_indptr, pop_matrix)
    n_slots = _negpop_out(out, table, train_indptr, pop_matrix, 2)
    if _need(step_dev, torch.int64, "step_dev").numel() != 2 or parity not in (0, 1):
        raise ValueError("negpop_sample_batches_into wants the two-slot step counter and parity 0 or 1")
    if int(n_pool) < 1:
        raise ValueError("negative sampler: drawing users needs n_pool >= 1")
    users, pos, neg, pp, pn = out
    n, B = users.shape
    if not all(t is None or t.is_contiguous() for t in out):
        raise ValueError("negative sampler output: contiguous [n, B] buffers")
    check(_lib.load().pda_negpop_sample_batches_dev(ptr(users), 1, ptr(user_pool), int(n_pool), B, n, ptr(train_indptr), ptr(train_indices),
                                                    ptr(train_slots), lo, hi, ptr(table.table), ptr(pop_matrix), n_slots, seed & (2 ** 64 - 1),
                                                    ptr(step_dev[parity:parity + 1]), ptr(step_dev[1 - parity:2 - parity]), ptr(pos), ptr(neg),
                                                    ptr(pp), ptr(pn), stream_ptr()), "pda_negpop_sample_batches_dev")
    return out


def negpop_ssm_sample(table, train_indptr, train_indices, B: int, N: int, *, seed: int, step: int, users=None, user_pool=None, n_pool: int = 0):
    """pda_negpop_ssm_sample -> (users, pos, negs [B, N]) on the device: ssm_sample with the negatives drawn from `table`; column 0 is the
    negative of negpop_sample_triplets."""
    lo, hi = _negpop_table(table, train_indptr)
    _ssm_sample_args(train_indptr, train_indices, B, N, (lo, hi), user_pool, n_pool)
    dev = train_indptr.device
    gen = users is None
    if gen:
        if int(n_pool) < 1:
            raise ValueError("negative sampler: drawing users needs n_pool >= 1")
        users = torch.zeros(B, dtype=torch.int32, device=dev)
    elif _need(users, torch.int32, "users").numel() != B:
        raise ValueError("users holds B int32")
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    negs = torch.zeros((B, N), dtype=torch.int32, device=dev)
    check(_lib.load().pda_negpop_ssm_sample(ptr(users), int(gen), ptr(user_pool), int(n_pool), int(B), int(N), ptr(train_indptr), ptr(train_indices),
                                            lo, hi, ptr(table.table), seed & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), ptr(pos), ptr(negs),
                                            stream_ptr()), "pda_negpop_ssm_sample")
    return users, pos, negs


def negpop_ssm_sample_into(out, table, train_indptr, train_indices, *, seed: int, step_dev: torch.Tensor, parity: Optional[int] = None,
                           user_pool=None, n_pool: int = 0):
    """pda_negpop_ssm_sample_dev: one batch into out = (users [B], pos [B], negs [B, N]), the step read from device memory (ssm_sample_into)."""
    lo, hi = _negpop_table(table, train_indptr)
    users, pos, negs = out
    users, pos, negs = _need(users, torch.int32, "users"), _need(pos, torch.int32, "pos"), _need(negs, torch.int32, "negs")
    B = users.numel()
    if pos.numel() != B or negs.dim() != 2 or negs.shape[0] != B:
        raise ValueError("negative sampler output: users [B], pos [B], negs [B, N]")
    _ssm_sample_args(train_indptr, train_indices, B, negs.shape[1], (lo, hi), user_pool, n_pool)
    if int(n_pool) < 1:
        raise ValueError("negative sampler: drawing users needs n_pool >= 1")
    src, nxt = _step_slots(_need(step_dev, torch.int64, "step_dev"), parity)
    check(_lib.load().pda_negpop_ssm_sample_dev(ptr(users), 1, ptr(user_pool), int(n_pool), B, int(negs.shape[1]), ptr(train_indptr),
                                                ptr(train_indices), lo, hi, ptr(table.table), seed & (2 ** 64 - 1), ptr(src), ptr(nxt), ptr(pos),
                                                ptr(negs), stream_ptr()), "pda_negpop_ssm_sample_dev")
    return out


# ---- iALS (include/pda_hip_ials.h) ---------------------------------------------------------------------------------------------------------------
IALS_EMBED_SIZES = (32, 64, 128)
IALS_CHUNK = _lib.IALS_CHUNK                  # PDA_IALS_CHUNK: a row with more pairs is cut into chunks of this many
IALS_GRAM_ROWS = _lib.IALS_GRAM_ROWS          # PDA_IALS_GRAM_ROWS: rows of Z per partial Gram matrix


def check_ials_params(lam, alpha0, nu):
    lam, alpha0, nu = float(lam), float(alpha0), float(nu)
    if not (lam > 0.0 and math.isfinite(lam)):
        raise ValueError(f"iALS: lambda must be a finite number > 0, got {lam}")
    if not (alpha0 >= 0.0 and math.isfinite(alpha0)):
        raise ValueError(f"iALS: alpha0 must be a finite number >= 0, got {alpha0}")
    if not 0.0 <= nu <= 1.0:
        raise ValueError(f"iALS: nu must lie in 0 .. 1, got {nu}")
    return lam, alpha0, nu


def ials_lam_row(deg, n_other: int, lam: float, alpha0: float, nu: float):
    """lambda_r = fl32(lambda * float64(n_r + alpha0 n_other)^nu), numpy float32 [n_rows]: rounded once, an input of the kernels."""
    import numpy as np
    lam, alpha0, nu = check_ials_params(lam, alpha0, nu)
    return (lam * np.power(np.asarray(deg, dtype=np.float64) + alpha0 * float(n_other), nu)).astype(np.float32)


# item-weighted iALS (include/pda_hip_ials_itemw.h): --ials_item_power
IALS_ITEM_POWER_MAX = 4.0


def check_ials_item_power(power) -> float:
    power = float(power)
    if not (math.isfinite(power) and 0.0 <= power <= IALS_ITEM_POWER_MAX):
        raise ValueError(f"iALS: the item power must be a finite number in [0, {IALS_ITEM_POWER_MAX:g}], got {power}")
    return power


def ials_item_weight_arrays(counts, power: float, alpha0: float) -> dict:
    """The per-item inputs of the item-weighted model on the host (numpy; no GPU needed), from the items' distinct train pairs c_i:
    q = (c + 1)^power / sum (float64, negpop_weights), scale = fl32(sqrt(n_items q)), w = float64(scale)^2 (THE weight of the model, mean 1
    up to rounding) and alpha_row = fl32(alpha0 w).  power 0: scale = w = 1 exactly and alpha_row = fl32(alpha0)."""
    import numpy as np
    power = check_ials_item_power(power)
    alpha0 = float(alpha0)
    if not (alpha0 >= 0.0 and math.isfinite(alpha0)):
        raise ValueError(f"iALS: alpha0 must be a finite number >= 0, got {alpha0}")
    counts = np.asarray(counts)
    if counts.ndim != 1 or counts.size < 1 or not (counts >= 0).all():
        raise ValueError("iALS item weights: one count >= 0 per item, at least one item")
    p = negpop_weights(counts, power)
    q = p / p.sum()
    scale = np.sqrt(float(p.size) * q).astype(np.float32)
    w = scale.astype(np.float64) ** 2
    alpha_row = (alpha0 * w).astype(np.float32)
    if not (np.isfinite(scale).all() and (scale > 0).all() and np.isfinite(alpha_row).all()):
        raise ValueError("iALS item weights: the weights left the range of float32")
    return dict(q=q, scale=scale, w=w, alpha_row=alpha_row)


class IalsItemWeights:
    """The per-item weights of an item-weighted iALS graph (ials_item_weight_arrays): `w` float64 [n_items] on the host, `scale` and
    `alpha_row` float32 [n_items] on the device (host_scale, host_alpha_row: their host copies)."""

    def __init__(self, counts, power: float, alpha0: float, device):
        h = ials_item_weight_arrays(counts, power, alpha0)
        self.power, self.alpha0 = float(power), float(alpha0)
        self.w, self.host_scale, self.host_alpha_row = h["w"], h["scale"], h["alpha_row"]
        self.scale = torch.from_numpy(h["scale"]).to(device)
        self.alpha_row = torch.from_numpy(h["alpha_row"]).to(device)


def ials_lam_row_items(deg, n_users: int, lam: float, alpha0: float, nu: float, w):
    """The item side's lam_row of the item-weighted model: fl32(lambda * float64(n_i + alpha0 w_i n_users)^nu); w all 1 is ials_lam_row."""
    import numpy as np
    lam, alpha0, nu = check_ials_params(lam, alpha0, nu)
    return (lam * np.power(np.asarray(deg, dtype=np.float64) + alpha0 * np.asarray(w, dtype=np.float64) * float(n_users), nu)).astype(np.float32)


def ials_graph_arrays(users, items, n_users: int, n_items: int, chunk: int = IALS_CHUNK) -> dict:
    """Both CSR directions and both work lists of include/pda_hip_ials.h from the train pairs, on the host (numpy; no GPU needed): what
    gcn_graph_arrays yields for the stacked graph, taken apart into the user side (rows: users, columns: item ids) and the item side (rows:
    items, columns: user ids), each with its own pair offsets and slot numbers.  Every list keeps gcn_graph_arrays' order: falling length,
    rows and chunks rising among equals."""
    import numpy as np
    h = gcn_graph_arrays(users, items, n_users, n_items, chunk)
    nu_, nnz = h["n_users"], int(h["edge_w"].shape[0])
    ip, ix, work, lr = h["indptr"], h["indices"], h["work"], h["long_rows"]
    u_slots = int(lr[lr[:, 0] < nu_, 2].sum())
    sides = {}
    for name, r0, n, e0, s0, col0 in (("user", 0, nu_, 0, 0, nu_), ("item", nu_, h["n_items"], nnz, u_slots, 0)):
        wk = work[(work[:, 0] >= r0) & (work[:, 0] < r0 + n)].copy()
        wk[:, 0] -= r0
        wk[:, 1:3] -= e0
        wk[:, 3] = np.where(wk[:, 3] >= 0, wk[:, 3] - s0, -1)
        l = lr[(lr[:, 0] >= r0) & (lr[:, 0] < r0 + n)].copy()
        l[:, 0] -= r0
        l[:, 1] -= s0
        indptr = (ip[r0:r0 + n + 1] - e0).astype(np.int64)
        sides[name] = dict(n_rows=n, n_other=h["n_items"] if name == "user" else nu_, indptr=np.ascontiguousarray(indptr),
                           indices=np.ascontiguousarray((ix[e0:e0 + nnz] - col0).astype(np.int32)), deg=np.diff(indptr),
                           work=np.ascontiguousarray(wk), long_rows=np.ascontiguousarray(l), n_slots=int(l[:, 2].sum()))
    return dict(n_users=nu_, n_items=h["n_items"], chunk=int(chunk), nnz=nnz, user=sides["user"], item=sides["item"])


class IalsWork:
    """A work list of one side on the device: `work` int64 [n_work, 4], `long_rows` int64 [n_long, 3], n_slots."""

    def __init__(self, work, long_rows, n_slots: int, device):
        self.host_work, self.host_long_rows, self.n_slots = work, long_rows, int(n_slots)
        self.work = torch.from_numpy(work).to(device)
        self.long_rows = torch.from_numpy(long_rows).to(device)
        self.n_work, self.n_long = int(work.shape[0]), int(long_rows.shape[0])


class IalsSide:
    """One side of an IalsGraph: its CSR (int64 indptr, int32 column ids ascending), degrees, lam_row and the work list of all its rows."""

    def __init__(self, h: dict, lam_row, device):
        self.host, self.device = h, device
        self.n_rows, self.n_other, self.nnz = int(h["n_rows"]), int(h["n_other"]), int(h["indices"].shape[0])
        self.indptr, self.indices = torch.from_numpy(h["indptr"]).to(device), torch.from_numpy(h["indices"]).to(device)
        self.host_lam_row = lam_row
        self.lam_row = torch.from_numpy(lam_row).to(device)
        self.all_rows = IalsWork(h["work"], h["long_rows"], h["n_slots"], device)

    def sub_list(self, rows, shuffle_seed=None) -> IalsWork:
        """The work list of the given rows alone (every entry of the side's own list whose row is among them, slots renumbered from 0),
        optionally in a shuffled order: what a call needs to solve a subset of the rows."""
        import numpy as np
        rows = np.unique(np.asarray(rows, dtype=np.int64))
        if rows.size == 0 or rows[0] < 0 or rows[-1] >= self.n_rows:
            raise ValueError("iALS work list: row ids inside the side, at least one")
        wk = self.host["work"][np.isin(self.host["work"][:, 0], rows)].copy()
        lr = self.host["long_rows"][np.isin(self.host["long_rows"][:, 0], rows)].copy()
        new0 = np.cumsum(lr[:, 2]) - lr[:, 2]
        for (r, s0, n), t0 in zip(lr.tolist(), new0.tolist()):
            m = wk[:, 0] == r
            wk[m, 3] += t0 - s0
        lr[:, 1] = new0
        if shuffle_seed is not None:
            g = np.random.default_rng(shuffle_seed)
            wk, lr = wk[g.permutation(len(wk))], lr[g.permutation(len(lr))]
        return IalsWork(np.ascontiguousarray(wk), np.ascontiguousarray(lr), int(lr[:, 2].sum()), self.device)


class IalsGraph:
    """The train pairs of an iALS model on the device, built once (ials_graph_arrays): both CSRs, both work lists, the degrees and lam_row of
    both sides for the given (lambda, alpha0, nu).  Ids and shapes are validated here, on the host, once: the kernels trust the graph.  It also
    owns what the calls write besides the tables: the workspace, the Gram matrix, the per-row loss terms and the failed-pivot counter, one set
    per row width.  item_power > 0 (include/pda_hip_ials_itemw.h): the graph also holds item_weights, an IalsItemWeights from the items' degrees,
    the item side's lam_row follows from its w, and every call on the graph that is not told otherwise runs the item-weighted model; at 0
    item_weights is None and nothing else is built or called."""

    def __init__(self, users, items, n_users: int, n_items: int, device, *, lam: float, alpha0: float = 0.1, nu: float = 1.0,
                 chunk: int = IALS_CHUNK, item_power: float = 0.0):
        self.lam, self.alpha0, self.nu = check_ials_params(lam, alpha0, nu)
        self.item_power = check_ials_item_power(item_power)
        h = self.host = ials_graph_arrays(users, items, n_users, n_items, chunk)
        self.n_users, self.n_items, self.nnz, self.chunk = h["n_users"], h["n_items"], h["nnz"], h["chunk"]
        self.device = torch.device(device)
        self.user = IalsSide(h["user"], ials_lam_row(h["user"]["deg"], self.n_items, self.lam, self.alpha0, self.nu), self.device)
        self.item_weights = None
        if self.item_power > 0.0:
            self.item_weights = IalsItemWeights(h["item"]["deg"], self.item_power, self.alpha0, self.device)
            lam_items = ials_lam_row_items(h["item"]["deg"], self.n_users, self.lam, self.alpha0, self.nu, self.item_weights.w)
        else:
            lam_items = ials_lam_row(h["item"]["deg"], self.n_users, self.lam, self.alpha0, self.nu)
        self.item = IalsSide(h["item"], lam_items, self.device)
        self._bufs = {}

    def side(self, side) -> IalsSide:
        if side not in ("user", "item"):
            raise ValueError(f"iALS: side must be 'user' or 'item', got {side!r}")
        return self.user if side == "user" else self.item

    # the block solver's state (include/pda_hip_ialspp.h), built on first use: an exact-solver run never touches it
    @property
    def pair_perm(self):
        """int64 [nnz] on the device: position in the item CSR -> position of the same pair in the user CSR."""
        return ialspp_pair_perm(self)

    @property
    def e(self):
        """The prediction cache of the block solver, float32 [nnz] in the user CSR's pair order."""
        return ialspp_cache(self)

    def blocks(self, d: int, k: int):
        """The first coordinates of the d / k blocks, ascending."""
        return ialspp_blocks(d, k)

    def buffers(self, d: int) -> dict:
        if d not in self._bufs:
            gram_slots = -(-max(self.n_users, self.n_items) // IALS_GRAM_ROWS)
            slots = max(gram_slots, self.user.all_rows.n_slots, self.item.all_rows.n_slots)
            nbytes = _lib.load().pda_ials_workspace_bytes(slots, d)
            self._bufs[d] = dict(ws=torch.empty(max(1, nbytes), dtype=torch.uint8, device=self.device),
                                 G=torch.empty((d, d), dtype=torch.float32, device=self.device),
                                 rows=torch.empty((self.n_users, 3), dtype=torch.float32, device=self.device),
                                 fail=torch.zeros(1, dtype=torch.int32, device=self.device))
        return self._bufs[d]


def _ials_row_vector(t, n_rows: int, what: str):
    t = _need(t, torch.float32, what)
    if t.dim() != 1 or t.numel() != n_rows:
        raise ValueError(f"iALS: {what} is float32 [{n_rows}], got {tuple(t.shape)}")
    return t


def _ials_graph_inputs(graph: "IalsGraph", side: str, alpha_row):
    """(scale for the Gram matrix of the table held fixed | None, alpha_row | None) of a call on `side`: what the caller handed over, or on an
    item-weighted graph the graph's own -- the user side solves against G_w, the item side with its alpha_row."""
    iw = graph.item_weights
    if alpha_row is None and iw is not None and side == "item":
        alpha_row = iw.alpha_row
    return (iw.scale if iw is not None and side == "user" else None), alpha_row


def _ials_table(t, n_rows: int, what: str):
    t = _need(t, torch.float32, what)
    if t.dim() != 2 or t.shape[0] != n_rows or t.shape[1] not in IALS_EMBED_SIZES:
        raise ValueError(f"iALS: {what} is float32 [{n_rows}, d] with d one of {IALS_EMBED_SIZES}, got {tuple(t.shape)}")
    return t


def ials_gram(Z, G=None, workspace=None, scale=None):
    """pda_ials_gram_f32: G = Z^T Z, float32 [d, d], partial Gram matrices over blocks of IALS_GRAM_ROWS rows added in block order.
    scale float32 [n] (pda_ials_gram_scaled_f32): the row c enters as fl(scale[c] z_c), G = sum (s z)(s z)^T."""
    Z = _need(Z, torch.float32, "Z")
    if Z.dim() != 2 or Z.shape[0] < 1 or Z.shape[1] not in IALS_EMBED_SIZES:
        raise ValueError(f"iALS: Z is float32 [n >= 1, d] with d one of {IALS_EMBED_SIZES}, got {tuple(Z.shape)}")
    n, d = Z.shape
    if G is None:
        G = torch.empty((d, d), dtype=torch.float32, device=Z.device)
    if _need(G, torch.float32, "G").shape != (d, d):
        raise ValueError("iALS: G is float32 [d, d]")
    nbytes = _lib.load().pda_ials_workspace_bytes(-(-n // IALS_GRAM_ROWS), d)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=Z.device)
    if _need(workspace, torch.uint8, "workspace").numel() < nbytes:
        raise ValueError(f"iALS: the Gram workspace holds {nbytes} bytes")
    if scale is not None:
        scale = _ials_row_vector(scale, n, "scale")
        check(_lib.load().pda_ials_gram_scaled_f32(ptr(Z), ptr(scale), n, d, ptr(G), ptr(workspace), workspace.numel() // 4, stream_ptr()),
              "pda_ials_gram_scaled_f32")
        return G
    check(_lib.load().pda_ials_gram_f32(ptr(Z), n, d, ptr(G), ptr(workspace), workspace.numel(), stream_ptr()), "pda_ials_gram_f32")
    return G


def ials_half_sweep(graph: IalsGraph, side: str, Z, X_out, *, G=None, work: Optional[IalsWork] = None, dbg_normal=None, fail_count=None,
                    alpha_row=None):
    """pda_ials_half_sweep_f32: X_out[r] = A_r^{-1} b_r for the rows of `work` (default: every row of the side), Z the other table held fixed.
    G: Z^T Z (computed here into the graph's buffer when missing).  dbg_normal float32 [n_rows, d * d + d]: receives (A_r, b_r) as they enter
    the factorisation.  fail_count int32 [1] (default: the graph's own) is raised once per row with a failed pivot.  alpha_row float32 [n_rows]
    (pda_ials_half_sweep_rowalpha_f32): the row's own weight in place of alpha0.  On an item-weighted graph the user side's G defaults to G_w
    and the item side's alpha_row to the graph's own.  Returns X_out."""
    s = graph.side(side)
    gram_scale, alpha_row = _ials_graph_inputs(graph, side, alpha_row)
    Z = _ials_table(Z, s.n_other, "Z (the table held fixed)")
    X_out = _ials_table(X_out, s.n_rows, "X_out")
    d = Z.shape[1]
    if X_out.shape[1] != d or X_out.data_ptr() == Z.data_ptr():
        raise ValueError("iALS: X_out and Z are two tables of one width")
    b = graph.buffers(d)
    if G is None:
        G = ials_gram(Z, b["G"], b["ws"], gram_scale)
    if _need(G, torch.float32, "G").shape != (d, d):
        raise ValueError("iALS: G is float32 [d, d]")
    w = s.all_rows if work is None else work
    if not isinstance(w, IalsWork):
        raise TypeError("iALS: work is an IalsWork of this side (IalsSide.sub_list)")
    if dbg_normal is not None and tuple(_need(dbg_normal, torch.float32, "dbg_normal").shape) != (s.n_rows, d * d + d):
        raise ValueError(f"iALS: dbg_normal is float32 [{s.n_rows}, {d * d + d}]")
    fail = b["fail"] if fail_count is None else _need(fail_count, torch.int32, "fail_count")
    if fail.numel() < 1:
        raise ValueError("iALS: fail_count holds one int32")
    nbytes = _lib.load().pda_ials_workspace_bytes(w.n_slots, d)
    ws = b["ws"]
    if ws.numel() < nbytes:
        ws = b["ws"] = torch.empty(nbytes, dtype=torch.uint8, device=graph.device)
    if alpha_row is not None:
        alpha_row = _ials_row_vector(alpha_row, s.n_rows, "alpha_row")
        check(_lib.load().pda_ials_half_sweep_rowalpha_f32(ptr(s.indptr), ptr(s.indices) if s.nnz else None, s.n_rows, s.nnz, ptr(w.work), w.n_work,
                                                           ptr(w.long_rows) if w.n_long else None, w.n_long, w.n_slots, ptr(Z), s.n_other, ptr(G), d,
                                                           ptr(alpha_row), ptr(s.lam_row), ptr(X_out), ptr(fail), ptr(dbg_normal),
                                                           ptr(ws) if w.n_slots else None, ws.numel() if w.n_slots else 0, stream_ptr()),
              "pda_ials_half_sweep_rowalpha_f32")
        mark_modified(X_out)
        return X_out
    check(_lib.load().pda_ials_half_sweep_f32(ptr(s.indptr), ptr(s.indices) if s.nnz else None, s.n_rows, s.nnz, ptr(w.work), w.n_work,
                                              ptr(w.long_rows) if w.n_long else None, w.n_long, w.n_slots, ptr(Z), s.n_other, ptr(G), d,
                                              float(graph.alpha0), ptr(s.lam_row), ptr(X_out), ptr(fail), ptr(dbg_normal),
                                              ptr(ws) if w.n_slots else None, ws.numel() if w.n_slots else 0, stream_ptr()),
          "pda_ials_half_sweep_f32")
    mark_modified(X_out)
    return X_out


def ials_loss(graph: IalsGraph, X, Y, *, G=None):
    """The objective of include/pda_hip_ials.h at the tables (X, Y) -> float64 [3] on the device, (L, fit, reg): fit = the squared errors of the
    observed pairs + alpha0 x the squared scores of all pairs, reg = the regulariser of both sides, L = fit + reg.  pda_ials_loss_f32 writes the
    three terms of every user row; they are summed here in float64 by torch reductions, as is the item side's regulariser.  G: Y^T Y (computed
    here when missing; G_w on an item-weighted graph, whose objective weighs the scores of item i by alpha0 w_i).  No host read."""
    X, Y = _ials_table(X, graph.n_users, "X"), _ials_table(Y, graph.n_items, "Y")
    d = X.shape[1]
    if Y.shape[1] != d:
        raise ValueError("iALS: X and Y share the embedding width")
    b = graph.buffers(d)
    if G is None:
        G = ials_gram(Y, b["G"], b["ws"], _ials_graph_inputs(graph, "user", None)[0])
    s = graph.user
    check(_lib.load().pda_ials_loss_f32(ptr(s.indptr), ptr(s.indices) if s.nnz else None, s.n_rows, s.nnz, ptr(X), ptr(Y), graph.n_items, ptr(G), d,
                                        ptr(s.lam_row), ptr(b["rows"]), stream_ptr()), "pda_ials_loss_f32")
    t = b["rows"].double().sum(0)
    reg_items = (graph.item.lam_row.double() * Y.double().square().sum(1)).sum()
    fit = t[0] + graph.alpha0 * t[1]
    reg = t[2] + reg_items
    return torch.stack([fit + reg, fit, reg])


# ---- iALS++ (include/pda_hip_ialspp.h): the block-wise solver of the same objective, on the same IalsGraph ------------------------------------------
IALSPP_EMBED_SIZES = (32, 64, 128, 256)
IALSPP_BLOCK_SIZES = (32, 64, 128)


def ials_pair_perm(user_indptr, user_indices, item_indptr, item_indices):
    """pair_perm int64 [nnz] on the host: position q of the item CSR -> position of the same pair in the user CSR (both CSRs hold the distinct
    pairs, column ids ascending within a row, so the user CSR's keys u * n_items + i are ascending)."""
    import numpy as np
    n_users, n_items = len(user_indptr) - 1, len(item_indptr) - 1
    ukey = np.repeat(np.arange(n_users, dtype=np.int64), np.diff(user_indptr)) * n_items + np.asarray(user_indices, dtype=np.int64)
    ikey = np.asarray(item_indices, dtype=np.int64) * n_items + np.repeat(np.arange(n_items, dtype=np.int64), np.diff(item_indptr))
    perm = np.searchsorted(ukey, ikey).astype(np.int64)
    if perm.size and not (perm.max() < ukey.size and np.array_equal(ukey[perm], ikey)):
        raise ValueError("iALS++: the two CSRs do not hold the same pairs")
    return perm


def ialspp_blocks(d: int, k: int):
    """The first coordinates p0 of the d / k blocks of an iALS++ epoch, ascending."""
    d, k = int(d), int(k)
    if d not in IALSPP_EMBED_SIZES:
        raise ValueError(f"iALS++: the embedding size is one of {IALSPP_EMBED_SIZES}, got {d}")
    if k not in IALSPP_BLOCK_SIZES:
        raise ValueError(f"iALS++: the block size is one of {IALSPP_BLOCK_SIZES}, got {k}")
    if d % k:
        raise ValueError(f"iALS++: the block size {k} does not divide the embedding size {d}")
    return list(range(0, d, k))


def _ialspp_state(graph: IalsGraph) -> dict:
    """What the block solver keeps on an IalsGraph besides the exact solver's buffers, built on first use (an exact-solver run never comes
    here): pair_perm, the prediction cache e and, per width, the Gram matrix, its workspace, the loss rows, the slots and the delta buffer.
    Every buffer is a torch.zeros: none needs it (the kernels write what they read), and tests/test_gpu_ialspp.py proves that."""
    st = graph.__dict__.get("_pp")
    if st is None:
        h = graph.host
        perm = ials_pair_perm(h["user"]["indptr"], h["user"]["indices"], h["item"]["indptr"], h["item"]["indices"])
        st = graph.__dict__["_pp"] = dict(pair_perm=torch.from_numpy(perm).to(graph.device), host_pair_perm=perm,
                                          e=torch.zeros(max(1, graph.nnz), dtype=torch.float32, device=graph.device)[:graph.nnz],
                                          fail=torch.zeros(1, dtype=torch.int32, device=graph.device))
    return st


def ialspp_pair_perm(graph: IalsGraph):
    return _ialspp_state(graph)["pair_perm"]


def ialspp_cache(graph: IalsGraph):
    """The graph's prediction cache e, float32 [nnz] in the user CSR's pair order."""
    return _ialspp_state(graph)["e"]


def ialspp_buffers(graph: IalsGraph, d: int, k: Optional[int] = None) -> dict:
    st = _ialspp_state(graph)
    if ("d", d) not in st:
        n = max(graph.n_users, graph.n_items)
        st[("d", d)] = dict(G=torch.zeros((d, d), dtype=torch.float32, device=graph.device),
                            gram_ws=torch.zeros(-(-n // IALS_GRAM_ROWS) * (d * d + d), dtype=torch.float32, device=graph.device),
                            rows=torch.zeros((graph.n_users, 3), dtype=torch.float32, device=graph.device))
    out = dict(st[("d", d)], fail=st["fail"], e=st["e"], pair_perm=st["pair_perm"])
    if k is not None:
        if ("k", k) not in st:
            slots = max(1, graph.user.all_rows.n_slots, graph.item.all_rows.n_slots)
            st[("k", k)] = dict(slots=torch.zeros(slots * (k * k + k), dtype=torch.float32, device=graph.device),
                                delta=torch.zeros(slots * k, dtype=torch.float32, device=graph.device))
        out.update(st[("k", k)])
    return out


def _ialspp_table(t, n_rows: int, what: str):
    t = _need(t, torch.float32, what)
    if t.dim() != 2 or t.shape[0] != n_rows or t.shape[1] not in IALSPP_EMBED_SIZES:
        raise ValueError(f"iALS++: {what} is float32 [{n_rows}, d] with d one of {IALSPP_EMBED_SIZES}, got {tuple(t.shape)}")
    return t


def ialspp_gram(Z, G=None, workspace=None, scale=None):
    """pda_ialspp_gram_f32: G = Z^T Z, float32 [d, d], at the four embedding sizes; workspace float32 of one slot of d * d + d per block of
    IALS_GRAM_ROWS rows.  scale float32 [n] (pda_ials_gram_scaled_f32): the row c enters as fl(scale[c] z_c)."""
    Z = _need(Z, torch.float32, "Z")
    if Z.dim() != 2 or Z.shape[0] < 1 or Z.shape[1] not in IALSPP_EMBED_SIZES:
        raise ValueError(f"iALS++: Z is float32 [n >= 1, d] with d one of {IALSPP_EMBED_SIZES}, got {tuple(Z.shape)}")
    n, d = Z.shape
    if G is None:
        G = torch.zeros((d, d), dtype=torch.float32, device=Z.device)
    if _need(G, torch.float32, "G").shape != (d, d):
        raise ValueError("iALS++: G is float32 [d, d]")
    need = -(-n // IALS_GRAM_ROWS) * (d * d + d)
    if workspace is None:
        workspace = torch.zeros(need, dtype=torch.float32, device=Z.device)
    if _need(workspace, torch.float32, "workspace").numel() < need:
        raise ValueError(f"iALS++: the Gram workspace holds {need} floats")
    if scale is not None:
        scale = _ials_row_vector(scale, n, "scale")
        check(_lib.load().pda_ials_gram_scaled_f32(ptr(Z), ptr(scale), n, d, ptr(G), ptr(workspace), workspace.numel(), stream_ptr()),
              "pda_ials_gram_scaled_f32")
        return G
    check(_lib.load().pda_ialspp_gram_f32(ptr(Z), n, d, ptr(G), ptr(workspace), workspace.numel(), stream_ptr()), "pda_ialspp_gram_f32")
    return G


def ialspp_predict(graph: IalsGraph, X, Y, e=None):
    """pda_ialspp_predict_f32: e[p] = x_u(p) . y_i(p) for every pair of the user CSR (default: into the graph's own cache).  Returns e."""
    X, Y = _ialspp_table(X, graph.n_users, "X"), _ialspp_table(Y, graph.n_items, "Y")
    d = X.shape[1]
    if Y.shape[1] != d:
        raise ValueError("iALS++: X and Y share the embedding width")
    e = ialspp_cache(graph) if e is None else _need(e, torch.float32, "e")
    if e.dim() != 1 or e.numel() != graph.nnz:
        raise ValueError(f"iALS++: e is float32 [{graph.nnz}]")
    s = graph.user
    check(_lib.load().pda_ialspp_predict_f32(ptr(s.indptr), ptr(s.indices) if s.nnz else None, s.n_rows, s.nnz, ptr(X), ptr(Y), graph.n_items, d,
                                             ptr(e) if s.nnz else None, stream_ptr()), "pda_ialspp_predict_f32")
    return e


def ialspp_block_pass(graph: IalsGraph, side: str, Z, X, block: int, k: int, *, G=None, e=None, work: Optional[IalsWork] = None, dbg=None,
                      fail_count=None, slots=None, delta_ws=None, alpha_row=None):
    """pda_ialspp_block_pass_f32: one pass of the coordinate block [block * k, (block + 1) * k) over the rows of `work` (default: every row of
    the side): x_{r,pi} <- the exact minimiser over the block, in place in X, and the rows' entries of the prediction cache e follow.  Z is the
    other table, held fixed; G: Z^T Z (computed here when missing); e: the cache (default: the graph's own, which ialspp_predict fills).
    dbg float32 [n_rows, k * k + k] receives (H, g) as they enter the factorisation.  slots / delta_ws: float32 scratch of n_slots * (k * k + k)
    and n_slots * k floats (default: the graph's own).  alpha_row float32 [n_rows] (pda_ialspp_block_pass_rowalpha_f32): the row's own weight in
    place of alpha0.  On an item-weighted graph the user side's G defaults to G_w and the item side's alpha_row to the graph's own.  Returns X."""
    s = graph.side(side)
    gram_scale, alpha_row = _ials_graph_inputs(graph, side, alpha_row)
    Z = _ialspp_table(Z, s.n_other, "Z (the table held fixed)")
    X = _ialspp_table(X, s.n_rows, "X")
    d = Z.shape[1]
    if X.shape[1] != d or X.data_ptr() == Z.data_ptr():
        raise ValueError("iALS++: X and Z are two tables of one width")
    p0s = ialspp_blocks(d, k)
    block = int(block)
    if not 0 <= block < len(p0s):
        raise ValueError(f"iALS++: block {block} is outside the {len(p0s)} blocks of d = {d}, k = {k}")
    b = ialspp_buffers(graph, d, k)
    if G is None:
        G = ialspp_gram(Z, b["G"], b["gram_ws"], gram_scale)
    if _need(G, torch.float32, "G").shape != (d, d):
        raise ValueError("iALS++: G is float32 [d, d]")
    e = b["e"] if e is None else _need(e, torch.float32, "e")
    if e.dim() != 1 or e.numel() != graph.nnz:
        raise ValueError(f"iALS++: e is float32 [{graph.nnz}]")
    w = s.all_rows if work is None else work
    if not isinstance(w, IalsWork):
        raise TypeError("iALS++: work is an IalsWork of this side (IalsSide.sub_list)")
    if dbg is not None and tuple(_need(dbg, torch.float32, "dbg").shape) != (s.n_rows, k * k + k):
        raise ValueError(f"iALS++: dbg is float32 [{s.n_rows}, {k * k + k}]")
    fail = b["fail"] if fail_count is None else _need(fail_count, torch.int32, "fail_count")
    if fail.numel() < 1:
        raise ValueError("iALS++: fail_count holds one int32")
    slots = b["slots"] if slots is None else _need(slots, torch.float32, "slots")
    delta_ws = b["delta"] if delta_ws is None else _need(delta_ws, torch.float32, "delta_ws")
    if slots.numel() < w.n_slots * (k * k + k) or delta_ws.numel() < w.n_slots * k:
        raise ValueError(f"iALS++: {w.n_slots} slots need {w.n_slots * (k * k + k)} and {w.n_slots * k} floats")
    perm = b["pair_perm"] if side == "item" else None
    if alpha_row is not None:
        alpha_row = _ials_row_vector(alpha_row, s.n_rows, "alpha_row")
        check(_lib.load().pda_ialspp_block_pass_rowalpha_f32(ptr(s.indptr), ptr(s.indices) if s.nnz else None, ptr(perm), s.n_rows, s.nnz, ptr(w.work),
                                                             w.n_work, ptr(w.long_rows) if w.n_long else None, w.n_long, w.n_slots, ptr(Z), s.n_other,
                                                             ptr(G), d, k, p0s[block], ptr(alpha_row), ptr(s.lam_row), ptr(X),
                                                             ptr(e) if s.nnz else None, ptr(fail), ptr(dbg), ptr(slots) if w.n_slots else None,
                                                             slots.numel() if w.n_slots else 0, ptr(delta_ws) if w.n_slots else None,
                                                             delta_ws.numel() if w.n_slots else 0, stream_ptr()),
              "pda_ialspp_block_pass_rowalpha_f32")
        mark_modified(X)
        return X
    check(_lib.load().pda_ialspp_block_pass_f32(ptr(s.indptr), ptr(s.indices) if s.nnz else None, ptr(perm), s.n_rows, s.nnz, ptr(w.work), w.n_work,
                                                ptr(w.long_rows) if w.n_long else None, w.n_long, w.n_slots, ptr(Z), s.n_other, ptr(G), d, k,
                                                p0s[block], float(graph.alpha0), ptr(s.lam_row), ptr(X), ptr(e) if s.nnz else None, ptr(fail),
                                                ptr(dbg), ptr(slots) if w.n_slots else None, slots.numel() if w.n_slots else 0,
                                                ptr(delta_ws) if w.n_slots else None, delta_ws.numel() if w.n_slots else 0, stream_ptr()),
          "pda_ialspp_block_pass_f32")
    mark_modified(X)
    return X


def ialspp_loss(graph: IalsGraph, X, Y, *, G=None, rows=None):
    """ials_loss at the four embedding sizes (pda_ialspp_loss_f32): float64 [3] on the device, (L, fit, reg), the predictions taken fresh from
    the tables.  rows float32 [n_users, 3]: the per-row terms (default: the graph's own buffer)."""
    X, Y = _ialspp_table(X, graph.n_users, "X"), _ialspp_table(Y, graph.n_items, "Y")
    d = X.shape[1]
    if Y.shape[1] != d:
        raise ValueError("iALS++: X and Y share the embedding width")
    b = ialspp_buffers(graph, d)
    if G is None:
        G = ialspp_gram(Y, b["G"], b["gram_ws"], _ials_graph_inputs(graph, "user", None)[0])
    rows = b["rows"] if rows is None else _need(rows, torch.float32, "rows")
    if tuple(rows.shape) != (graph.n_users, 3):
        raise ValueError(f"iALS++: rows is float32 [{graph.n_users}, 3]")
    s = graph.user
    check(_lib.load().pda_ialspp_loss_f32(ptr(s.indptr), ptr(s.indices) if s.nnz else None, s.n_rows, s.nnz, ptr(X), ptr(Y), graph.n_items, ptr(G), d,
                                          ptr(s.lam_row), ptr(rows), stream_ptr()), "pda_ialspp_loss_f32")
    t = rows.double().sum(0)
    reg_items = (graph.item.lam_row.double() * Y.double().square().sum(1)).sum()
    fit = t[0] + graph.alpha0 * t[1]
    reg = t[2] + reg_items
    return torch.stack([fit + reg, fit, reg])


def ialspp_epoch(graph: IalsGraph, X, Y, k: int):
    """One iALS++ epoch on the tables (X, Y), in place: the prediction cache recomputed from the tables, then for each block in ascending
    order the user pass (G = Y^T Y) and the item pass (G = X^T X), then the objective from the tables -> float64 [3] (L, fit, reg)."""
    d = X.shape[1]
    p0s = ialspp_blocks(d, k)
    ialspp_predict(graph, X, Y)
    for blk in range(len(p0s)):
        ialspp_block_pass(graph, "user", Y, X, blk, k)
        ialspp_block_pass(graph, "item", X, Y, blk, k)
    return ialspp_loss(graph, X, Y)


# ---- exact ranks of held-out items (include/pda_hip_rank.h) ---------------------------------------------------------------------------------
RANK_TCHUNK = _lib.RANK_TCHUNK


def _rank_args(U, I_shard, users, tgt_indptr, head, pop_shard, hist):
    bf = U is not None and U.dtype == torch.bfloat16
    tdt = torch.bfloat16 if bf else torch.float32
    U, I_shard = _need(U, tdt, "U"), _need(I_shard, tdt, "I_shard")
    users = _need(users, torch.int32, "users")
    tgt_indptr = _need(tgt_indptr, torch.int64, "tgt_indptr")
    pop_shard = _need(pop_shard, torch.float32, "pop_shard", optional=True)
    nu, nloc, d = users.numel(), I_shard.shape[0], I_shard.shape[1]
    if U.shape[1] != d:
        raise ValueError("U and I_shard must share the embed dim")
    if d not in (32, 64, 128, 256):
        raise ValueError(f"ranks support embed sizes 32, 64, 128 and 256, not {d}")
    if head not in (HEAD_RAW, HEAD_POP):
        raise ValueError("ranks are taken by the raw head or the popularity head")
    if head == HEAD_POP:
        if pop_shard is None or pop_shard.numel() != nloc:
            raise ValueError("pop_shard must hold one value per local item row")
        _check_pop(pop_shard)
    if nu == 0 or nloc == 0:
        raise ValueError("empty user block or item shard")
    if tgt_indptr.numel() != nu + 1:
        raise ValueError("tgt_indptr holds one row per user of the block")
    if hist is not None and hist.indices.numel() == 0:
        hist = None
    head_args = (ptr(U), ptr(I_shard), ptr(pop_shard), ptr(users), nu)
    hist_args = (ptr(hist.indptr) if hist else None, ptr(hist.indices) if hist else None, hist.mode if hist else 0)
    return bf, nloc, d, head_args, hist_args


def rank_max_row(tgt_indptr) -> int:
    """The longest row of a target CSR (one device -> host read)."""
    return int((tgt_indptr[1:] - tgt_indptr[:-1]).max().item()) if tgt_indptr.numel() > 1 else 0


def rank_keys(U, I_shard, users, tgt_indptr, tgt_indices, head=HEAD_RAW, pop_shard=None, hist: Optional[HistoryCSR] = None, item_offset=0,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pda_rank_keys_f32 / _bf16: packed keys int64 [n_entries] of the target entries (CSR by block row: int64 indptr, int32 global item ids):
    the entry's key if its item lies in the shard and ranks for its user, 0 if it lies in the shard and does not (listed in the history, head
    value not > -inf).  Entries outside the shard are not written: `out` (zeros when missing) keeps what it held, so the keys of several
    shards collect in one tensor.  No target, no launch."""
    bf, nloc, d, head_args, hist_args = _rank_args(U, I_shard, users, tgt_indptr, head, pop_shard, hist)
    tgt_indices = _need(tgt_indices, torch.int32, "tgt_indices")
    if out is None:
        out = torch.zeros(tgt_indices.numel(), dtype=torch.int64, device=tgt_indices.device)
    out = _need(out, torch.int64, "out")
    if out.numel() != tgt_indices.numel():
        raise ValueError("out holds one key per target entry")
    if tgt_indices.numel() == 0:
        return out
    lib = _lib.load()
    fn = lib.pda_rank_keys_bf16 if bf else lib.pda_rank_keys_f32
    check(fn(*head_args, int(item_offset), nloc, d, *hist_args, ptr(tgt_indptr), ptr(tgt_indices), int(head), ptr(out), stream_ptr()),
          "pda_rank_keys_bf16" if bf else "pda_rank_keys_f32")
    return out


def rank_count(U, I_shard, users, tgt_indptr, tgt_keys, head=HEAD_RAW, pop_shard=None, hist: Optional[HistoryCSR] = None, item_offset=0,
               n_splits=0, above: Optional[torch.Tensor] = None, n_ranked: Optional[torch.Tensor] = None, max_row: Optional[int] = None):
    """pda_rank_count_f32 / _bf16 -> (above int32 [n_entries], n_ranked int32 [Bu]), both ADDED to (zeros when missing): above[e] += the ranking
    items of this shard whose key is > tgt_keys[e] (entries with key 0 are left alone), n_ranked[r] += the ranking items of this shard for
    block row r.  max_row: the longest target row if the caller knows it (else one host read)."""
    bf, nloc, d, head_args, hist_args = _rank_args(U, I_shard, users, tgt_indptr, head, pop_shard, hist)
    tgt_keys = _need(tgt_keys, torch.int64, "tgt_keys")
    dev = tgt_keys.device
    if above is None:
        above = torch.zeros(tgt_keys.numel(), dtype=torch.int32, device=dev)
    if n_ranked is None:
        n_ranked = torch.zeros(users.numel(), dtype=torch.int32, device=dev)
    above, n_ranked = _need(above, torch.int32, "above"), _need(n_ranked, torch.int32, "n_ranked")
    if above.numel() != tgt_keys.numel() or n_ranked.numel() != users.numel():
        raise ValueError("above holds one count per target entry and n_ranked one per user of the block")
    if int(n_splits) < 0:
        raise ValueError("n_splits must be >= 0 (0: the call chooses)")
    if max_row is None:
        max_row = rank_max_row(tgt_indptr) if tgt_keys.numel() else 0
    lib = _lib.load()
    fn = lib.pda_rank_count_bf16 if bf else lib.pda_rank_count_f32
    above_arg = above if above.numel() else torch.zeros(1, dtype=torch.int32, device=dev)     # (no entry: the lengths alone; the call wants a buffer)
    check(fn(*head_args, int(item_offset), nloc, d, *hist_args, ptr(tgt_indptr), ptr(tgt_keys), int(max_row), int(head), int(n_splits),
             ptr(above_arg), ptr(n_ranked), stream_ptr()), "pda_rank_count_bf16" if bf else "pda_rank_count_f32")
    return above, n_ranked


def rank_targets(U, I_shard, users, tgt_indptr, tgt_indices, head=HEAD_RAW, pop_shard=None, hist: Optional[HistoryCSR] = None, item_offset=0,
                 n_splits=0, max_row: Optional[int] = None):
    """The exact position of every target entry in its user's masked ranking of the shard -> (rank int32 [n_entries], n_ranked int32 [Bu]).
    rank is 0-based (the number of ranking items above the entry's, value descending, id ascending) and -1 for an entry that does not rank:
    listed in the history, outside the shard, or head value not > -inf.  n_ranked: the length of the row's ranking."""
    keys = rank_keys(U, I_shard, users, tgt_indptr, tgt_indices, head, pop_shard, hist, item_offset)
    above, n_ranked = rank_count(U, I_shard, users, tgt_indptr, keys, head, pop_shard, hist, item_offset, n_splits, max_row=max_row)
    return torch.where(keys != 0, above, torch.full_like(above, -1)), n_ranked
