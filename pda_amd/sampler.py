"""Triplet samplers.

Sampler protocol of the reference (MF/train_new_api.py:178-220, 260-288, 366-412): a zero-argument generator
yielding, per step, a tuple of sequences of length batch_size -- (users, pos, neg) for BPRMF or
(users, pos, neg, pos_pop, neg_pop) for PD/PDA -- exactly `n_train // batch_size + 1` times per epoch (:190).

    host_generator_with_temp   the same for BPRMF(t)-pop (:415-455): (users, pos, neg, temp, raw).
    host_generator   single-process restatement of the reference's Python generators (same distribution:
                     rd.sample users, uniform positive with its time slot, rejection-sampled negative);
                     yields python lists like the reference, for drop-in use and for injecting fixed batches.
    DeviceSampler    pda_sample_triplets (HIP): counter-based, O(B) per batch, tensors never leave HBM.
                     Not stream-identical to the host generators -- parity is defined on injected batches
                     (last bullet).  mode="dice": PNSM, DICE's popularity-margin negative sampler
                     (pda_dice_sample): (users, pos, neg, mask), and the margin's schedule (start_epoch).
                     mode="ssm": the sampled-softmax batches (pda_ssm_sample_dev): (users, pos, negs [B, n_negs]).
                     mode="dns": the batches of mode="bpr" with the negative picked among the topn best-scoring of n_cands
                     uniform candidates under the model's live tables (pda_dns_sample_f32; set_tables).
                     mode="warp": the batches of mode="bpr" with the negative the FIRST of max_trials uniform candidates that violates
                     the margin under the model's live tables (pda_warp_sample_f32; set_tables): (users, pos, neg, coef), coef the
                     rank weight wtab[trials] the WARP step scales the triplet by.
                     neg_table (mode="bpr" | "ssm"): an ops.NegPopTable; the negatives are drawn from its popularity proposal
                     (pda_negpop_*) instead of uniformly, everything else about the batches stays.
    HostDiceSampler  PNSM in numpy, the debugging twin of mode="dice" (--sampler host): the same algorithm on the
                     host's random streams -- NOT draw for draw the device stream.
"""
from __future__ import annotations

import random as rd

import numpy as np
import torch

from . import ops


def n_batches(data) -> int:
    return data.n_train // data.batch_size + 1


def host_generator(data, with_pop: bool):
    """generator_n_batch (:260-288) / generator_n_batch_with_pop (:366-412), one process, one epoch."""
    all_users = list(data.train_user_list.keys())
    bs = data.batch_size
    for _ in range(n_batches(data)):
        if bs <= data.n_users:
            users = rd.sample(all_users, bs)                    # :380-381 unique users
        else:
            users = [rd.choice(all_users) for _ in range(bs)]   # :383
        pos, neg, ppop, npop = [], [], [], []
        for u in users:
            clicked = data.train_user_list[u]
            if not clicked:                                     # :387-390
                p, t = 0, (rd.choice(data.unique_times) if with_pop else 0)
            else:
                idx = np.random.randint(len(clicked))           # :392-396
                p = clicked[idx]
                t = data.train_user_list_time[u][idx] if with_pop else 0
            while True:                                         # :397-401
                n = rd.choice(data.items)
                if n not in clicked:
                    break
            pos.append(p)
            neg.append(n)
            if with_pop:
                ppop.append(data.expo_popularity[p, t])         # :402-403
                npop.append(data.expo_popularity[n, t])
        yield (users, pos, neg, ppop, npop) if with_pop else (users, pos, neg)


def host_generator_with_temp(data):
    """generator_n_batch_with_temp (:415-455), one process, one epoch: (users, pos, neg, temp, raw) -- temp is the time slot of the drawn
    positive (a user without clicks: pos 0 and a slot drawn from unique_times), raw = arange(batch_size)."""
    all_users = list(data.train_user_list.keys())
    bs = data.batch_size
    raw = np.arange(bs)
    for _ in range(n_batches(data)):
        if bs <= data.n_users:
            users = rd.sample(all_users, bs)
        else:
            users = [rd.choice(all_users) for _ in range(bs)]
        pos, neg, temp = [], [], []
        for u in users:
            clicked = data.train_user_list[u]
            if not clicked:
                p, t = 0, rd.choice(data.unique_times)
            else:
                idx = np.random.randint(len(clicked))
                p, t = clicked[idx], data.train_user_list_time[u][idx]
            while True:
                n = rd.choice(data.items)
                if n not in clicked:
                    break
            pos.append(p)
            neg.append(n)
            temp.append(t)
        yield (users, pos, neg, temp, raw)


def to_device_batch(batch, device):
    """Tuple of python lists / numpy arrays (sampler protocol) -> int32/float32 device tensors."""
    out = [torch.as_tensor(np.asarray(b, dtype=np.int32), device=device) for b in batch[:3]]
    if len(batch) == 4:           # DICE: the mask of the triplets
        out.append(torch.as_tensor(np.asarray(batch[3], dtype=np.uint8), device=device))
    if len(batch) == 5:
        out += [torch.as_tensor(np.asarray(b, dtype=np.float32), device=device) for b in batch[3:]]
    return tuple(out)


class DeviceSampler:
    """ahead: batches drawn per sampler launch (pda_sample_batches_dev; the reference's generator thread keeps a queue of
    batches as well, :178-220).  The batches are bit for bit those of ahead = 1 (one pda_sample_triplets launch per step); a
    batch handed out is a row view of the queue and stays valid until `ahead` further batches have been taken."""

    def __init__(self, data, device, with_pop: bool, seed: int = 2020, neg_range=None, ahead: int = 32, temp_slots: int = 0, mode: str = "bpr",
                 margin: float = 40.0, margin_decay: float = 0.9, n_negs: int = 0, n_cands: int = 0, topn: int = 1, neg_table=None,
                 max_trials: int = 0, wtab=None):
        if mode not in ("bpr", "dice", "ssm", "dns", "warp"):
            raise ValueError("DeviceSampler mode must be 'bpr', 'dice', 'ssm', 'dns' or 'warp', not %r" % (mode,))
        if mode == "warp":
            # (margin: the hinge's margin here, PNSM's popularity margin under mode="dice")
            ops.check_warp_sizes(max_trials, margin, "mode='warp'")
            if with_pop or temp_slots > 0:
                raise ValueError("mode='warp' draws (users, pos, neg, coef) for the raw head: no popularity columns (with_pop), no time slots (temp_slots)")
            if not isinstance(wtab, ops.WarpWeights) or wtab.T != int(max_trials):
                raise ValueError("mode='warp': wtab is an ops.WarpWeights built for max_trials = %r" % (max_trials,))
        self.max_trials, self.warp_weights = int(max_trials), wtab
        self._warp_rows = 0
        self.warp_stat = None         # mode="warp": int64 [2] += (sum of trials over rows with a violator, rows without one); take_warp_stat
        if mode == "dns":
            ops.check_dns_sizes(n_cands, topn, "mode='dns'")
        if neg_table is not None:
            if mode not in ("bpr", "ssm"):
                raise ValueError("mode=%r draws its negatives its own way: a neg_table goes with mode='bpr' and mode='ssm' only" % (mode,))
            if not isinstance(neg_table, ops.NegPopTable):
                raise ValueError("neg_table is an ops.NegPopTable")
            if neg_range is not None and tuple(int(x) for x in neg_range) != neg_table.neg_range:
                raise ValueError("neg_range %r is not the range %r the neg_table was built for" % (tuple(neg_range), neg_table.neg_range))
            if neg_range is None and neg_table.neg_range != (0, data.n_items):
                raise ValueError("the neg_table covers %r, the sampler draws from (0, %d): pass the table's neg_range" % (neg_table.neg_range, data.n_items))
        self.neg_table = neg_table
        self.n_cands, self.topn = int(n_cands), int(topn)
        self._tables = None           # mode="dns" | "warp": set_tables
        if mode == "ssm":
            if with_pop or temp_slots > 0:
                raise ValueError("mode='ssm' draws (users, pos, negs): no popularity columns (with_pop), no time slots (temp_slots)")
            if not 1 <= int(n_negs) <= ops.SSM_MAX_NEGS:
                raise ValueError("mode='ssm': n_negs must lie in 1 .. %d, got %r" % (ops.SSM_MAX_NEGS, n_negs))
        self.n_negs = int(n_negs)
        if mode == "dice" and (with_pop or temp_slots > 0 or neg_range is not None):
            raise ValueError("mode='dice' draws (users, pos, neg, mask) over the whole catalogue: no popularity columns, no time slots, no neg_range")
        self.mode = mode
        self.data, self.device, self.with_pop, self.seed = data, torch.device(device), with_pop or temp_slots > 0, seed
        self.indptr, self.indices, self.slots = data.train_csr(self.device)
        self.margin, self.margin_decay = float(margin), float(margin_decay)
        self.dice_pop = ops.DicePop(self.indices, data.n_items) if mode == "dice" else None
        pool = np.fromiter(data.train_user_list.keys(), dtype=np.int32)   # all_users = users with train rows
        self.pool = torch.from_numpy(pool).to(self.device)
        self.pop = None
        if temp_slots > 0:
            # BPRMF(t)-pop: the batch's 4th / 5th outputs carry the positive's time slot as a float, like the reference's placeholder
            # (MF/train_new_api.py:575): the sampler reads a [n_items, T] matrix whose column t holds t.  A user without clicks draws its
            # slot uniformly from [0, T) (the reference: from unique_times, the same set when every slot occurs in train)
            self.pop = torch.arange(temp_slots, dtype=torch.float32, device=self.device).repeat(data.n_items, 1).contiguous()
        elif with_pop:
            self.pop = torch.as_tensor(np.ascontiguousarray(data.expo_popularity, dtype=np.float32), device=self.device)
        # mode="dns": the head the candidates are scored by -- the popularity head on the very matrix the columns are read from (PD/PDA),
        # the raw dot product otherwise (the time-slot matrix of temp_slots is no popularity)
        self.dns_head = ops.HEAD_POP if (with_pop and temp_slots <= 0) else ops.HEAD_RAW
        self.neg_range = neg_range or (0, data.n_items)
        self.step = 0
        self.ahead = max(1, int(ahead))
        self._queue, self._left, self._calls = None, 0, 0
        # users are distinct inside a batch (pda_sample_triplets: a keyed permutation of the pool) as long as the batch is not
        # larger than the pool -- the contract the planned exact SGD step relies on (ops.bpr_step_plan)
        self.distinct_users = data.batch_size <= self.pool.numel()
        self.with_plan = False        # set by the trainer (--optimizer sgd): every batch comes with its pda_triplet_plan
        self.plan = None              # the plan of the batch handed out last

    def _next_queue(self, columns) -> int:
        """The bookkeeping of both refills -> which of the two queues is to be filled (now self._queue).  Two queues in turn: a batch
        handed out stays valid while the next `ahead` are drawn and consumed.  columns: (dtype or None, trailing shape) of each buffer
        of a queue, [ahead, B, ...] each; allocated, with the two-slot device counter, on the first call and when ahead or B changed."""
        B, n = self.data.batch_size, self.ahead
        if self._queue is None or self._queue[0].shape != (n, B):
            self._queues = [tuple(None if dt is None else torch.empty((n, B) + tail, dtype=dt, device=self.device) for dt, tail in columns)
                            for _ in range(2)]
            self._ctr = torch.tensor([self.step, 0], dtype=torch.int64, device=self.device)      # (batch() has counted this one)
            self._calls = self._draws = 0
            self._plans = None
        which = self._calls & 1
        self._queue = self._queues[which]
        self._calls += 1
        self._left = n
        return which

    def _refill_ssm(self):
        """The next `ahead` batches of mode="ssm", one pda_ssm_sample_dev launch each on the two-slot device counter (the protocol of the bpr
        queue; bit for bit the batches of ops.ssm_sample(step = 1, 2, ..))."""
        self._next_queue([(torch.int32, ()), (torch.int32, ()), (torch.int32, (self.n_negs,))])
        for j in range(self.ahead):
            if self.neg_table is not None:
                ops.negpop_ssm_sample_into(tuple(q[j] for q in self._queue), self.neg_table, self.indptr, self.indices, seed=self.seed,
                                           step_dev=self._ctr, parity=self._draws & 1, user_pool=self.pool, n_pool=self.pool.numel())
            else:
                ops.ssm_sample_into(tuple(q[j] for q in self._queue), self.indptr, self.indices, seed=self.seed, step_dev=self._ctr,
                                    parity=self._draws & 1, user_pool=self.pool, n_pool=self.pool.numel(), neg_range=self.neg_range)
            self._draws += 1

    def _refill(self):
        pop_dt = torch.float32 if self.with_pop else None
        which = self._next_queue([(torch.int32, ())] * 3 + [(pop_dt, ())] * 2)
        if self.neg_table is not None:
            ops.negpop_sample_batches_into(self._queue, self.neg_table, self.indptr, self.indices, seed=self.seed, step_dev=self._ctr,
                                           parity=which, user_pool=self.pool, n_pool=self.pool.numel(),
                                           train_slots=self.slots if self.with_pop else None, pop_matrix=self.pop)
        else:
            ops.sample_batches_into(self._queue, self.indptr, self.indices, seed=self.seed, step_dev=self._ctr, parity=which,
                                    user_pool=self.pool, n_pool=self.pool.numel(), train_slots=self.slots if self.with_pop else None,
                                    neg_range=self.neg_range, pop_matrix=self.pop)
        if self.with_plan:
            # the plans of the whole queue in ONE launch (one workgroup per batch), like the batches themselves
            if self._plans is None:
                nb = ops.triplet_plan_bytes(self.data.batch_size)
                self._plans = [torch.empty((self.ahead, nb), dtype=torch.uint8, device=self.device) for _ in range(2)]
            ops.triplet_plan(self._queue[0], self._queue[1], self._queue[2], out=self._plans[which])

    def start_epoch(self, epoch: int) -> float:
        """mode="dice": the margin's schedule -- multiplied by margin_decay at the start of every epoch after the first.  -> the margin."""
        if epoch > 0:
            self.margin *= self.margin_decay
        return self.margin

    def set_tables(self, fn):
        """mode="dns" | "warp": fn() -> (U, I), the LIVE fp32 tables the candidates are scored on (the trainer hands it over once the Recommender
        exists; called at every batch, so it may return new tensors)."""
        self._tables = fn

    def _batch_dns(self):
        """One pda_dns_sample_f32 launch on the tables as they stand: no look-ahead queue, the tables move between steps.  With popularity
        columns the candidates are scored by the popularity head on the matrix the columns are read from, else by the raw dot product."""
        if self._tables is None:
            raise ValueError("mode='dns' scores its candidates on the model's tables: call set_tables(fn) before the first batch")
        U, I = self._tables()
        u, p, n, pp, pn = ops.dns_sample(U, I, self.indptr, self.indices, self.data.batch_size, n_cands=self.n_cands, topn=self.topn,
                                         head=self.dns_head, seed=self.seed, step=self.step,
                                         neg_range=self.neg_range, user_pool=self.pool, n_pool=self.pool.numel(),
                                         train_slots=self.slots if self.with_pop else None, pop_matrix=self.pop)
        self.plan = ops.triplet_plan(u, p, n)[0] if self.with_plan else None
        return (u, p, n, pp, pn) if self.with_pop else (u, p, n)

    def _batch_warp(self):
        """One pda_warp_sample_f32 launch on the tables as they stand: no look-ahead queue, the tables move between steps.  The coefficient
        column travels with the batch; the trial counts go into warp_stat on the device (no host read)."""
        if self._tables is None:
            raise ValueError("mode='warp' scores its candidates on the model's tables: call set_tables(fn) before the first batch")
        U, I = self._tables()
        if self.warp_stat is None:
            self.warp_stat = torch.zeros(2, dtype=torch.int64, device=self.device)
        if self.warp_weights.wtab.device != U.device:
            self.warp_weights.wtab = self.warp_weights.wtab.to(U.device)
        u, p, n, coef = ops.warp_sample(U, I, self.indptr, self.indices, self.data.batch_size, max_trials=self.max_trials, margin=self.margin,
                                        wtab=self.warp_weights.wtab, seed=self.seed, step=self.step, neg_range=self.neg_range,
                                        user_pool=self.pool, n_pool=self.pool.numel(), stat=self.warp_stat)[:4]
        self._warp_rows += self.data.batch_size
        self.plan = None
        return (u, p, n, coef)

    def take_warp_stat(self):
        """mode="warp": (mean trials over the rows with a violator, share of rows without one) since the last call (one host read), and a
        fresh count."""
        if self.warp_stat is None:
            return 0.0, 0.0
        total, none = (int(x) for x in self.warp_stat.tolist())
        rows = self._warp_rows
        self.warp_stat.zero_()
        self._warp_rows = 0
        return total / max(rows - none, 1), none / max(rows, 1)

    def batch(self):
        self.step += 1
        if self.mode == "dns":
            return self._batch_dns()
        if self.mode == "warp":
            return self._batch_warp()
        if self.mode == "dice":     # one pda_dice_sample launch per step; the margin travels by value
            self.plan = None
            return ops.dice_sample(self.indptr, self.indices, self.dice_pop, self.data.batch_size, margin=self.margin, seed=self.seed,
                                   step=self.step, user_pool=self.pool, n_pool=self.pool.numel())
        if self.mode == "ssm":
            if self.with_plan:
                raise ValueError("mode='ssm' has no triplet plan (with_plan): the sampled-softmax step sums its gradients with float atomics")
            self.plan = None
            if self._left == 0:
                self._refill_ssm()
            j = self.ahead - self._left
            self._left -= 1
            return tuple(q[j] for q in self._queue)
        if self.ahead == 1:
            if self.neg_table is not None:
                u, p, n, pp, pn = ops.negpop_sample_triplets(self.neg_table, self.indptr, self.indices, self.data.batch_size, seed=self.seed,
                                                             step=self.step, user_pool=self.pool, n_pool=self.pool.numel(),
                                                             train_slots=self.slots if self.with_pop else None, pop_matrix=self.pop)
            else:
                u, p, n, pp, pn = ops.sample_triplets(self.indptr, self.indices, self.data.batch_size, seed=self.seed,
                                                      step=self.step, user_pool=self.pool, n_pool=self.pool.numel(),
                                                      train_slots=self.slots if self.with_pop else None,
                                                      neg_range=self.neg_range, pop_matrix=self.pop)
            self.plan = ops.triplet_plan(u, p, n)[0] if self.with_plan else None
            return (u, p, n, pp, pn) if self.with_pop else (u, p, n)
        if self._left == 0:
            self._refill()
        j = self.ahead - self._left
        self._left -= 1
        q = self._queue
        self.plan = self._plans[(self._calls - 1) & 1][j] if (self.with_plan and self._plans is not None) else None
        return (q[0][j], q[1][j], q[2][j], q[3][j], q[4][j]) if self.with_pop else (q[0][j], q[1][j], q[2][j])

    def __call__(self):
        """Zero-argument generator: one epoch of device-tensor batches."""
        for _ in range(n_batches(self.data)):
            yield self.batch()


def pnsm_ranges(sorted_pop: np.ndarray, pop_p, margin):
    """PNSM's two ranges of `order` for positives of popularity pop_p (fp32 arithmetic, like the kernel): H = [hi_at, n) holds the items with
    pop > pop_p + margin, L = [0, lo_end) those with pop < pop_p - margin.  -> (hi_at, lo_end)."""
    sp = np.asarray(sorted_pop).astype(np.float32)
    P, M = np.asarray(pop_p).astype(np.float32), np.float32(margin)
    return np.searchsorted(sp, P + M, side="right"), np.searchsorted(sp, P - M, side="left")


class HostDiceSampler:
    """PNSM on the host (--sampler host with --train dice): users and positives like host_generator, the negative from the more popular
    side H or the less popular side L of the positive (a fair coin where both exist, the whole catalogue where neither does), uniform
    inside the side with rejection against the user's train items (REJECT_CAP tries, then the last draw stays).  Yields python lists
    (users, pos, neg, mask).  The algorithm of pda_dice_sample on Python's and numpy's generators: not the device's stream."""
    REJECT_CAP = 4096

    def __init__(self, data, margin: float = 40.0, margin_decay: float = 0.9):
        self.data, self.margin, self.margin_decay = data, float(margin), float(margin_decay)
        pop = np.zeros(data.n_items, dtype=np.int32)
        for items in data.train_user_list.values():
            np.add.at(pop, np.asarray(items, dtype=np.int64), 1)
        self.pop = pop
        self.order = np.lexsort((np.arange(data.n_items), pop)).astype(np.int32)
        self.sorted_pop = pop[self.order]

    def start_epoch(self, epoch: int) -> float:
        if epoch > 0:
            self.margin *= self.margin_decay
        return self.margin

    def draw_negative(self, p: int, clicked):
        """-> (neg, mask) for one positive and the user's train items."""
        n_items = self.data.n_items
        hi_at, lo_end = (int(x) for x in pnsm_ranges(self.sorted_pop, self.pop[p], self.margin))
        nH, nL = n_items - hi_at, lo_end
        whole = nH == 0 and nL == 0
        from_h = nH > 0 and (nL == 0 or rd.random() < 0.5)
        start, span = (0, n_items) if whole else ((hi_at, nH) if from_h else (0, nL))
        clicked = set(clicked)
        for _ in range(self.REJECT_CAP):
            at = start + rd.randrange(span)
            n = at if whole else int(self.order[at])
            if n not in clicked:
                break
        return n, int(self.pop[n] > self.pop[p]) if whole else int(from_h)

    def __call__(self):
        data = self.data
        all_users = list(data.train_user_list.keys())
        bs = data.batch_size
        for _ in range(n_batches(data)):
            users = rd.sample(all_users, bs) if bs <= data.n_users else [rd.choice(all_users) for _ in range(bs)]
            pos, neg, mask = [], [], []
            for u in users:
                clicked = data.train_user_list[u]
                p = clicked[np.random.randint(len(clicked))] if clicked else 0
                n, m = self.draw_negative(p, clicked)
                pos.append(p)
                neg.append(n)
                mask.append(m)
            yield (users, pos, neg, mask)
