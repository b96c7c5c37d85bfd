"""The bias report (`--bias_report 1`): what a method's lists do to popularity bias, from the per-item histogram of the lists.

    item_groups          items grouped by train popularity (equal items or equal train interactions per group)
    ExposureReport       the statistics of one evaluation pass, per cut-off K: recommendation rate, hit share and recall per group, ARP, coverage,
                         Gini, APLT -- plain numpy, float64 on integer counts
    ExposureAccumulator  the two device buffers pda_list_exposure (include/pda_hip_exposure.h) adds every block's lists to
    BiasReport           the flags' side: groups and head of a dataset, the accumulator of an evaluation object, the `||--- bias@K` lines

The histogram is the only part that touches the lists; it runs on the device next to pda_metrics.  The contract and the measurement are in
DESIGN.md, "5k. Bias report".
"""
from __future__ import annotations

from typing import Optional

import numpy as np

MAX_GROUPS = 64
GROUP_BY = ("interactions", "items")


def popularity_order(train_counts) -> np.ndarray:
    """The items by (train count descending, id ascending): the order of xquad.head_items."""
    counts = np.asarray(train_counts, dtype=np.int64).reshape(-1)
    return np.lexsort((np.arange(counts.shape[0]), -counts))


def item_groups(train_counts, G, by="interactions") -> np.ndarray:
    """int64 [n_items]: the popularity group of each item, 0 = the most popular, 1 <= G <= 64.  The items are taken in popularity_order:
    by="items": position p is in group (p G) // n_items (equal item counts, up to rounding);
    by="interactions": group min(G - 1, (cum_before G) // total), cum_before the train count of the items in front -- groups of equal train
    interactions, which differ in size and may be empty.  Integer arithmetic throughout."""
    counts = np.asarray(train_counts, dtype=np.int64).reshape(-1)
    if int(G) != G or not 1 <= int(G) <= MAX_GROUPS:
        raise ValueError("the number of groups must lie in 1 .. %d, got %r" % (MAX_GROUPS, G))
    G = int(G)
    if by not in GROUP_BY:
        raise ValueError("items are grouped by 'interactions' or 'items', not %r" % (by,))
    n = counts.shape[0]
    if n < 1:
        raise ValueError("an empty catalogue has no groups")
    if (counts < 0).any():
        raise ValueError("train counts must be >= 0")
    order = popularity_order(counts)
    groups = np.empty(n, dtype=np.int64)
    if by == "items":
        groups[order] = (np.arange(n, dtype=np.int64) * G) // n
        return groups
    total = int(counts.sum())
    if total == 0:
        raise ValueError("a train set without interactions cannot be cut into groups of equal interactions")
    sorted_counts = counts[order]
    cum_before = np.cumsum(sorted_counts) - sorted_counts
    groups[order] = np.minimum(G - 1, (cum_before * G) // total)
    return groups


def gini(x) -> float:
    """Gini coefficient of non-negative counts: sum_r (2r - n - 1) x_(r) / (n sum x) on the ascending sort, r = 1 .. n; 0 for all-zero counts."""
    v = np.sort(np.asarray(x, dtype=np.float64).reshape(-1))
    n, s = v.shape[0], float(v.sum())
    if n == 0 or s == 0.0:
        return 0.0
    r = np.arange(1, n + 1, dtype=np.float64)
    return float(((2.0 * r - n - 1.0) * v).sum() / (n * s))


def cumulate(buckets) -> np.ndarray:
    """int64 [n_ks, n_items]: the counts at the cut-off Ks[b] = the sum of pda_list_exposure's buckets <= b."""
    return np.cumsum(np.asarray(buckets, dtype=np.int64), axis=0)


def _per_group(x, groups, G):
    return np.bincount(groups, weights=np.asarray(x, dtype=np.float64), minlength=G)[:G]


def _share(x):
    s = float(x.sum())
    return x / s if s > 0.0 else np.zeros_like(x)


def _group_line(group_items, train_share) -> str:
    return "||--- bias groups items=[%s] train_share=[%s]" % (",".join(str(int(x)) for x in group_items), ",".join("%.4f" % x for x in train_share))


class ExposureReport:
    """The statistics of one pass.  shown / hit: the CUMULATED counts int [n_ks, n_items] (hit None: lists without targets, no hit statistics);
    rows: the lists counted; Ks; train_counts [n_items]; groups int [n_items] (item_groups) with n_groups groups; is_head [n_items], non-zero =
    short head (xquad.head_items); tgt_counts [n_items]: how often each item is a target of the evaluated users (np.bincount of tgt_indices).

    Per cut-off (arrays with a leading axis over Ks):
        rr[g]            shown in group g / shown in total (0 when nothing was shown)
        hit_share[g]     hits in group g / hits in total
        group_recall[g]  hits in group g / targets in group g (0 for a group without targets)
        arp              sum shown_i count_i / sum shown_i: the average train popularity of a shown item
        coverage         items shown at least once / n_items
        gini             of shown over all items
        aplt             (tail_shown / K) / rows: the expression of xquad.ListTap.aplt
    Once: train_share[g] (the groups' share of the train interactions), group_items[g]."""

    def __init__(self, shown, hit, rows, Ks, train_counts, groups, is_head, tgt_counts=None, n_groups: Optional[int] = None):
        shown = np.asarray(shown, dtype=np.int64)
        counts = np.asarray(train_counts, dtype=np.int64).reshape(-1)
        groups = np.asarray(groups, dtype=np.int64).reshape(-1)
        head = np.asarray(is_head).reshape(-1) != 0
        self.Ks = [int(k) for k in Ks]
        n = counts.shape[0]
        if shown.ndim != 2 or shown.shape != (len(self.Ks), n) or groups.shape[0] != n or head.shape[0] != n:
            raise ValueError("shown is [len(Ks), n_items]; train_counts, groups and is_head hold one entry per item")
        G = int(groups.max()) + 1 if n_groups is None else int(n_groups)
        if groups.min() < 0 or groups.max() >= G:
            raise ValueError("group ids must lie in [0, %d)" % G)
        self.rows, self.n_groups = int(rows), G
        self.group_items = np.bincount(groups, minlength=G)[:G].astype(np.int64)
        self.train_share = _share(_per_group(counts, groups, G))
        nk = len(self.Ks)
        self.rr = np.zeros((nk, G))
        self.arp, self.coverage, self.gini, self.aplt = np.zeros(nk), np.zeros(nk), np.zeros(nk), np.zeros(nk)
        for q, K in enumerate(self.Ks):
            x = shown[q].astype(np.float64)
            tot = float(x.sum())
            self.rr[q] = _share(_per_group(x, groups, G))
            self.arp[q] = float((x * counts.astype(np.float64)).sum()) / tot if tot > 0.0 else 0.0
            self.coverage[q] = float(np.count_nonzero(shown[q])) / float(n)
            self.gini[q] = gini(shown[q])
            self.aplt[q] = (float(shown[q][~head].sum()) / float(K)) / float(max(self.rows, 1))
        self.has_hits = hit is not None
        if self.has_hits:
            hit = np.asarray(hit, dtype=np.int64)
            if hit.shape != shown.shape or tgt_counts is None:
                raise ValueError("hit is shaped like shown and comes with the target counts")
            tgt = np.asarray(tgt_counts, dtype=np.float64).reshape(-1)
            if tgt.shape[0] != n:
                raise ValueError("tgt_counts holds one entry per item")
            tgt_g = _per_group(tgt, groups, G)
            self.hit_share, self.group_recall = np.zeros((nk, G)), np.zeros((nk, G))
            for q in range(nk):
                h = _per_group(hit[q], groups, G)
                self.hit_share[q] = _share(h)
                self.group_recall[q] = np.divide(h, tgt_g, out=np.zeros(G), where=tgt_g > 0)

    def lines(self):
        """One `||--- bias@K` line per cut-off."""
        def vec(v):
            return "[" + ",".join("%.4f" % x for x in v) + "]"
        out = []
        for q, K in enumerate(self.Ks):
            s = "||--- bias@%d arp=%.2f cov=%.5f gini=%.5f aplt=%.5f rr=%s" % (K, self.arp[q], self.coverage[q], self.gini[q], self.aplt[q],
                                                                             vec(self.rr[q]))
            if self.has_hits:
                s += " hit_share=%s group_recall=%s" % (vec(self.hit_share[q]), vec(self.group_recall[q]))
            out.append(s)
        return out

    def group_line(self):
        return _group_line(self.group_items, self.train_share)


class ExposureAccumulator:
    """The device buffers of one evaluation pass: shown and (with_hits) hit, int32 [len(Ks), n_items] of column buckets, and the rows added."""

    def __init__(self, n_items, Ks, device, with_hits: bool = True):
        import torch
        from . import ops
        self.Ks = list(ops.exposure_ks(Ks))
        self.n_items = int(n_items)
        self.device = torch.device(device)
        self.shown = torch.zeros((len(self.Ks), self.n_items), dtype=torch.int32, device=self.device)
        self.hit = torch.zeros_like(self.shown) if with_hits else None
        self.rows = 0

    def reset(self):
        self.shown.zero_()
        if self.hit is not None:
            self.hit.zero_()
        self.rows = 0

    def add(self, idx, tgt_indptr=None, tgt_indices=None):
        """One block of lists idx int32 [n, k] with the CSR of its rows' targets (needed exactly when the accumulator counts hits)."""
        from . import ops
        if (self.hit is not None) != (tgt_indptr is not None):
            raise ValueError("an accumulator with hit counts takes every block with its targets, one without takes none")
        ops.list_exposure(idx, self.Ks, self.n_items, tgt_indptr, tgt_indices, self.shown, self.hit)
        self.rows += int(idx.shape[0])

    def counts(self):
        """-> (shown, hit | None): the cumulated counts at every cut-off, int64 [len(Ks), n_items] on the host."""
        return cumulate(self.shown.cpu().numpy()), None if self.hit is None else cumulate(self.hit.cpu().numpy())

    def report(self, train_counts, groups, is_head, tgt_counts=None, n_groups=None) -> ExposureReport:
        shown, hit = self.counts()
        return ExposureReport(shown, hit, self.rows, self.Ks, train_counts, groups, is_head, tgt_counts, n_groups)


class EvalResult(dict):
    """The four metric arrays of evaluation.eval, with the bias lines of the same pass (and the BiasReport they come from) and the pass's rank
    lines (--rank_report 1, pda_amd/rank_report.py) beside them, not among the keys."""
    bias_lines = ()
    bias = None
    rank_lines = ()


def report_ks(Ks, topk_max) -> list:
    """The report's cut-offs: the Ks that are <= --topk_max, ascending, each once."""
    ks = sorted({int(k) for k in Ks if 1 <= int(k) <= int(topk_max)})
    if not ks:
        raise ValueError("--bias_report: no cut-off of --Ks %r lies in 1 .. --topk_max %d" % (list(Ks), int(topk_max)))
    return ks


def check_flags(args, topk_shard=None):
    """The bias flags, checked before anything is built -> whether the report is on."""
    on = int(getattr(args, "bias_report", 0) or 0)
    if on not in (0, 1):
        raise ValueError("--bias_report is 0 or 1, got %r" % (args.bias_report,))
    if not on:
        return False
    if topk_shard is not None:
        raise NotImplementedError("--bias_report 1: the report counts the lists of one GPU (an item-sharded evaluation is out of its scope)")
    if not 1 <= int(args.bias_groups) <= MAX_GROUPS:
        raise ValueError("--bias_groups must lie in 1 .. %d, got %r" % (MAX_GROUPS, args.bias_groups))
    if args.bias_group_by not in GROUP_BY:
        raise ValueError("--bias_group_by is interactions or items, not %r" % (args.bias_group_by,))
    if not 0.0 < float(args.xq_head_share) < 1.0:
        raise ValueError("--xq_head_share must lie strictly inside 0 .. 1, got %r" % (args.xq_head_share,))
    return True


class BiasReport:
    """What `--bias_report 1` adds to an evaluation object (evaluation.set_bias_report): the dataset's groups and head, one accumulator per
    evaluation device, and the lines of a pass."""

    def __init__(self, train_counts, Ks, n_groups=10, group_by="interactions", head_share=0.8):
        from .xquad import head_items
        self.train_counts = np.asarray(train_counts, dtype=np.int64).reshape(-1)
        self.n_items = self.train_counts.shape[0]
        self.Ks = list(Ks)
        self.n_groups = int(n_groups)
        self.groups = item_groups(self.train_counts, n_groups, group_by)
        self.is_head = head_items(self.train_counts, head_share)
        self._acc = {}
        self._group_line = _group_line(np.bincount(self.groups, minlength=self.n_groups)[:self.n_groups],
                                       _share(_per_group(self.train_counts, self.groups, self.n_groups)))
        self._groups_printed = False

    @staticmethod
    def from_args(args, data_, Ks, topk_shard=None) -> Optional["BiasReport"]:
        """None with --bias_report 0."""
        if not check_flags(args, topk_shard):
            return None
        from .xquad import train_counts
        topk_max = getattr(args, "topk_max", None)
        return BiasReport(train_counts(data_), report_ks(Ks, 50 if topk_max is None else topk_max), args.bias_groups, args.bias_group_by,
                          args.xq_head_share)

    def accumulator(self, device, with_hits=True) -> ExposureAccumulator:
        """The (zeroed) accumulator of this device."""
        key = (str(device), bool(with_hits))
        acc = self._acc.get(key)
        if acc is None:
            acc = self._acc[key] = ExposureAccumulator(self.n_items, self.Ks, device, with_hits)
        acc.reset()
        return acc

    def report(self, acc: ExposureAccumulator, tgt_indices=None) -> ExposureReport:
        """tgt_indices: the flat targets of the evaluated users (host), for an accumulator with hit counts."""
        tgt = None if acc.hit is None else np.bincount(np.asarray(tgt_indices, dtype=np.int64).reshape(-1), minlength=self.n_items)[:self.n_items]
        return acc.report(self.train_counts, self.groups, self.is_head, tgt, self.n_groups)

    def header(self) -> list:
        """The line that names the groups, the first time it is asked for; nothing afterwards (a run prints it once)."""
        out = [] if self._groups_printed else [self._group_line]
        self._groups_printed = True
        return out
