"""The rank report (`--rank_report 1`): where the held-out items stand in the masked full-catalogue rankings, below the lists too.

    RankStats    the statistics of one evaluation pass from the exact 0-based position of every target entry (ops.rank_targets,
                 include/pda_hip_rank.h) and the length of every user's ranking -- plain numpy, float64 on integer ranks
    RankReport   the flags' side: the cut-offs and the popularity groups of a dataset, the `||--- rank` lines of a pass

Per user: P = the DISTINCT ranked targets (a duplicated entry counts once; rank -1 = does not rank: listed in the history, outside the
catalogue, head value not > -inf), their ranks sorted r_(0) < r_(1) < ..., n = the ranking's length.

    AUC          mean over the users with |P| >= 1 and n > |P| of 1 - sum_k (r_(k) - k) / (|P| (n - |P|)): the share of (ranked target, other
                 ranked item) pairs the target wins.  The users left out are counted.
    MRR          mean over ALL users of 1 / (1 + r_(0)), 0 for a user without a ranked target
    MPR          mean over the ranked targets of r / max(n - 1, 1): the expected percentile rank of Hu et al. on the masked ranking
    recall@K     per user (ranked targets with r < K) / (target entries of the row), hit@K whether there is one; both summed over the users
                 with targets and divided by ALL users -- the metrics line's denominators; an unranked target is a miss.  Any positive K.
    per group    of the TARGET item (exposure.item_groups): target entries, MPR and median rank of the ranked targets, recall@K = ranked
                 targets with r < K / target entries of the group (exposure.ExposureReport.group_recall at the same K)

The contract and the measurement are in DESIGN.md, "5q. Ranks of held-out items".
"""
from __future__ import annotations

import ast
from typing import Optional

import numpy as np

from .exposure import GROUP_BY, MAX_GROUPS, item_groups


def rank_ks(text) -> list:
    """--rank_ks, a list literal like --Ks -> the cut-offs ascending, each once; any positive integer."""
    try:
        raw = list(ast.literal_eval(text) if isinstance(text, str) else text)
        ok = bool(raw) and all(isinstance(k, (int, np.integer)) and not isinstance(k, bool) and k >= 1 for k in raw)
    except (ValueError, SyntaxError, TypeError):
        ok = False
    if not ok:
        raise ValueError("--rank_ks is a list of positive integers like [50, 1000], got %r" % (text,))
    return sorted({int(k) for k in raw})


def check_rank_report(args, topk_shard=None) -> bool:
    """The rank flags, checked before anything is built -> whether the report is on."""
    on = int(getattr(args, "rank_report", 0) or 0)
    if on not in (0, 1):
        raise ValueError("--rank_report is 0 or 1, got %r" % (args.rank_report,))
    if not on:
        return False
    if topk_shard is not None:
        raise NotImplementedError("--rank_report 1: item shards are not wired up (the counts of the shards add, include/pda_hip_rank.h, but the "
                                  "report ranks on one GPU)")
    if getattr(args, "train", "normal") == "temp_pop" or getattr(args, "test", "normal") == "temp_pop":
        raise NotImplementedError("--rank_report 1: the temp_pop head (s + alpha beta) has no rank kernel; ranks are taken by the raw and the "
                                  "popularity head")
    if getattr(args, "train", "normal") == "macr" or getattr(args, "test", "normal") == "macr":
        raise NotImplementedError("--rank_report 1: --train macr ranks by its counterfactual head, which has no rank kernel")
    rank_ks(args.rank_ks)
    if not 1 <= int(args.bias_groups) <= MAX_GROUPS:
        raise ValueError("--bias_groups must lie in 1 .. %d, got %r" % (MAX_GROUPS, args.bias_groups))
    if args.bias_group_by not in GROUP_BY:
        raise ValueError("--bias_group_by is interactions or items, not %r" % (args.bias_group_by,))
    return True


def refuse_rank_report(args, who: str):
    """The tools that re-rank or only write lists do not take the flag: a re-ranked list has no full-catalogue order."""
    if int(getattr(args, "rank_report", 0) or 0):
        raise NotImplementedError("--rank_report 1: %s does not take the flag (a re-ranked or exported list has no full-catalogue order); "
                                  "python -m pda_amd.train_new_api prints the rank lines" % who)


class RankStats:
    """The statistics of one pass.  rank int [n_entries] (-1: unranked), n_ranked int [n_users], the targets' CSR (indptr [n_users + 1], ids
    [n_entries]), Ks; groups int [n_items] with n_groups groups or None (no per-group statistics)."""

    def __init__(self, rank, n_ranked, tgt_indptr, tgt_indices, Ks, groups=None, n_groups: Optional[int] = None):
        rank = np.asarray(rank, dtype=np.int64).reshape(-1)
        n = np.asarray(n_ranked, dtype=np.int64).reshape(-1)
        tp = np.asarray(tgt_indptr, dtype=np.int64).reshape(-1)
        ids = np.asarray(tgt_indices, dtype=np.int64).reshape(-1)
        nu = n.shape[0]
        if tp.shape[0] != nu + 1 or rank.shape[0] != ids.shape[0] or (nu and tp[-1] - tp[0] != ids.shape[0]):
            raise ValueError("rank holds one position per target entry, n_ranked one length per row of the targets' CSR")
        self.Ks = [int(k) for k in Ks]
        lens = np.diff(tp)
        row = np.repeat(np.arange(nu, dtype=np.int64), lens)
        ranked = rank >= 0
        # a duplicated entry counts once: the first of every (row, item) pair
        first = np.zeros(ids.shape[0], dtype=bool)
        if ids.shape[0]:
            first[np.unique(np.stack([row, ids]), axis=1, return_index=True)[1]] = True
        keep = ranked & first
        self.n_users, self.n_entries = int(nu), int(ids.shape[0])
        self.n_ranked_targets = int(keep.sum())
        self.n_unranked_targets = int((first & ~ranked).sum())
        r, u = rank[keep].astype(np.float64), row[keep]
        P = np.bincount(u, minlength=nu)[:nu].astype(np.float64)
        rsum = np.bincount(u, weights=r, minlength=nu)[:nu]
        nf = n.astype(np.float64)
        # ---- AUC ----
        use = (P >= 1) & (nf > P)
        self.auc_users, self.auc_left_out = int(use.sum()), int(nu - use.sum())
        auc_u = 1.0 - (rsum[use] - P[use] * (P[use] - 1.0) / 2.0) / (P[use] * (nf[use] - P[use]))
        self.auc = float(auc_u.mean()) if auc_u.size else 0.0
        # ---- MRR ----
        rmin = np.full(nu, np.inf)
        np.minimum.at(rmin, u, r)
        self.mrr = float((1.0 / (1.0 + rmin)).sum() / nu) if nu else 0.0        # (1 / inf = 0: no ranked target)
        # ---- percentile, mean, median ----
        pct = r / np.maximum(nf[u] - 1.0, 1.0)
        self.mpr = float(pct.mean()) if r.size else 0.0
        self.mean_rank = float(r.mean()) if r.size else 0.0
        self.median_rank = float(np.median(r)) if r.size else 0.0
        # ---- recall@K, hit@K: the metrics line's denominators ----
        nk = len(self.Ks)
        self.recall, self.hit = np.zeros(nk), np.zeros(nk)
        has = lens > 0
        for q, K in enumerate(self.Ks):
            hits = np.bincount(u[r < K], minlength=nu)[:nu].astype(np.float64)
            if nu:
                self.recall[q] = float((hits[has] / lens[has]).sum() / nu)
                self.hit[q] = float((hits[has] > 0).sum() / nu)
        # ---- per popularity group of the target item ----
        self.has_groups = groups is not None
        if self.has_groups:
            groups = np.asarray(groups, dtype=np.int64).reshape(-1)
            G = int(groups.max()) + 1 if n_groups is None else int(n_groups)
            inside = (ids >= 0) & (ids < groups.shape[0])
            g_all = groups[ids[inside]]
            self.n_groups = G
            self.group_targets = np.bincount(g_all, minlength=G)[:G].astype(np.int64)          # entries, as ExposureReport counts targets
            g = groups[ids[keep]]
            cnt = np.bincount(g, minlength=G)[:G].astype(np.float64)
            self.group_mpr = np.divide(np.bincount(g, weights=pct, minlength=G)[:G], cnt, out=np.zeros(G), where=cnt > 0)
            self.group_median = np.array([float(np.median(r[g == k])) if (g == k).any() else 0.0 for k in range(G)])
            self.group_recall = np.zeros((nk, G))
            tg = self.group_targets.astype(np.float64)
            for q, K in enumerate(self.Ks):
                h = np.bincount(g[r < K], minlength=G)[:G].astype(np.float64)
                self.group_recall[q] = np.divide(h, tg, out=np.zeros(G), where=tg > 0)

    def lines(self):
        """The `||--- rank` lines of the pass."""
        def vec(v, fmt="%.4f"):
            return "[" + ",".join(fmt % x for x in v) + "]"
        out = ["||--- rank auc=%.6f (users=%d, left_out=%d) mrr=%.6f mpr=%.6f mean_rank=%.2f median_rank=%.1f ranked=%d unranked=%d"
               % (self.auc, self.auc_users, self.auc_left_out, self.mrr, self.mpr, self.mean_rank, self.median_rank, self.n_ranked_targets,
                  self.n_unranked_targets)]
        for q, K in enumerate(self.Ks):
            out.append("||--- rank@%d recall=%.5f hit=%.5f" % (K, self.recall[q], self.hit[q]))
        if self.has_groups:
            out.append("||--- rank groups targets=%s mpr=%s median_rank=%s" % (vec(self.group_targets, "%d"), vec(self.group_mpr),
                                                                             vec(self.group_median, "%.1f")))
            for q, K in enumerate(self.Ks):
                out.append("||--- rank@%d group_recall=%s" % (K, vec(self.group_recall[q])))
        return out


class RankReport:
    """What `--rank_report 1` adds to an evaluation object (evaluation.set_rank_report): the cut-offs and the target items' groups."""

    def __init__(self, train_counts, Ks, n_groups=10, group_by="interactions"):
        self.Ks = rank_ks(Ks)
        self.n_groups = int(n_groups)
        self.groups = item_groups(np.asarray(train_counts, dtype=np.int64).reshape(-1), n_groups, group_by)

    @staticmethod
    def from_args(args, data_, topk_shard=None) -> Optional["RankReport"]:
        """None with --rank_report 0."""
        if not check_rank_report(args, topk_shard):
            return None
        from .xquad import train_counts
        return RankReport(train_counts(data_), args.rank_ks, args.bias_groups, args.bias_group_by)

    def stats(self, rank, n_ranked, tgt_indptr, tgt_indices) -> RankStats:
        return RankStats(rank, n_ranked, tgt_indptr, tgt_indices, self.Ks, self.groups, self.n_groups)
