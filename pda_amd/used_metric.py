"""Ranking metrics with the reference's names (MF/used_metric.py).

`evaluate_on_device` is the product path: pda_metrics (HIP) over the whole top-K matrix, replacing the
reference's multiprocessing.Pool(5) that pickles every block (MF/train_new_api.py:741-778).
`get_performance` keeps the reference's per-user host signature for callers that still hold python lists
(MF/used_metric.py:69-80); it is host glue, not a fallback for the kernel.
"""
from __future__ import annotations

import numpy as np


def get_r(user_pos_test, r):
    return np.isin(np.asarray(r), np.asarray(list(user_pos_test))).astype(np.float64)


def check_ks(Ks):
    """The cut-offs as a list of ints, checked while they are still on the host: the kernels divide by min(K, columns), so a K < 1 there is
    a division by zero."""
    ks = [int(k) for k in Ks]
    if not ks or any(k != k0 for k, k0 in zip(ks, Ks)) or min(ks) < 1:
        raise ValueError("Ks must be a non-empty list of integers >= 1, got %r" % (list(Ks),))
    return ks


def get_performance(user_pos_test, r, Ks):
    """Two cases the reference leaves open follow the kernels: a K beyond len(r) is cut to len(r) (in the ideal DCG too), and a user
    without targets gets zeros (the reference: recall 0/0)."""
    hit = get_r(user_pos_test, r)
    n_pos = len(user_pos_test)
    out = {"recall": [], "precision": [], "ndcg": [], "hit_ratio": []}
    for K in check_ks(Ks):
        h = hit[:K]
        disc = 1.0 / np.log2(np.arange(2, h.size + 2))
        ideal = disc[:n_pos].sum()
        out["precision"].append(np.mean(h) if n_pos else 0.0)
        out["recall"].append(np.sum(h) / n_pos if n_pos else 0.0)
        out["ndcg"].append(0.0 if not ideal else float((h * disc).sum() / ideal))
        out["hit_ratio"].append(min(1.0, np.sum(h)))
    return {k: np.array(v) for k, v in out.items()}


def evaluate_on_device(topk, tgt_indptr, tgt_indices, Ks, tot_user=None):
    """topk i32 [n,k] (cuda), targets CSR by row (cuda) -> dict of float64 numpy arrays [len(Ks)] = sums / tot_user."""
    import torch
    from . import ops
    ks = torch.as_tensor(check_ks(Ks), dtype=torch.int32, device=topk.device)
    sums = ops.metrics_sums(topk, tgt_indptr, tgt_indices, ks).cpu().numpy()
    n = float(tot_user if tot_user is not None else topk.shape[0])
    return {"precision": sums[0] / n, "recall": sums[1] / n, "ndcg": sums[2] / n, "hit_ratio": sums[3] / n}
