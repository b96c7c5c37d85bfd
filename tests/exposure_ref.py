"""The numpy restatement of the contract of pda_list_exposure (include/pda_hip_exposure.h): a loop over the rows with np.add.at."""
import numpy as np


def exposure_ref(topk, Ks, n_items, tgt_rows=None, shown=None, hit=None):
    """topk int [n, k]; Ks strictly ascending; tgt_rows: one sequence of target ids per row, or None (no hit counts)
    -> (shown, hit | None) int64 [len(Ks), n_items] of column BUCKETS, added to the buffers given."""
    topk = np.asarray(topk, dtype=np.int64)
    n, k = topk.shape
    Ks = [int(x) for x in Ks]
    shown = np.zeros((len(Ks), n_items), np.int64) if shown is None else shown
    if tgt_rows is not None and hit is None:
        hit = np.zeros((len(Ks), n_items), np.int64)
    edges = [0] + [min(x, k) for x in Ks]
    for r in range(n):
        tgt = None if tgt_rows is None else np.asarray(tgt_rows[r], dtype=np.int64).reshape(-1)
        for b in range(len(Ks)):
            ids = topk[r, edges[b]:edges[b + 1]]
            ids = ids[(ids >= 0) & (ids < n_items)]
            np.add.at(shown[b], ids, 1)
            if tgt is not None:
                np.add.at(hit[b], ids[np.isin(ids, tgt)], 1)
    return shown, hit


def csr_of(rows):
    """-> (indptr int64 [n + 1], indices int32) of a list of target rows, kept in the order given."""
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    flat = np.concatenate([np.asarray(r, np.int64).reshape(-1) for r in rows]).astype(np.int32) if len(rows) else np.zeros(0, np.int32)
    return indptr, flat
