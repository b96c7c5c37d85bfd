"""numpy restatement of the rank calls (include/pda_hip_rank.h), independent of any kernel: from a matrix of head values (the dense kernel's
float32 scores, or float64 products), the history rows and the target rows, the 0-based position of every target entry in its row's masked
ranking by (value descending, global id ascending), -1 for an entry that does not rank, and the length of every ranking."""
import numpy as np


def rank_ref(values, hist_rows, tgt_rows, item_offset=0):
    """values [n_rows, n_items_local] (column c = global item item_offset + c); hist_rows / tgt_rows: per row, global item ids (any order,
    duplicates allowed, ids outside the shard allowed) -> (rank int64 [n_entries], n_ranked int64 [n_rows])."""
    values = np.asarray(values)
    n_rows, nloc = values.shape
    ranks, n_ranked = [], np.zeros(n_rows, dtype=np.int64)
    ids = np.arange(nloc, dtype=np.int64)
    for r in range(n_rows):
        v = values[r].astype(np.float64)
        ok = v > -np.inf                                   # (NaN: false)
        h = np.asarray(hist_rows[r], dtype=np.int64) - item_offset if hist_rows is not None else np.zeros(0, np.int64)
        h = h[(h >= 0) & (h < nloc)]
        ok[h] = False
        n_ranked[r] = int(ok.sum())
        vr, ir = v[ok], ids[ok]
        for t in np.asarray(tgt_rows[r], dtype=np.int64):
            c = t - item_offset
            if c < 0 or c >= nloc or not ok[c]:
                ranks.append(-1)
            else:
                ranks.append(int(((vr > v[c]) | ((vr == v[c]) & (ir < c))).sum()))
    return np.asarray(ranks, dtype=np.int64), n_ranked


def lists_from(values, hist_rows, K, item_offset=0):
    """The lists the same order implies: int64 [n_rows, K] global ids of the K best ranking items of every row (rows must hold K of them)."""
    values = np.asarray(values)
    n_rows, nloc = values.shape
    out = np.zeros((n_rows, K), dtype=np.int64)
    ids = np.arange(nloc, dtype=np.int64)
    for r in range(n_rows):
        v = values[r].astype(np.float64)
        ok = v > -np.inf
        if hist_rows is not None:
            h = np.asarray(hist_rows[r], dtype=np.int64) - item_offset
            ok[h[(h >= 0) & (h < nloc)]] = False
        assert ok.sum() >= K
        order = np.lexsort((ids, -np.where(ok, v, -np.inf)))[:K]
        out[r] = order + item_offset
    return out


def csr_of(rows):
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(x) for x in rows])
    flat = np.concatenate([np.asarray(x, dtype=np.int32) for x in rows]).astype(np.int32) if len(rows) and indptr[-1] else np.zeros(0, np.int32)
    return indptr, flat
