"""Numpy restatement of BPR-PC (MF/BPR_PC.py:684-713, driven by its evaluation class) for the BPR-PC tests.

    constants          a, b, w, e of the contract ("5b. BPR-PC")
    stats_direct       A_u, Bc_u, n_u as direct float64 sums over the catalogue (s = u . v and C = (b s + w) p real-valued)
    stats_moments      the same from the item moments G, H, h, P and the history alone (what the library computes)
    finish_stats       U_n, U_c, k_u from A_u, Bc_u, n_u (fp32 roundings of the contract; k_u = 0 where n_u = 0 or U_c = 0)
    pc_lists           the contract's lists from the fp32 scores s and a given k_u: r, one m per block, g, the masked values, top-K
    transcription      a line-by-line numpy transcription of creat_recommendation (dense clicked matrix by scatter-add, reduce_min over
                       the whole block, fp32 elementwise ops), one reference block at a time
"""
import numpy as np

f32 = np.float32


def constants(alpha, beta):
    return f32(alpha), f32(beta), f32(1.0 - float(beta)), f32(0.01)


def counts_matrix(hist_rows, n_items):
    """int64 [B, n_items]: how many times each item is listed in each row."""
    c = np.zeros((len(hist_rows), n_items), dtype=np.int64)
    for r, items in enumerate(hist_rows):
        np.add.at(c[r], np.asarray(items, dtype=np.int64), 1)
    return c


def item_p(pop):
    return (f32(1.0) / np.asarray(pop, dtype=f32)).astype(f32)


def moments(I, pop):
    """float64 G, H, h, P of the item table."""
    V = np.asarray(I, dtype=np.float64)
    p2 = item_p(pop).astype(np.float64) ** 2
    return V.T @ V, (V * p2[:, None]).T @ V, (V * p2[:, None]).sum(0), p2.sum()


def stats_direct(U, I, users, hist_rows, pop, beta):
    """-> (A, Bc, n_u) float64 / int64 [B], straight from the definitions."""
    _, b, w, _ = constants(0.0, beta)
    S = np.asarray(U, dtype=np.float64)[np.asarray(users)] @ np.asarray(I, dtype=np.float64).T
    C = (float(b) * S + float(w)) * item_p(pop).astype(np.float64)[None, :]
    c = counts_matrix(hist_rows, I.shape[0])
    f = (1.0 - c) ** 2
    return (f * S * S).sum(1), (f * C * C).sum(1), I.shape[0] - c.sum(1)


def stats_moments(U, I, users, hist_rows, pop, beta, mom=None):
    """-> (A, Bc, n_u) from the moments and each row's history alone."""
    _, b, w, _ = constants(0.0, beta)
    b, w = float(b), float(w)
    G, H, h, P = moments(I, pop) if mom is None else mom
    Uu = np.asarray(U, dtype=np.float64)[np.asarray(users)]
    V = np.asarray(I, dtype=np.float64)
    p = item_p(pop).astype(np.float64)
    A = np.einsum("bi,ij,bj->b", Uu, G, Uu)
    Bc = b * b * np.einsum("bi,ij,bj->b", Uu, H, Uu) + 2 * b * w * (Uu @ h) + w * w * P
    n = np.full(len(users), I.shape[0], dtype=np.int64)
    for r, items in enumerate(hist_rows):
        it, c = np.unique(np.asarray(items, dtype=np.int64), return_counts=True)
        s = V[it] @ Uu[r]
        C = (b * s + w) * p[it]
        f = (1.0 - c) ** 2 - 1.0
        A[r] += (f * s * s).sum()
        Bc[r] += (f * C * C).sum()
        n[r] -= c.sum()
    return A, Bc, n


def finish_stats(A, Bc, n):
    """-> (U_n, U_c, k) float32 [B]; U_n = RN32(|inv_u| sqrt(A_u)), U_c alike."""
    Un = np.zeros(len(A), f32)
    Uc = np.zeros(len(A), f32)
    k = np.zeros(len(A), f32)
    for r in range(len(A)):
        if n[r] == 0:
            continue
        inv = abs(f32(1.0) / f32(n[r]))          # (duplicates can make n_u negative: a norm of x / n_u scales by |1 / n_u|)
        Un[r] = f32(float(inv) * np.sqrt(max(A[r], 0.0)))
        Uc[r] = f32(float(inv) * np.sqrt(max(Bc[r], 0.0)))
        if Uc[r] > 0 and np.isfinite(Uc[r]):
            k[r] = Un[r] * (f32(1.0) / Uc[r])
    return Un, Uc, k


def ratings(s, pop, k, alpha, beta):
    """r = RN32(s + RN32(a RN32(C k))), C = RN32(RN32(RN32(s b) + w) p), float32 [B, N]."""
    a, b, w, _ = constants(alpha, beta)
    s = np.asarray(s, dtype=f32)
    C = ((s * b + w) * item_p(pop)[None, :]).astype(f32)
    return (s + a * (C * np.asarray(k, dtype=f32)[:, None])).astype(f32)


def masked_values(g, counts):
    """g after c subtractions of g, in turn (what SparseTensorDenseAdd does with c entries of -g)."""
    v = g.copy()
    for t in range(int(counts.max(initial=0))):
        sel = counts > t
        v[sel] = (v[sel] - g[sel]).astype(f32)
    return v


def rank_rows(v, K):
    """The first K of each row by (v descending, index ascending) -- tf.nn.top_k."""
    idx = np.empty((v.shape[0], K), dtype=np.int32)
    for r in range(v.shape[0]):
        o = np.lexsort((np.arange(v.shape[1]), -v[r].astype(np.float64)))
        idx[r] = o[:K]
    return idx, np.take_along_axis(v, idx.astype(np.int64), 1)


def pc_lists(s, hist_rows, pop, k, alpha, beta, K, block=2048, return_r=False):
    """The contract's lists for fp32 scores s [B, N] and per-row k, one m per `block` consecutive rows -> (idx int32, val float32)."""
    _, _, _, e = constants(alpha, beta)
    r = ratings(s, pop, k, alpha, beta)
    c = counts_matrix(hist_rows, s.shape[1])
    g = np.empty_like(r)
    for b0 in range(0, r.shape[0], block):
        m = r[b0:b0 + block].min()
        g[b0:b0 + block] = ((r[b0:b0 + block] - m).astype(f32) + e).astype(f32)
    v = masked_values(g, c)
    idx, val = rank_rows(v, K)
    return (idx, val, r) if return_r else (idx, val)


def transcription(s, hist_rows, pop, alpha, beta, K, k=None):
    """MF/BPR_PC.py:684-713 line by line for ONE reference block (fp32 elementwise, float64 norms).  k: feed this scale instead of the
    transcription's own (to compare lists with a library-side k).  -> (U_n, U_c, k, idx, val)."""
    s = np.asarray(s, dtype=f32)
    B, N = s.shape
    a, b, w, e = constants(alpha, beta)
    rows = np.concatenate([np.full(len(h), r) for r, h in enumerate(hist_rows)]).astype(np.int64) if B else np.zeros(0, np.int64)
    cols = np.concatenate([np.asarray(h, dtype=np.int64) for h in hist_rows]) if B else np.zeros(0, np.int64)
    clicked = np.zeros((B, N), f32)
    np.add.at(clicked, (rows, cols), f32(1.0))                                   # sparse_cliked_matrix, values 1.0
    clicked_num = clicked.sum(-1, dtype=f32)                                     # tf.sparse.reduce_sum
    non_clicked_num = (-clicked_num + f32(N)).astype(f32)
    pop_ = (f32(1.0) / np.asarray(pop, dtype=f32)).reshape(1, -1)                # tf.reciprocal(self.pop)
    inv = (f32(1.0) / non_clicked_num).reshape(-1, 1)
    U_n = s.copy()
    np.add.at(U_n, (rows, cols), -s[rows, cols])                                 # tf.sparse.add(scores, clicked * -scores)
    U_n = (U_n * inv).astype(f32)
    U_n = f32(np.sqrt((U_n.astype(np.float64) ** 2).sum(-1)))                   # tf.norm (float64 here)
    C_u = ((s * b).astype(f32) + w).astype(f32)
    C_u = (C_u * pop_).astype(f32)
    U_c = C_u.copy()
    np.add.at(U_c, (rows, cols), -C_u[rows, cols])
    U_c = (U_c * inv).astype(f32)
    U_c = f32(np.sqrt((U_c.astype(np.float64) ** 2).sum(-1)))
    scale = (U_n * (f32(1.0) / U_c)).astype(f32)
    if k is not None:
        scale = np.asarray(k, dtype=f32)
    rating = (s + (a * (C_u * scale.reshape(-1, 1)).astype(f32)).astype(f32)).astype(f32)
    rating = ((rating - rating.min()).astype(f32) + e).astype(f32)               # quirk 1: tf.reduce_min over the whole block
    np.add.at(rating, (rows, cols), -rating[rows, cols])                         # quirk 2: clicked entries, one -g per entry in turn
    idx, val = rank_rows(rating, K)
    return U_n, U_c, scale, idx, val
