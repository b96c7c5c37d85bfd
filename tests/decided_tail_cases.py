"""Data and the CPU restatement of the huge geometry's DECIDED half-tile (pda_amd/csrc/pda_v5_sweep.h), shared by
test_decided_tail_criterion.py (CPU) and test_gpu_huge_decided_tail.py (GPU).  No tests in here.

The criterion (the one that ends generation 4's early-terminating sweeps): behind the first 64-item tile t of the visiting order with

    fmaf(nu, sufB[t], sufA[t]) * 1.000002f < tau

no item can reach the K-th value tau of a user with padded norm nu -- sufA / sufB: the maxima of |pop| and |pop| ||i|| over every
position at or behind the tile.  The kernel takes it once per workgroup on (largest norm, lowest threshold)."""
import numpy as np

from oracle import pda_oracle as po

F = np.float32


def steep_case(rng, nU, nI, d, ratio=0.998, scale=0.1, max_hist=20, hist=True):
    """Popularity falling by `ratio` per item id (strictly: the visiting order -- |pop| descending -- is the identity)."""
    U = (rng.standard_normal((nU, d)) * scale).astype(F)
    I = (rng.standard_normal((nI, d)) * scale).astype(F)
    pop = (ratio ** np.arange(nI, dtype=np.float64)).astype(F)
    assert np.all(np.diff(pop) < 0), "the visiting order must be the identity"
    rows = [np.unique(rng.integers(0, nI, rng.integers(0, max_hist + 1))).astype(np.int32) for _ in range(nU)] if hist else None
    return U, I, pop, rows


def plant(U, I, pop, item, users, strength=5000.0):
    """Item `item` (far down the visiting order: a small popularity) gets a norm so large that its head pop x (1 + u . i) enters the
    top-K of the users aligned with it: `users` get a unit component along the item's direction."""
    d = U.shape[1]
    v = np.zeros(d, F)
    v[item % d] = 1.0
    I[item] = v * F(strength)
    U[users] += v


def csr(rows):
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(h) for h in rows])
    idx = np.concatenate([np.sort(h) for h in rows]).astype(np.int32) if len(rows) else np.zeros(0, np.int32)
    return indptr, idx


def oracle_lists(U, I, pop, users, rows, K):
    """oracle/pda_oracle.py alone: (item ids [B, K], heads [B, K]) of the popularity head with the history masked"""
    ip, ix = csr([rows[u] if rows is not None else np.zeros(0, np.int32) for u in users])
    return po.recommend_topk(U, I, users, ip, ix, K, "condition", pop)


def suffix_bounds(I, pop):
    """sufA, sufB per 64-item tile of the visiting order (|pop| descending, stable): a LOWER, tighter restatement of what tile_bound4_kernel /
    suffix_max4_kernel store, not the kernels' own padding -- the norm here is padded by 1.0000005, the kernel's by 1.0009765625 * 1.0001.  sufA is
    bit-equal to the kernel's, sufB never above it (tests/test_prep_host.py holds both against the fp32 emulation of the prep), and a larger bound
    decides later, never earlier: what is proved on these bounds holds on the device's.  -> (order, sufA, sufB)"""
    order = np.argsort(-np.abs(pop), kind="stable")
    p = np.abs(pop[order]).astype(F)
    nr = np.sqrt((I[order].astype(np.float64) ** 2).sum(1)).astype(F) * F(1.0000005)      # (the kernel's norm is an upper bound of the exact one)
    ok = ~np.isnan(p)
    a = np.where(ok, p, F(0))
    b = np.where(ok, p * nr * F(1.000001), F(0)).astype(F)
    n_tiles = (len(pop) + 63) // 64
    pad = n_tiles * 64 - len(pop)
    a = np.concatenate([a, np.zeros(pad, F)]).reshape(n_tiles, 64).max(1)
    b = np.concatenate([b, np.zeros(pad, F)]).reshape(n_tiles, 64).max(1)
    return order, np.maximum.accumulate(a[::-1])[::-1].astype(F), np.maximum.accumulate(b[::-1])[::-1].astype(F)


def decided_tile(sufA, sufB, nu, tau):
    """first tile t with the criterion true (the bound falls along the order), len(sufA) = never; nu, tau scalars (float32 arithmetic)"""
    if not tau > -np.inf:
        return len(sufA)
    bound = (F(nu) * sufB + sufA).astype(F) * F(1.000002)
    hit = np.nonzero(bound < F(tau))[0]
    return int(hit[0]) if len(hit) else len(sufA)


def padded_norm(U, users):
    return (np.sqrt((U[users].astype(np.float64) ** 2).sum(1)) * 1.0009765625 * 1.0001).astype(F)


def lowered(tau):
    """the threshold the kernel compares against: strictly below the exact K-th value"""
    tau = np.asarray(tau, dtype=F)
    return np.where(np.isfinite(tau), tau - np.abs(tau) * F(1.52587890625e-5) - F(1e-30), tau).astype(F)
