"""Restatement of popularity-weighted negative sampling (include/pda_hip_negpop.h) for its tests; it holds no test.

    weights, build       w_i = (c_i + 1)^beta and Vose's alias table in numpy float64 -> (thr, alias), uint32 each
    slot_counts          how many of the 2^32 words `bounded` sends to each of n slots (Python integers)
    implied              the EXACT distribution a table draws from, as Fractions: the non-uniformity of `bounded` over slots included
    alias_items          one try per (row, draw number): the slot, the coin, the item
    negatives            the rejection loop of negative j of a row -> items and the number of rejected tries
    sample, block        the triplet batch and the [B, N] block on top of tests/sampler_ref.py
    logq_terms, logq_grads   the sampled-softmax loss with logQ in torch (float64 by default), `mutant` breaks one clause of it
    chi2_sf              the tail of a chi-square with an even number of degrees of freedom, in closed form

Written from the contract in the header, not from the kernel.
"""
from fractions import Fraction

import numpy as np
import torch

import sampler_ref as sr

u64 = np.uint64
COIN = 0x80000000
FULL_THR = (1 << 32) - 1
MUTANTS = ("skip_pos", "sign", "by_column")


def weights(counts, beta):
    return (np.asarray(counts, dtype=np.float64) + 1.0) ** float(beta)


def build(w):
    """Vose's method as DESIGN.md 5u states it: p = w n / sum(w); a slot whose p >= 1 when its turn comes is full; a slot below takes
    thr = min(rint(p 2^32), 2^32 - 1) and a large slot as its alias; what is left over when one list runs dry is full."""
    w = np.asarray(w, dtype=np.float64)
    n = len(w)
    p = list(w * n / w.sum())
    thr, alias = [FULL_THR] * n, list(range(n))
    small = [i for i in range(n) if p[i] < 1.0]
    large = [i for i in range(n) if p[i] >= 1.0]
    while small and large:
        s, l = small.pop(), large.pop()
        thr[s], alias[s] = min(int(np.rint(p[s] * 2.0 ** 32)), FULL_THR), l
        p[l] = (p[l] + p[s]) - 1.0
        (large if p[l] >= 1.0 else small).append(l)
    return np.array(thr, dtype=np.uint32), np.array(alias, dtype=np.uint32)


def slot_counts(n):
    """bounded(r, n) == s for exactly ceil((s + 1) 2^32 / n) - ceil(s 2^32 / n) of the 2^32 words r."""
    edge = [-((-s << 32) // n) for s in range(n + 1)]
    return [edge[s + 1] - edge[s] for s in range(n)]


def implied(thr, alias):
    """P_i of every slot's item, exact: slot s comes up with cnt_s / 2^32, keeps itself always when alias_s == s and with thr_s / 2^32
    otherwise (coin < thr, the coin one of 2^32 words), and hands the rest to alias_s.  -> list of Fractions that sum to 1."""
    n = len(thr)
    num = [0] * n                                   # numerators over 2^64
    for s, cnt in enumerate(slot_counts(n)):
        t, a = int(thr[s]), int(alias[s])
        if a == s:
            num[s] += cnt << 32
        else:
            num[s] += cnt * t
            num[a] += cnt * ((1 << 32) - t)
    return [Fraction(x, 1 << 64) for x in num]


def alias_items(seed, step, rows, k, thr, alias):
    """Try with draw number k (scalar or array) of each (step, row) -> slot-space items x in [0, n), int64."""
    thr, alias = np.asarray(thr, dtype=u64), np.asarray(alias, dtype=u64)
    k = np.asarray(k, dtype=u64)
    slot = sr.bounded(sr.draw(seed, step, rows, k), len(thr))
    coin = sr.draw(seed, step, rows, k | u64(COIN))
    other = alias[slot]
    keep = (other == slot) | (coin < thr[slot])
    return np.where(keep, slot, other).astype(np.int64)


def negatives(seed, step, rows, j, thr, alias, lo, indices, b, e):
    """Negative j[i] of row rows[i] (train items indices[b[i]:e[i]]): tries 16 + 4096 j + a, a = 0 .. 4095, rejected while a train item; the
    last draw stays.  -> (items int64, rejections int64)."""
    rows, j = np.asarray(rows, dtype=np.int64), np.asarray(j, dtype=np.int64)
    step = np.broadcast_to(np.atleast_1d(sr._steps(step)), rows.shape)
    neg = np.full(len(rows), lo, dtype=np.int64)
    rej = np.zeros(len(rows), dtype=np.int64)
    act = np.arange(len(rows))
    for a in range(sr.REJECT_CAP):
        neg[act] = lo + alias_items(seed & sr.MASK, step[act], rows[act], 16 + 4096 * j[act] + a, thr, alias)
        act = act[sr._in_row(indices, b[act], e[act], neg[act])]
        if not act.size:
            break
        rej[act] += 1
    return neg, rej


def sample(seed, step, B, indptr, indices, thr, alias, *, neg_lo=0, slots=None, user_pool=None, n_pool=0, users=None, pop_matrix=None):
    """pda_negpop_sample_triplets for one batch -> dict(users, pos, neg, pos_pop, neg_pop, rejections): sampler_ref.sample's users, positives
    and slots, the negative through the table."""
    lo, hi = neg_lo, neg_lo + len(thr)
    base = sr.sample(seed, step, B, indptr, indices, slots=slots, user_pool=user_pool, n_pool=n_pool, users=users, neg_range=(lo, hi),
                     pop_matrix=pop_matrix)
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32)
    u = base["users"].astype(np.int64)
    r = np.arange(B, dtype=np.int64)
    neg, rej = negatives(seed, step, r, np.zeros(B, dtype=np.int64), thr, alias, lo, indices, indptr[u], indptr[u + 1])
    out = dict(users=base["users"], pos=base["pos"], neg=neg.astype(np.int32), pos_pop=base["pos_pop"], neg_pop=None, rejections=rej)
    if pop_matrix is not None:
        # the slot of the row: that of the drawn train entry, or of an empty row the draw number 1
        empty = base["idx"] < 0
        slot = np.zeros(B, dtype=np.int64)
        slot[empty] = sr.bounded(sr.draw(seed & sr.MASK, step, r[empty], 1), pop_matrix.shape[1]).astype(np.int64)
        if slots is not None and indices.size:
            slot[~empty] = np.asarray(slots)[(indptr[u] + base["idx"])[~empty]]
        out["neg_pop"] = pop_matrix[neg, slot]
    return out


def block(seed, step, B, N, indptr, indices, thr, alias, *, neg_lo=0, user_pool=None, n_pool=0, users=None):
    """pda_negpop_ssm_sample for one batch -> dict(users, pos, negs [B, N], rejections [B, N])."""
    lo, hi = neg_lo, neg_lo + len(thr)
    base = sr.sample(seed, step, B, indptr, indices, user_pool=user_pool, n_pool=n_pool, users=users, neg_range=(lo, hi))
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32)
    u = np.repeat(base["users"].astype(np.int64), N)
    r, j = np.repeat(np.arange(B, dtype=np.int64), N), np.tile(np.arange(N, dtype=np.int64), B)
    neg, rej = negatives(seed, step, r, j, thr, alias, lo, indices, indptr[u], indptr[u + 1])
    return dict(users=base["users"], pos=base["pos"], negs=neg.astype(np.int32).reshape(B, N), rejections=rej.reshape(B, N))


# ---- the sampled-softmax loss with logQ (include/pda_hip_ssm.h) --------------------------------------------------------------------------------
def _unit(x):
    return x / torch.linalg.vector_norm(x, dim=-1, keepdim=True).clamp_min(1e-12)


def logq_terms(U, I, users, pos, negs, logq, *, tau, norm, regs, reg_div, mutant=None):
    """-> dict(loss, mf, reg), 0-d tensors of U's dtype: s_k = (u . i_k) / tau - logq[item_k] for every k = 0 .. N, the positive's included;
    logq None: no correction.  mutant: one of MUTANTS -- skip_pos (the positive's logit is left uncorrected), sign (+ logq), by_column
    (logq[k], the column's number, in place of logq[item_k])."""
    B = len(users)
    ids = torch.cat([pos[:, None], negs], dim=1)                                     # [B, N + 1]
    u, items = U[users], I[ids]
    uq, iq = (_unit(u), _unit(items)) if norm else (u, items)
    s = torch.einsum("rd,rkd->rk", uq, iq) / tau
    if logq is not None:
        lq = logq[ids]
        if mutant == "by_column":
            lq = logq[torch.arange(ids.shape[1]) % len(logq)][None, :].expand_as(s)
        if mutant == "skip_pos":
            lq = torch.cat([torch.zeros_like(lq[:, :1]), lq[:, 1:]], dim=1)
        s = s + lq if mutant == "sign" else s - lq
    mf = (torch.logsumexp(s, dim=1) - s[:, 0]).sum() / B
    reg = regs * 0.5 * ((u ** 2).sum() + (items ** 2).sum()) / reg_div
    return dict(loss=mf + reg, mf=mf, reg=reg)


def logq_grads(U, I, users, pos, negs, logq, dtype=torch.float64, **kw):
    """numpy in, numpy out: (terms float64 [3] = loss, mf, reg; gU; gI), computed in `dtype` (logq has no gradient)."""
    Ut = torch.tensor(np.asarray(U), dtype=dtype, requires_grad=True)
    It = torch.tensor(np.asarray(I), dtype=dtype, requires_grad=True)
    ix = [torch.as_tensor(np.asarray(a, dtype=np.int64)) for a in (users, pos, negs)]
    lq = None if logq is None else torch.tensor(np.asarray(logq), dtype=dtype)
    t = logq_terms(Ut, It, *ix, lq, **kw)
    t["loss"].backward()
    return np.array([float(t[k].detach()) for k in ("loss", "mf", "reg")]), Ut.grad.numpy(), It.grad.numpy()


def loss_tolerance(tau, logq):
    """1e-5 max(1, 1 / tau + max |logq|): the project's figure per unit (ssm_ref.TOL) times the size a logit now has."""
    m = 0.0 if logq is None else float(np.abs(np.asarray(logq, dtype=np.float64)).max())
    return 1e-5 * max(1.0, 1.0 / float(tau) + m)


def chi2_sf(x, dof):
    """P(chi-square with an EVEN number of degrees of freedom > x), in closed form: exp(-x / 2) sum_{i < dof / 2} (x / 2)^i / i!.
    A statistic lies below the 1 - p quantile exactly when this exceeds p."""
    assert dof % 2 == 0 and dof > 0
    import math
    h = x / 2.0
    term, total = 1.0, 1.0
    for i in range(1, dof // 2):
        term *= h / i
        total += term
    return math.exp(-h) * total if h < 700 else 0.0


# ---- inputs shared by the host and the GPU tests -------------------------------------------------------------------------------------------------
def pareto_counts(n, seed=7):
    """Pareto-skewed train counts of n items: a few items hold most pairs, many hold none."""
    rng = np.random.default_rng(seed + n)
    return np.floor(rng.pareto(1.2, n) * 3.0).astype(np.int64)


def toy_graph(n_users, n_items, seed, *, heavy=True, empty_every=7, neg_lo=0):
    """A train CSR with skewed items: user u holds a sorted sample of the items (a heavy user holds most of them; every empty_every-th user
    holds none).  -> (indptr int64, indices int32, slots int32 in [0, 4))."""
    rng = np.random.default_rng(seed)
    p = 1.0 / (1.0 + np.arange(n_items)) ** 0.8
    p /= p.sum()
    rows = []
    for u in range(n_users):
        if empty_every and u % empty_every == empty_every - 1:
            k = 0
        elif heavy and u % 11 == 0:
            k = max(1, (n_items * 9) // 10)
        else:
            k = int(rng.integers(1, max(2, min(n_items, 12))))
        k = min(k, n_items)
        rows.append(np.sort(rng.choice(n_items, size=k, replace=False, p=p)).astype(np.int32))
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    indptr = np.zeros(n_users + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    indices = np.concatenate(rows) if rows else np.zeros(0, np.int32)
    slots = rng.integers(0, 4, indices.size).astype(np.int32)
    return indptr, indices.astype(np.int32), slots
