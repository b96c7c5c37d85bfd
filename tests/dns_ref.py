"""Numpy restatement, in float64, of dynamic hard-negative sampling (include/pda_hip_dns.h, pda_amd/csrc/pda_dns.hip) for the DNS tests.

    sample        one batch: the user, positive and popularity columns of sampler_ref.sample, the candidates of ssm_ref.ssm_sample, their
                  float64 scores under one of the two heads, the order of every row, the pick index t = bounded(draw(seed, step, r, 3),
                  min(topn, M)) and the picked candidate
    scores        the two heads in float64, with the a-priori bound of the kernel's fp32 score against them
    order         the order rule: score descending, then column ascending; NaNs behind every number, among themselves by column
    rank_interval the positions a candidate may take when every score is only known to its bound

The bound (score_bound).  The kernel's dot product is a sum of d fp32 products added in SOME order (four per lane, then a butterfly): for any
order the computed value x^ obeys |x^ - x| <= gamma_d sum_k |u_k i_k| with gamma_d = d eps / (1 - d eps), eps = 2^-24 the unit roundoff
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (3.5): d - 1 additions and one product rounding per term give at most d
roundings on any term).  gamma_d <= 2 d eps for d <= 2^22, which is the figure used:
    raw head:   e_raw = 2 d 2^-24 sum_k |u_k i_k|.
The popularity head is g(x) pop with g = elu + 1, g(x) = x + 1 for x > 0 and exp(x) otherwise.  g is 1-Lipschitz (|g'| <= 1 on both
branches, continuous at 0), so |g(x^) - g(x)| <= e_raw.  The kernel evaluates g(x^) with one fp32 addition (half an ulp) or one expf, which
the HIP device library documents to 1 ulp; EXPF_ULPS = 4 ulps = 8 eps relative are granted, a few as the contract says.  The product with
pop >= 0 (an fp32, exact in float64) is one more rounding.  Together, with g^ <= g(x) + e_raw:
    |s^ - s| <= pop (e_raw + (2 EXPF_ULPS + 1) eps (g(x) + e_raw)) (1 + eps)  +  the spacing of the denormals, 2^-149,
and the factor (1 + eps) of the last rounding is covered by granting one more eps: (2 EXPF_ULPS + 2).  It is a bound, not a tuned number:
a candidate outside it means the kernel (or this derivation) is wrong.
"""
import numpy as np

import sampler_ref as sr
import ssm_ref

HEAD_RAW, HEAD_POP = 0, 1
EPS = 2.0 ** -24
EXPF_ULPS = 4
PICK_DRAW = 3


NU, NI, N_SLOTS = 300, 200, 5
EMPTY_USER, FULL_USER, FREE_ITEM = 3, 4, 77     # a user without train items; a user whose train row leaves FREE_ITEM alone in [0, NI)


def graph(seed=11):
    """The train CSR every DNS test draws from: NU users over NI items, rows of 0 .. 30 sorted items with a time slot each; EMPTY_USER has
    none, FULL_USER has every item but FREE_ITEM.  -> (indptr int64, indices int32, slots int32)."""
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(NI, rng.integers(1, 31), replace=False)) for _ in range(NU)]
    rows[EMPTY_USER] = np.zeros(0, dtype=np.int64)
    rows[FULL_USER] = np.delete(np.arange(NI), FREE_ITEM)
    indptr = np.zeros(NU + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.concatenate(rows).astype(np.int32)
    return indptr, indices, rng.integers(0, N_SLOTS, len(indices)).astype(np.int32)


def exact_tables(d, seed=5):
    """Tables whose entries are multiples of 1/8 in [-1, 1]: every product has at most 6 fraction bits and every partial sum of d <= 256 of
    them stays below 2^8, so an fp32 dot product is exact in ANY order (14 of 24 significand bits)."""
    rng = np.random.default_rng(seed + d)
    return (rng.integers(-8, 9, (NU, d)) / 8.0).astype(np.float32), (rng.integers(-8, 9, (NI, d)) / 8.0).astype(np.float32)


def gaussian_tables(d, seed=6):
    rng = np.random.default_rng(seed + d)
    return rng.standard_normal((NU, d)).astype(np.float32), rng.standard_normal((NI, d)).astype(np.float32)


def pop_matrix(seed=8):
    return (np.random.default_rng(seed).uniform(0.05, 1.0, (NI, N_SLOTS)) ** 0.22).astype(np.float32)


def slots_of(base, seed, step, indptr, slots, n_slots):
    """The time slot of every row of a sampler_ref.sample batch: the drawn entry's (0 without slots), an empty row's from draw number 1."""
    u = base["users"].astype(np.int64)
    B = len(u)
    indptr = np.asarray(indptr, dtype=np.int64)
    idx = base["idx"]
    slot = np.zeros(B, dtype=np.int64)
    empty = idx < 0
    if n_slots > 0 and empty.any():
        r = np.arange(B, dtype=np.int64)[empty]
        slot[empty] = sr.bounded(sr.draw(seed & sr.MASK, np.broadcast_to(sr._steps(step), r.shape), r, 1), n_slots).astype(np.int64)
    if slots is not None:
        slot[~empty] = np.asarray(slots)[(indptr[u] + idx)[~empty]]
    return slot


def scores(U, I, users, cand, head, pop_matrix=None, slot=None):
    """-> (float64 scores [B, M], bound [B, M]) of the candidates cand [B, M] of the rows' users under `head`."""
    U64, I64 = np.asarray(U, dtype=np.float64), np.asarray(I, dtype=np.float64)
    d = U64.shape[1]
    u = U64[np.asarray(users, dtype=np.int64)]
    cand = np.asarray(cand, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        # (every user against every item, then the candidates' columns: the same float64 numbers as a gather first, far less memory)
        x = np.take_along_axis(u @ I64.T, cand, 1)
        e_raw = 2.0 * d * EPS * np.take_along_axis(np.abs(u) @ np.abs(I64).T, cand, 1)
        if head == HEAD_RAW:
            return x, e_raw
        p = np.asarray(pop_matrix, dtype=np.float64)[np.asarray(cand, dtype=np.int64), np.asarray(slot, dtype=np.int64)[:, None]]
        g = np.where(x > 0, x + 1.0, np.exp(np.minimum(x, 0.0)))
        g = np.where(np.isnan(x), np.nan, g)
        return g * p, p * (e_raw + (2 * EXPF_ULPS + 2) * EPS * (g + e_raw)) + 2.0 ** -149


def order(s):
    """s [B, M] -> the columns of every row in the order of the contract: [B, M] int64, position 0 first."""
    s = np.asarray(s, dtype=np.float64)
    B, M = s.shape
    nan = np.isnan(s)
    key = np.where(nan, 0.0, s)
    col = np.broadcast_to(np.arange(M), (B, M))
    out = np.empty((B, M), dtype=np.int64)
    for r in range(B):
        out[r] = np.lexsort((col[r], -key[r], nan[r]))          # last key first: NaNs behind, then score descending, then column
    return out


def pick_index(seed, step, B, topn, M):
    """t of every row: bounded(draw(seed, step, r, 3), min(topn, M))."""
    r = np.arange(B, dtype=np.int64)
    return sr.bounded(sr.draw(seed & sr.MASK, np.broadcast_to(sr._steps(step), r.shape), r, PICK_DRAW), min(int(topn), int(M))).astype(np.int64)


def sample(seed, step, B, M, topn, U, I, indptr, indices, *, head=HEAD_RAW, slots=None, user_pool=None, n_pool=0, users=None, neg_range,
           pop_matrix=None):
    """pda_dns_sample_f32 for one batch -> dict(users, pos, neg, pos_pop, neg_pop, cand [B, M], score [B, M] float64, bound [B, M], order
    [B, M], t [B], pick_col [B], slot [B])."""
    base = sr.sample(seed, step, B, indptr, indices, slots=slots, user_pool=user_pool, n_pool=n_pool, users=users, neg_range=neg_range,
                     pop_matrix=pop_matrix)
    cand = ssm_ref.ssm_sample(seed, step, B, M, indptr, indices, user_pool=user_pool, n_pool=n_pool, users=users, neg_range=neg_range)["negs"]
    n_slots = 0 if pop_matrix is None else pop_matrix.shape[1]
    slot = slots_of(base, seed, step, indptr, slots, n_slots)
    s, bound = scores(U, I, base["users"], cand, head, pop_matrix, slot)
    o = order(s)
    t = pick_index(seed, step, B, topn, M)
    col = o[np.arange(B), t]
    neg = cand[np.arange(B), col].astype(np.int32)
    out = dict(users=base["users"], pos=base["pos"], neg=neg, pos_pop=base["pos_pop"], neg_pop=None, cand=cand, score=s, bound=bound, order=o, t=t,
               pick_col=col.astype(np.int32), slot=slot, neg0=base["neg"], neg0_pop=base["neg_pop"])
    if pop_matrix is not None:
        out["neg_pop"] = pop_matrix[neg.astype(np.int64), slot]
    return out


def rank_interval(s, bound, col):
    """Row by row, for the candidate in column col[r]: (how many candidates are better than it by more than the two bounds allow, how many --
    itself included -- are not worse than it by more than they allow).  A kernel within its bounds that picks position t has first <= t < second.
    NaN scores stand behind every number and never inside an interval."""
    s, bound = np.asarray(s, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    B = s.shape[0]
    rows = np.arange(B)
    sp, bp = s[rows, col][:, None], bound[rows, col][:, None]
    with np.errstate(invalid="ignore"):
        surely_better = (s - bound > sp + bp).sum(1)
        maybe_not_worse = (s + bound >= sp - bp).sum(1)
    return surely_better, maybe_not_worse


def single_item_share(ref):
    """The share of rows in which every candidate the bound admits at the picked position is the same ITEM as the reference's pick."""
    lo, hi = rank_interval(ref["score"], ref["bound"], ref["pick_col"])
    B, M = ref["cand"].shape
    rows = np.arange(B)
    s, b = ref["score"], ref["bound"]
    sp, bp = s[rows, ref["pick_col"]][:, None], b[rows, ref["pick_col"]][:, None]
    near = (np.abs(s - sp) <= b + bp)                                     # the candidates whose order against the pick the bound leaves open
    same = ref["cand"] == ref["neg"][:, None]
    assert ((lo <= ref["t"]) & (ref["t"] < hi)).all()
    return float((near <= same).all(1).mean())
