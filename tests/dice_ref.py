"""Restatement of the DICE contract of include/pda_hip_dice.h for the DICE tests; it holds no test.

    dice_terms     the loss of one batch in torch float64 (or any dtype), term by term
    dice_grads     the same with autograd: the six loss terms and the dense gradients of both tables
    dice_adam      one whole train step: dice_grads, then the project's Adam restatement (oracle.pda_oracle.adam_dense_decay_step)
    pnsm_sets      the sets H and L of a positive by enumeration (no search): what the boundaries are checked against
    pnsm           PNSM in numpy with the counter-based draws of tests/sampler_ref.py, vectorised over the rows of a batch
    parity_data    the train lists the sampler tests draw from (tied popularities; user 0 owns the whole popular side)

Layout: a row of 2d floats is the interest embedding [0, d) followed by the conformity embedding [d, 2d).
"""
import numpy as np
import torch

from sampler_ref import REJECT_CAP, _in_row, _steps, bounded, draw, sample_users

f32 = np.float32
MASK64 = (1 << 64) - 1


def lsig(x):
    return torch.log(torch.sigmoid(x) + 1e-10)


def dis(a, b, kind):
    """Mean over all elements of |a - b| (l1; torch's |.| has the zero subgradient at a == b) or of (a - b)^2 (l2)."""
    return (a - b).abs().mean() if kind == "l1" else ((a - b) ** 2).mean()


def dice_terms(U, I, users, pos, neg, mask, *, w_int, w_con, dis_pen, dis_kind, regs, reg_div):
    """-> dict of the loss terms (0-d tensors of U's dtype).  users / pos / neg: int64 tensors, mask: tensor of 0 / 1."""
    d = U.shape[1] // 2
    m = mask.to(U.dtype)
    u, p, n = U[users], I[pos], I[neg]
    x_int = (u[:, :d] * p[:, :d]).sum(1) - (u[:, :d] * n[:, :d]).sum(1)
    x_con = (u[:, d:] * p[:, d:]).sum(1) - (u[:, d:] * n[:, d:]).sum(1)
    L_click = -lsig(x_int + x_con).mean()
    L_int = -(m * lsig(x_int)).mean()
    L_con = -(m * lsig(-x_con) + (1 - m) * lsig(x_con)).mean()
    S_i, S_u = torch.unique(torch.cat([pos, neg])), torch.unique(users)
    L_dis = dis(I[S_i, :d], I[S_i, d:], dis_kind) + dis(U[S_u, :d], U[S_u, d:], dis_kind)
    reg = regs * 0.5 * ((u ** 2).sum() + (p ** 2).sum() + (n ** 2).sum()) / reg_div        # tf.nn.l2_loss = sum(x^2) / 2
    mf = L_click + w_int * L_int + w_con * L_con - dis_pen * L_dis
    return dict(loss=mf + reg, mf=mf, reg=reg, L_int=L_int, L_con=L_con, L_dis=L_dis)


def dice_grads(U, I, users, pos, neg, mask, dtype=torch.float64, **kw):
    """numpy in, numpy out: (terms float64 [6] = loss, mf, reg, L_int, L_con, L_dis; gU; gI), computed in `dtype`."""
    Ut = torch.tensor(np.asarray(U), dtype=dtype, requires_grad=True)
    It = torch.tensor(np.asarray(I), dtype=dtype, requires_grad=True)
    ix = [torch.as_tensor(np.asarray(a, dtype=np.int64)) for a in (users, pos, neg)]
    t = dice_terms(Ut, It, *ix, torch.as_tensor(np.asarray(mask, dtype=np.int64)), **kw)
    t["loss"].backward()
    terms = np.array([float(t[k].detach()) for k in ("loss", "mf", "reg", "L_int", "L_con", "L_dis")])
    return terms, Ut.grad.numpy(), It.grad.numpy()


def dice_adam(U, I, state, t, lr, users, pos, neg, mask, **kw):
    """One train step in float64: -> (U1, I1, state, terms).  state = dict(mU, vU, mI, vI) or None."""
    from oracle import pda_oracle as po
    terms, gU, gI = dice_grads(U, I, users, pos, neg, mask, **kw)
    if state is None:
        state = {k: np.zeros_like(x, dtype=np.float64) for k, x in (("mU", U), ("vU", U), ("mI", I), ("vI", I))}
    U1, mU, vU = po.adam_dense_decay_step(np.asarray(U, dtype=np.float64), state["mU"], state["vU"], gU, t, lr)
    I1, mI, vI = po.adam_dense_decay_step(np.asarray(I, dtype=np.float64), state["mI"], state["vI"], gI, t, lr)
    return U1, I1, dict(mU=mU, vU=vU, mI=mI, vI=vI), terms


# ---- PNSM ---------------------------------------------------------------------------------------------------------------------------------
def pop_order(pop):
    """-> (order, sorted_pop): the items ascending by (pop, id)."""
    pop = np.asarray(pop, dtype=np.int32)
    order = np.lexsort((np.arange(pop.size), pop)).astype(np.int32)
    return order, pop[order]


def pnsm_sets(pop, p, margin):
    """H and L of positive p by enumeration, in fp32 like the kernel: (sorted ids of H, sorted ids of L)."""
    P, M = f32(pop[p]), f32(margin)
    q = np.asarray(pop).astype(f32)
    return np.nonzero(q > f32(P + M))[0], np.nonzero(q < f32(P - M))[0]


def pnsm_bounds(sorted_pop, pop_p, margin):
    """The two binary searches: H = order[hi_at:], L = order[:lo_end]."""
    sp = np.asarray(sorted_pop).astype(f32)
    P, M = np.asarray(pop_p).astype(f32), f32(margin)
    return np.searchsorted(sp, (P + M).astype(f32), side="right"), np.searchsorted(sp, (P - M).astype(f32), side="left")


def pnsm(seed, step, B, indptr, indices, pop, margin, *, user_pool=None, n_pool=0, users=None):
    """pda_dice_sample for the rows of one batch -> dict(users, pos, neg, mask, from_h, whole, rejections)."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32)
    pop = np.asarray(pop, dtype=np.int32)
    n_items = pop.size
    order, sorted_pop = pop_order(pop)
    r = np.arange(B, dtype=np.int64)
    seed, stp = seed & MASK64, np.broadcast_to(np.atleast_1d(_steps(step)), r.shape)
    u = sample_users(seed, stp, r, B, n_pool, user_pool) if users is None else np.asarray(users, dtype=np.int64)[r]
    b, e = indptr[u], indptr[u + 1]
    ln = e - b
    empty = ln == 0
    idx = np.where(empty, 0, bounded(draw(seed, stp, r, 0), np.maximum(ln, 0)).astype(np.int64))
    pos = np.where(empty, 0, indices[np.where(empty, 0, b + idx)]).astype(np.int64)
    hi_at, lo_end = pnsm_bounds(sorted_pop, pop[pos], margin)
    nH, nL = n_items - hi_at, lo_end
    bit = (draw(seed, stp, r, 2) >> np.uint64(31)).astype(np.int64) != 0
    from_h = np.where((nH > 0) & (nL > 0), bit, nH > 0)
    whole = (nH == 0) & (nL == 0)
    start = np.where(whole, 0, np.where(from_h, hi_at, 0)).astype(np.int64)
    span = np.where(whole, n_items, np.where(from_h, nH, nL)).astype(np.int64)
    neg = np.zeros(B, dtype=np.int64)
    rej = np.zeros(B, dtype=np.int64)
    act = np.arange(B)
    for k in range(REJECT_CAP):
        at = start[act] + bounded(draw(seed, stp[act], r[act], 16 + k), span[act]).astype(np.int64)
        neg[act] = np.where(whole[act], at, order[at])
        act = act[_in_row(indices, b[act], e[act], neg[act])]
        if not act.size:
            break
        rej[act] += 1
    mask = np.where(whole, pop[neg] > pop[pos], from_h).astype(np.uint8)
    return dict(users=u.astype(np.int32), pos=pos.astype(np.int32), neg=neg.astype(np.int32), mask=mask, from_h=from_h & ~whole, whole=whole,
                rejections=rej)


def parity_data(n_users=200):
    """Train lists for the sampler tests -> (indptr int64, indices int32, pop int32), built without a random generator.  100 items in ten
    groups of ten with equal popularity inside a group (ties everywhere), dealt round-robin to users 1 .. n_users - 1, who end up with at
    most six items each: fewer than any H or L, which are unions of whole groups.  User 0 owns the two most popular groups: the H of a
    positive from the second group is the first group, all of it in the user's own history (the rejection cap)."""
    tiers = (1, 2, 3, 4, 6, 8, 10, 14, 20, 30)
    rows = [[] for _ in range(n_users)]
    nxt = 0
    for item in range(100):
        for _ in range(tiers[item // 10]):
            rows[1 + nxt % (n_users - 1)].append(item)
            nxt += 1
    rows[0] = list(range(80, 100))
    rows = [np.unique(np.asarray(r, dtype=np.int32)) for r in rows]
    assert max(len(r) for r in rows[1:]) <= 6 and all(len(r) for r in rows)
    indices = np.concatenate(rows)
    pop = np.bincount(indices, minlength=100).astype(np.int32)
    assert (pop == np.repeat(np.asarray(tiers) + np.asarray([0] * 8 + [1, 1]), 10)).all()
    indptr = np.zeros(n_users + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, indices, pop


PARITY_CASES = [(B, M) for B in (1, 64, 2048) for M in (0.0, 3.0, 1e9)]     # (batch, margin): B <= 200 users draws them distinct, 2 048 with replacement
PARITY_SEED, PARITY_STEP = 2020, 3
