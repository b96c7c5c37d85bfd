"""Restatement of the full-catalogue softmax contract of include/pda_hip_fullsm.h for the full-softmax tests; it holds no test.

    fullsm_terms     the loss of one batch in torch float64 (or any dtype): logits by u @ I.T, masked_fill(-inf), logsumexp; reg per row;
                     `mutant` breaks one clause of it
    fullsm_grads     the same with autograd: the three loss terms, the dense gradients of both tables, l_r and (m_r, log se_r)
    membership       bool [B, n_items]: item c is a train item of users[r], from Python sets
    make_case        tables, a Zipf batch and a train graph around it; CASES / parity_case: the combinations of the gradient comparison
    ADAM / adam_reference   the three whole Adam steps

Written from the contract, not from the kernel.
"""
import numpy as np
import torch

import ssm_ref
from inbatch_ref import csr, valid_rows, worst, zipf  # noqa: F401  (the tests take them from here)
from ssm_ref import DIMS, NU, REGS, tables, tolerance  # noqa: F401

T = 32                      # max(FULLSM_ROW_TILE, FULLSM_COL_TILE); tests/test_fullsm_host.py holds it against the binding
MUTANTS = ("no_mask", "pos_masked", "reg_per_column", "no_proj", "no_tau_grad", "mean_over_valid", "last_tile_dropped")


def _unit(x):
    return x / torch.linalg.vector_norm(x, dim=-1, keepdim=True).clamp_min(1e-12)


def fullsm_terms(U, I, users, pos, *, tau, norm, regs, reg_div, member=None, B=None, mutant=None):
    """-> dict(loss, mf, reg, l, m, logse) of tensors of U's dtype.  users / pos int64 [R]: the batch's VALID rows; member bool [R, n_items]: True
    where item c is a train item of users[r] (the row's own positive may be among them: it stays in); B: the batch size the mean divides by
    (more than R when rows were dropped).  mutant: one of MUTANTS -- the contract with one clause broken."""
    R, nI = len(users), I.shape[0]
    B = R if B is None else B
    u, it = U[users], I[pos]
    uq, iq = u, I
    if norm:
        if mutant == "no_proj":        # x / |x| with |x| a constant: the gradient loses its projection term
            uq = u / torch.linalg.vector_norm(u, dim=-1, keepdim=True).clamp_min(1e-12).detach()
            iq = I / torch.linalg.vector_norm(I, dim=-1, keepdim=True).clamp_min(1e-12).detach()
        else:
            uq, iq = _unit(u), _unit(I)
    raw = uq @ iq.T
    s = raw / tau
    if mutant == "no_tau_grad":        # the value of raw / tau with the gradient of raw
        s = (raw / tau).detach() + (raw - raw.detach())
    own = torch.zeros((R, nI), dtype=torch.bool)
    own[torch.arange(R), pos] = True
    out = torch.zeros((R, nI), dtype=torch.bool)
    if member is not None and mutant != "no_mask":
        out |= torch.as_tensor(member, dtype=torch.bool)
    if mutant == "last_tile_dropped":  # the columns behind the last full tile of 32 never enter
        out[:, (nI // T) * T:] = True
    if not (mutant == "pos_masked" and member is not None):
        out &= ~own                    # the row's own positive is always in ...
    s_pos = s[torch.arange(R), pos]
    masked = s.masked_fill(out, float("-inf"))
    lse = torch.logsumexp(masked, dim=1)
    if mutant == "pos_masked":         # ... unless the clause is broken (a row with nothing left keeps its positive)
        lse = torch.where(torch.isfinite(lse), lse, s_pos)
    l = lse - s_pos
    mf = l.sum() / (R if mutant == "mean_over_valid" else B)
    if mutant == "reg_per_column":     # every admitted column regularised again, as the sampled path counts occurrences
        reg = regs * 0.5 * ((u ** 2).sum() + ((~out).to(U.dtype) @ (I ** 2).sum(1)).sum()) / reg_div
    else:
        reg = regs * 0.5 * ((u ** 2).sum() + (it ** 2).sum()) / reg_div
    m = masked.max(dim=1).values
    return dict(loss=mf + reg, mf=mf, reg=reg, l=l, m=m, logse=lse - m)


def fullsm_grads(U, I, users, pos, dtype=torch.float64, **kw):
    """numpy in, numpy out: (terms float64 [3] = loss, mf, reg; gU; gI; l [R]; stats [R, 2] = (m, log se)), computed in `dtype`."""
    Ut = torch.tensor(np.asarray(U), dtype=dtype, requires_grad=True)
    It = torch.tensor(np.asarray(I), dtype=dtype, requires_grad=True)
    ix = [torch.as_tensor(np.asarray(a, dtype=np.int64)) for a in (users, pos)]
    t = fullsm_terms(Ut, It, *ix, **kw)
    t["loss"].backward()
    stats = np.stack([t["m"].detach().numpy(), t["logse"].detach().numpy()], axis=1)
    return (np.array([float(t[k].detach()) for k in ("loss", "mf", "reg")]), Ut.grad.numpy(), It.grad.numpy(), t["l"].detach().numpy(),
            stats.astype(np.float64))


def reference(U, I, users, pos, *, member=None, dtype=torch.float64, **kw):
    """fullsm_grads on the valid rows of a batch that may hold ids outside the tables; B stays the length of the batch."""
    keep = np.flatnonzero(valid_rows(users, pos, U.shape[0], I.shape[0]))
    if member is not None:
        member = np.asarray(member)[keep]
    return fullsm_grads(U, I, np.asarray(users)[keep], np.asarray(pos)[keep], dtype=dtype, member=member, B=len(users), **kw)


def membership(users, train, nU, nI):
    """bool [B, n_items]: (r, c) True iff users[r] is a valid user and c is one of its train items.  train: {user: set of items}."""
    out = np.zeros((len(users), nI), dtype=bool)
    for r, u in enumerate(users):
        if 0 <= int(u) < nU:
            out[r, list(train.get(int(u), ()))] = True
    return out


def make_case(seed, d, B, nI, *, distinct=False, drop=False, nU=NU):
    """-> dict(U, I, users, pos int32 [B], train {user: set}, nU, nI).  Positives are Zipf over the items, so equal positives occur; every user
    holds about a sixth of the catalogue (Zipf, without repeats) plus the positives of its rows as train items.  Users: distinct (a
    permutation), or drawn from 20 so that they repeat.  drop: five ids of the batch lie outside the tables (B >= 40)."""
    rng = np.random.default_rng(seed)
    nU = max(nU, B + 5)
    U, I = tables(rng, d, nU, nI)
    users = (rng.permutation(nU)[:B] if distinct else rng.integers(0, min(20, nU), B)).astype(np.int32)
    pos = zipf(rng, B, nI).astype(np.int32)
    p = 1.0 / np.arange(1, nI + 1)
    train = {u: set(int(i) for i in rng.choice(nI, size=max(3, nI // 6), replace=False, p=p / p.sum())) for u in range(nU)}
    for u, q in zip(users, pos):
        train[int(u)].add(int(q))
    if drop:
        users[1], pos[5], users[T - 1], pos[T], users[B - 1] = -1, nI, nU, -7, nU + 9
    return dict(U=U, I=I, users=users, pos=pos, train=train, nU=nU, nI=nI)


# Every value of every axis with every d: B in {1, 33, 69}, n_items in {20, 70, 257, 5 000} (one partial tile; tiles plus a remainder; one item
# past a tile edge; more than one column split), norm in {0, 1}, tau in {1, 0.1}, the train mask on | off, users repeated | distinct (with
# PDA_UPD_USERS_DISTINCT), and one batch with five ids outside the tables.  Six per d, 24 cases.
#          B   n_items norm tau  mask distinct drop
COMBOS = ((1, 20, 0, 1.0, 1, False, False),
          (33, 70, 1, 0.1, 0, True, False),
          (69, 257, 0, 0.1, 1, False, True),
          (69, 5000, 1, 1.0, 1, True, False),
          (33, 5000, 0, 1.0, 0, False, False),
          (69, 70, 1, 0.1, 1, False, False))
CASES = tuple((d,) + c for d in DIMS for c in COMBOS)


def case_id(c):
    return "d%d-B%d-nI%d-norm%d-tau%g-mask%d-%s%s" % (c[0], c[1], c[2], c[3], c[4], c[5], "distinct" if c[6] else "rep", "-drop" if c[7] else "")


def parity_case(d, B, nI, norm, tau, use_mask, distinct, drop):
    """-> (case dict of make_case, member or None): the inputs of one gradient comparison, the same on the CPU and on the GPU."""
    c = make_case(9000 * d + 10 * B + nI + norm, d, B, nI, distinct=distinct, drop=drop)
    return c, (membership(c["users"], c["train"], c["nU"], nI) if use_mask else None)


def case_reference(case, dtype=torch.float64, mutant=None):
    d, B, nI, norm, tau, use_mask, distinct, drop = case
    c, member = parity_case(*case)
    return reference(c["U"], c["I"], c["users"], c["pos"], member=member, tau=tau, norm=norm, regs=REGS, reg_div=B, dtype=dtype, mutant=mutant)


# ---- three whole Adam steps: d, lr, tau of ssm_ref.ADAM_STEPS, B = 67, the 200 items of ssm_ref ---------------------------------------------------------
ADAM = dict(d=ssm_ref.ADAM_STEPS["d"], B=67, nI=ssm_ref.NI, lr=ssm_ref.ADAM_STEPS["lr"], tau=ssm_ref.ADAM_STEPS["tau"], seed=61)


def adam_case():
    """-> (case dict with the tables and the train graph, [(users, pos) of step 1, 2, 3])."""
    c = make_case(ADAM["seed"], ADAM["d"], ADAM["B"], ADAM["nI"])
    rng = np.random.default_rng(ADAM["seed"] + 1)
    batches = [(c["users"], c["pos"])]
    for _ in range(2):
        users = rng.integers(0, 20, ADAM["B"]).astype(np.int32)
        pos = zipf(rng, ADAM["B"], c["nI"]).astype(np.int32)
        for u, q in zip(users, pos):
            c["train"][int(u)].add(int(q))
        batches.append((users, pos))
    return c, batches


def adam_reference(norm, dtype=torch.float64):
    """The three steps: fullsm_grads, then the project's Adam restatement -> dict(U, I, mU, vU, mI, vI), and the loss terms of every step."""
    from oracle import pda_oracle as po
    c, batches = adam_case()
    U, I = c["U"].astype(np.float64), c["I"].astype(np.float64)
    st = {k: np.zeros_like(x) for k, x in (("mU", U), ("vU", U), ("mI", I), ("vI", I))}
    terms = []
    for t, (users, pos) in enumerate(batches, 1):
        member = membership(users, c["train"], c["nU"], c["nI"])
        Ug, Ig = (U.astype(np.float32).astype(np.float64), I.astype(np.float32).astype(np.float64)) if dtype == torch.float32 else (U, I)
        tm, gU, gI, _, _ = fullsm_grads(Ug, Ig, users, pos, dtype=dtype, member=member, tau=ADAM["tau"], norm=norm, regs=REGS, reg_div=ADAM["B"])
        U, st["mU"], st["vU"] = po.adam_dense_decay_step(U, st["mU"], st["vU"], gU.astype(np.float64), t, ADAM["lr"])
        I, st["mI"], st["vI"] = po.adam_dense_decay_step(I, st["mI"], st["vI"], gI.astype(np.float64), t, ADAM["lr"])
        terms.append(tm)
    return dict(U=U, I=I, **st), terms
