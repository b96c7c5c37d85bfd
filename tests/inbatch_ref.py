"""Restatement of the in-batch softmax contract of include/pda_hip_inbatch.h for the in-batch tests; it holds no test.

    inbatch_terms    the loss of one batch in torch float64 (or any dtype): logits by u @ i.T, masked_fill(-inf), logsumexp; reg per row;
                     `mutant` breaks one clause of it
    inbatch_grads    the same with autograd: the three loss terms and the dense gradients of both tables, on the batch's VALID rows
    exclusion        the train mask of a batch from Python sets of each user's train items (bool [B, B]); pack_mask: the kernel's words
    logq_ref         log q_i of the sampler's columns from the train sets
    make_case        tables, a Zipf batch and a train graph around it; CASES / parity_case: the combinations of the gradient comparison
    ADAM / adam_reference   the three whole Adam steps

Written from the contract, not from the kernel.
"""
import numpy as np
import torch

import ssm_ref
from ssm_ref import DIMS, NI, NU, REGS, tables, tolerance  # noqa: F401  (the tests take them from here)

T = 32                      # max(INBATCH_ROW_TILE, INBATCH_COL_TILE); tests/test_inbatch_host.py holds it against the binding
MUTANTS = ("no_logq", "logq_negs_only", "no_mask", "equal_pos_kept", "no_diag", "reg_per_column", "no_tau_grad", "no_proj")


def _unit(x):
    return x / torch.linalg.vector_norm(x, dim=-1, keepdim=True).clamp_min(1e-12)


def inbatch_terms(U, I, users, pos, *, tau, norm, regs, reg_div, logq=None, excl=None, B=None, mutant=None):
    """-> dict(loss, mf, reg, l) of tensors of U's dtype.  users / pos int64 [R]: the batch's VALID rows; excl bool [R, R]: True where the mask
    excludes column c from row r; logq [n_items] or None; B: the batch size the mean divides by (more than R when rows were dropped).
    mutant: one of MUTANTS -- the contract with one clause broken."""
    R = len(users)
    B = R if B is None else B
    u, it = U[users], I[pos]
    uq, iq = u, it
    if norm:
        if mutant == "no_proj":        # x / |x| with |x| a constant: the gradient loses its projection term
            uq = u / torch.linalg.vector_norm(u, dim=-1, keepdim=True).clamp_min(1e-12).detach()
            iq = it / torch.linalg.vector_norm(it, dim=-1, keepdim=True).clamp_min(1e-12).detach()
        else:
            uq, iq = _unit(u), _unit(it)
    raw = uq @ iq.T
    s = raw / tau
    if mutant == "no_tau_grad":        # the value of raw / tau with the gradient of raw
        s = (raw / tau).detach() + (raw - raw.detach())
    eye = torch.eye(R, dtype=torch.bool)
    if logq is not None and mutant != "no_logq":
        lq = torch.as_tensor(logq, dtype=U.dtype)[pos][None, :].expand(R, R)
        if mutant == "logq_negs_only":
            lq = lq.masked_fill(eye, 0.0)
        s = s - lq
    out = torch.zeros((R, R), dtype=torch.bool)
    if mutant != "equal_pos_kept":
        out |= (pos[:, None] == pos[None, :])
    if excl is not None and mutant != "no_mask":
        out |= torch.as_tensor(excl, dtype=torch.bool)
    out &= ~eye                        # the row's own column is always in ...
    diag = torch.diagonal(s)
    if mutant == "no_diag":            # ... unless the clause is broken
        out |= eye
    lse = torch.logsumexp(s.masked_fill(out, float("-inf")), dim=1)
    if mutant == "no_diag":
        lse = torch.where(torch.isfinite(lse), lse, diag)
    l = lse - diag
    mf = l.sum() / B
    if mutant == "reg_per_column":     # every admitted column regularised again, as the sampled path counts occurrences
        reg = regs * 0.5 * ((u ** 2).sum() + ((~out).to(U.dtype) @ (it ** 2).sum(1)).sum()) / reg_div
    else:
        reg = regs * 0.5 * ((u ** 2).sum() + (it ** 2).sum()) / reg_div
    return dict(loss=mf + reg, mf=mf, reg=reg, l=l, excluded=out)


def inbatch_grads(U, I, users, pos, dtype=torch.float64, **kw):
    """numpy in, numpy out: (terms float64 [3] = loss, mf, reg; gU; gI; l [R]), computed in `dtype`."""
    Ut = torch.tensor(np.asarray(U), dtype=dtype, requires_grad=True)
    It = torch.tensor(np.asarray(I), dtype=dtype, requires_grad=True)
    ix = [torch.as_tensor(np.asarray(a, dtype=np.int64)) for a in (users, pos)]
    t = inbatch_terms(Ut, It, *ix, **kw)
    t["loss"].backward()
    return np.array([float(t[k].detach()) for k in ("loss", "mf", "reg")]), Ut.grad.numpy(), It.grad.numpy(), t["l"].detach().numpy()


def valid_rows(users, pos, nU, nI):
    users, pos = np.asarray(users, dtype=np.int64), np.asarray(pos, dtype=np.int64)
    return (users >= 0) & (users < nU) & (pos >= 0) & (pos < nI)


def reference(U, I, users, pos, *, excl=None, dtype=torch.float64, **kw):
    """inbatch_grads on the valid rows of a batch that may hold ids outside the tables; B stays the length of the batch."""
    ok = valid_rows(users, pos, U.shape[0], I.shape[0])
    keep = np.flatnonzero(ok)
    if excl is not None:
        excl = np.asarray(excl)[np.ix_(keep, keep)]
    return inbatch_grads(U, I, np.asarray(users)[keep], np.asarray(pos)[keep], dtype=dtype, excl=excl, B=len(users), **kw)


# ---- the train graph, the mask and logq ---------------------------------------------------------------------------------------------------------
def exclusion(users, pos, train, nU, nI):
    """bool [B, B]: (r, c) True iff c != r, both rows valid and pos[c] is a train item of users[r].  train: {user: set of items}."""
    B = len(users)
    ok = valid_rows(users, pos, nU, nI)
    member = np.zeros((B, nI), dtype=bool)          # member[r, i]: item i is in the set of users[r]
    for r in np.flatnonzero(ok):
        member[r, list(train.get(int(users[r]), ()))] = True
    out = member[:, np.where(ok, pos, 0)] & ok[None, :] & ok[:, None]
    return out & ~np.eye(B, dtype=bool)


def pack_mask(excl):
    """bool [B, B] -> the kernel's words as int32 [B, ceil(B / 32)]: bit c % 32 of word [r, c / 32]."""
    B = excl.shape[0]
    W = (B + 31) // 32
    bits = np.zeros((B, W * 32), dtype=np.uint64)
    bits[:, :B] = excl
    words = (bits.reshape(B, W, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    return words.view(np.int32)


def unpack_mask(words, B):
    w = np.asarray(words).view(np.uint32).reshape(B, -1)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(B, -1)[:, :B].astype(bool)


def csr(train, nU):
    """{user: set} -> (indptr int64 [nU + 1], indices int32, sorted inside a row)."""
    rows = [np.sort(np.fromiter(train.get(u, ()), dtype=np.int32)) for u in range(nU)]
    indptr = np.zeros(nU + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, (np.concatenate(rows) if indptr[-1] else np.zeros(0, np.int32)).astype(np.int32)


def logq_ref(train, nI, pool):
    """q_i = (1 / n_pool) sum_{u in pool, i in I_u} 1 / |I_u| in float64, log, rounded once; q_i = 0 takes the smallest positive q."""
    q = np.zeros(nI, dtype=np.float64)
    for u in pool:
        items = train.get(int(u), set())
        for i in items:
            q[i] += 1.0 / len(items)
    q /= len(pool)
    q[q == 0] = q[q > 0].min()
    return np.log(q).astype(np.float32)


def zipf(rng, n, nI):
    p = 1.0 / np.arange(1, nI + 1)
    return rng.choice(nI, size=n, p=p / p.sum())


def make_case(seed, d, B, *, distinct=False, grouped=False, nU=NU, nI=NI):
    """-> dict(U, I, users, pos int32 [B], train {user: set}, nU, nI).  Positives are Zipf over the items, so equal positives occur; every user
    has about 8 Zipf train items plus the positives of its rows.  Users: distinct (a permutation), or drawn from 20 so that they repeat.
    grouped: rows sorted by positive; otherwise shuffled as drawn."""
    rng = np.random.default_rng(seed)
    nU = max(nU, B + 5)
    U, I = tables(rng, d, nU, nI)
    users = (rng.permutation(nU)[:B] if distinct else rng.integers(0, min(20, nU), B)).astype(np.int32)
    pos = zipf(rng, B, nI).astype(np.int32)
    if grouped:
        order = np.argsort(pos, kind="stable")
        users, pos = users[order], pos[order]
    train = {u: set(int(i) for i in zipf(rng, 8, nI)) for u in range(nU)}
    for u, p in zip(users, pos):
        train[int(u)].add(int(p))
    return dict(U=U, I=I, users=users, pos=pos, train=train, nU=nU, nI=nI)


def excluded_share(users, pos, excl):
    """The share of the off-diagonal pairs the step leaves out: the mask or equal positives."""
    B = len(users)
    if B < 2:
        return 0.0
    out = (np.asarray(pos)[:, None] == np.asarray(pos)[None, :]) | (excl if excl is not None else False)
    out = out & ~np.eye(B, dtype=bool)
    return out.sum() / (B * (B - 1))


# Every value of every axis with every d: B in {1, 2, T + 3, 2 T + 5} (the column splits are already more than one at T + 3), norm in {0, 1},
# tau in {1, 0.1}, logq on | off, the mask given | null, any order | grouped by positive, users repeated | distinct.  Six per d, 24 cases.
#          B        norm tau  logq mask grouped distinct
COMBOS = ((1, 0, 1.0, 1, 1, False, False),
          (2, 1, 0.1, 0, 0, True, True),
          (T + 3, 0, 0.1, 1, 0, False, True),
          (T + 3, 1, 1.0, 0, 1, True, False),
          (2 * T + 5, 1, 0.1, 1, 1, False, False),
          (2 * T + 5, 0, 1.0, 1, 1, True, True))
CASES = tuple((d,) + c for d in DIMS for c in COMBOS)


def parity_case(d, B, norm, tau, use_logq, use_mask, grouped, distinct):
    """-> (case dict of make_case, logq or None, excl or None): the inputs of one gradient comparison, the same on the CPU and on the GPU."""
    c = make_case(7000 * d + 10 * B + norm, d, B, distinct=distinct, grouped=grouped)
    logq = logq_ref(c["train"], c["nI"], range(c["nU"])) if use_logq else None
    excl = exclusion(c["users"], c["pos"], c["train"], c["nU"], c["nI"]) if use_mask else None
    return c, logq, excl


def case_reference(case, dtype=torch.float64, mutant=None):
    d, B, norm, tau, use_logq, use_mask, grouped, distinct = case
    c, logq, excl = parity_case(*case)
    return reference(c["U"], c["I"], c["users"], c["pos"], excl=excl, logq=logq, tau=tau, norm=norm, regs=REGS, reg_div=B, dtype=dtype, mutant=mutant)


def worst(a, b):
    return max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max(), np.abs(a[2] - b[2]).max())


# ---- three whole Adam steps: d, lr, tau of ssm_ref.ADAM_STEPS, B = 67 ---------------------------------------------------------------------------------
ADAM = dict(d=ssm_ref.ADAM_STEPS["d"], B=67, lr=ssm_ref.ADAM_STEPS["lr"], tau=ssm_ref.ADAM_STEPS["tau"], seed=57)


def adam_case():
    """-> (case dict with the tables and the train graph, [(users, pos) of step 1, 2, 3], logq)."""
    c = make_case(ADAM["seed"], ADAM["d"], ADAM["B"])
    rng = np.random.default_rng(ADAM["seed"] + 1)
    batches = [(c["users"], c["pos"])]
    for _ in range(2):
        users = rng.integers(0, 20, ADAM["B"]).astype(np.int32)
        pos = zipf(rng, ADAM["B"], c["nI"]).astype(np.int32)
        for u, p in zip(users, pos):
            c["train"][int(u)].add(int(p))
        batches.append((users, pos))
    return c, batches, logq_ref(c["train"], c["nI"], range(c["nU"]))


def adam_reference(norm, dtype=torch.float64):
    """The three steps: inbatch_grads, then the project's Adam restatement -> dict(U, I, mU, vU, mI, vI), and the loss terms of every step."""
    from oracle import pda_oracle as po
    c, batches, logq = adam_case()
    U, I = c["U"].astype(np.float64), c["I"].astype(np.float64)
    st = {k: np.zeros_like(x) for k, x in (("mU", U), ("vU", U), ("mI", I), ("vI", I))}
    terms = []
    for t, (users, pos) in enumerate(batches, 1):
        excl = exclusion(users, pos, c["train"], c["nU"], c["nI"])
        Ug, Ig = (U.astype(np.float32).astype(np.float64), I.astype(np.float32).astype(np.float64)) if dtype == torch.float32 else (U, I)
        tm, gU, gI, _ = inbatch_grads(Ug, Ig, users, pos, dtype=dtype, excl=excl, logq=logq, tau=ADAM["tau"], norm=norm, regs=REGS, reg_div=ADAM["B"])
        U, st["mU"], st["vU"] = po.adam_dense_decay_step(U, st["mU"], st["vU"], gU.astype(np.float64), t, ADAM["lr"])
        I, st["mI"], st["vI"] = po.adam_dense_decay_step(I, st["mI"], st["vI"], gI.astype(np.float64), t, ADAM["lr"])
        terms.append(tm)
    return dict(U=U, I=I, **st), terms
