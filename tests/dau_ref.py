"""Restatement of the DirectAU contract of include/pda_hip_dau.h for the DirectAU tests; it holds no test.

    dau_terms        the loss of one batch in torch float64 (or any dtype), from the DEFINITION: the masked matrix of exp(-t |x^_a - x^_b|^2),
                     its sum S and the pair count P, log(S / P); `mutant` breaks one clause of it
    dau_grads        the same with autograd: the three loss terms, the dense gradients of both tables and (align, uni_U, uni_I)
    reference        dau_grads on the valid rows of a batch that may hold ids outside the tables
    make_case        tables with rows of norm near 1, a Zipf batch; CASES / parity_case: the combinations of the gradient comparison
    ADAM / adam_reference   the three whole Adam steps

Written from the contract, not from the kernel: the kernel takes its gradient from the row sums r_a and G_a = sum_b e_ab x^_b, this file never
forms them.
"""
import numpy as np
import torch

import inbatch_ref
from ssm_ref import DIMS, REGS  # noqa: F401  (the tests take them from here)

T = 32                      # DAU_TILE; tests/test_dau_host.py holds it against the binding
NU, NI = 80, 40             # items repeat inside every batch of T + 3 rows and more
TOL = 1e-5
MUTANTS = ("no_proj", "uni_per_row", "same_dropped", "same_kept", "diag_kept", "half_gamma_missing", "t_not_in_grad", "align_unnormalised",
           "reg_per_occurrence")


def tolerance(t, gamma):
    """1e-5 max(1, 2 t gamma) absolute on every loss term and gradient element: the project's fp32 figure times the bound of the uniformity
    coefficient per unit row (r_a / S <= 1, |x^_a - x^_b| <= 2, weight gamma / 2)."""
    return TOL * max(1.0, 2.0 * float(t) * float(gamma))


def _unit(x, detach_norm=False):
    n = torch.linalg.vector_norm(x, dim=-1, keepdim=True).clamp_min(1e-12)
    return x / (n.detach() if detach_norm else n)


def _uniformity(x, ids, *, t, same, mutant):
    """-> (uni, n_a [R]) of one side: x [R, d] the unit rows, ids int64 [R]."""
    R = x.shape[0]
    eye = torch.eye(R, dtype=torch.bool)
    adm = ~eye
    drop = same == "drop"
    if mutant == "same_dropped":
        drop = True
    if mutant == "same_kept":
        drop = False
    if drop:
        adm = adm & (ids[:, None] != ids[None, :])
    if mutant == "diag_kept":
        adm = adm | eye
    sq = (x * x).sum(1)
    d2 = sq[:, None] + sq[None, :] - 2.0 * (x @ x.T)
    arg = -t * d2
    if mutant == "t_not_in_grad":       # the value of exp(-t d2) with the gradient of exp(-d2)
        arg = arg.detach() - (d2 - d2.detach())
    e = torch.where(adm, torch.exp(arg), torch.zeros_like(arg))
    n = adm.sum(1)
    P = float(n.sum()) / 2.0
    if P <= 0:
        return x.sum() * 0.0, n
    if mutant == "uni_per_row":         # a log-mean-exp per row, averaged over the rows that have a pair
        has = n > 0
        return torch.log(e.sum(1)[has] / n[has].to(x.dtype)).mean(), n
    return torch.log(e.sum() / 2.0 / P), n


def dau_terms(U, I, users, pos, *, t, gamma, same, regs, reg_div, B=None, mutant=None):
    """-> dict(loss, mf, reg, align, uni_u, uni_i) of tensors of U's dtype.  users / pos int64 [R]: the batch's VALID rows; B: the batch size
    the alignment mean divides by (more than R when rows were dropped).  mutant: one of MUTANTS -- the contract with one clause broken."""
    R = len(users)
    B = R if B is None else B
    u, it = U[users], I[pos]
    uq, iq = _unit(u, mutant == "no_proj"), _unit(it, mutant == "no_proj")
    if mutant == "align_unnormalised":
        align = ((u - it) ** 2).sum() / B
    else:
        align = ((uq - iq) ** 2).sum() / B
    uni_u, n_u = _uniformity(uq, users, t=t, same=same, mutant=mutant)
    uni_i, n_i = _uniformity(iq, pos, t=t, same=same, mutant=mutant)
    w = gamma if mutant == "half_gamma_missing" else gamma / 2.0
    mf = align + w * (uni_u + uni_i)
    if mutant == "reg_per_occurrence":  # a row regularised again for every pair it forms in its Gram matrix
        reg = regs * 0.5 * (((1 + n_u).to(U.dtype) * (u ** 2).sum(1)).sum() + ((1 + n_i).to(U.dtype) * (it ** 2).sum(1)).sum()) / reg_div
    else:
        reg = regs * 0.5 * ((u ** 2).sum() + (it ** 2).sum()) / reg_div
    return dict(loss=mf + reg, mf=mf, reg=reg, align=align, uni_u=uni_u, uni_i=uni_i)


def dau_grads(U, I, users, pos, dtype=torch.float64, **kw):
    """numpy in, numpy out: (terms float64 [3] = loss, mf, reg; gU; gI; stat float64 [3] = align, uni_U, uni_I), computed in `dtype`."""
    Ut = torch.tensor(np.asarray(U), dtype=dtype, requires_grad=True)
    It = torch.tensor(np.asarray(I), dtype=dtype, requires_grad=True)
    ix = [torch.as_tensor(np.asarray(a, dtype=np.int64)) for a in (users, pos)]
    tm = dau_terms(Ut, It, *ix, **kw)
    gU, gI = torch.zeros_like(Ut), torch.zeros_like(It)
    if len(ix[0]):
        tm["loss"].backward()
        gU, gI = Ut.grad, It.grad
    return (np.array([float(tm[k].detach()) for k in ("loss", "mf", "reg")]), gU.detach().numpy(), gI.detach().numpy(),
            np.array([float(tm[k].detach()) for k in ("align", "uni_u", "uni_i")]))


valid_rows = inbatch_ref.valid_rows
zipf = inbatch_ref.zipf


def reference(U, I, users, pos, *, dtype=torch.float64, **kw):
    """dau_grads on the valid rows of a batch that may hold ids outside the tables; B stays the length of the batch."""
    keep = np.flatnonzero(valid_rows(users, pos, U.shape[0], I.shape[0]))
    return dau_grads(U, I, np.asarray(users)[keep], np.asarray(pos)[keep], dtype=dtype, B=len(users), **kw)


def tables(rng, d, nU=NU, nI=NI):
    """Rows with norms in 0.7 .. 1.3 whose directions cluster around one axis (cosine about 0.8 between two rows, as trained embeddings cluster
    around the popular items): a raw row is not its unit row, and at t = 10 the pairs of DIFFERENT rows still weigh exp(-4) against the exact 1
    of a repeated id, so every clause of the uniformity gradient stands well above the bound."""
    m = rng.standard_normal(d)
    m /= np.linalg.norm(m)

    def one(n):
        g = rng.standard_normal((n, d))
        x = 2.0 * m + g / np.linalg.norm(g, axis=1, keepdims=True)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        return (x * rng.uniform(0.7, 1.3, (n, 1))).astype(np.float32)
    return one(nU), one(nI)


def make_case(seed, d, B, *, distinct=False, grouped=False, nU=NU, nI=NI):
    """-> dict(U, I, users, pos int32 [B], nU, nI).  Positives are Zipf over the items, so equal positives occur; users distinct (a permutation),
    or drawn from 20 so that they repeat.  grouped: rows sorted by positive; otherwise shuffled as drawn."""
    rng = np.random.default_rng(seed)
    nU = max(nU, B + 5)
    U, I = tables(rng, d, nU, nI)
    users = (rng.permutation(nU)[:B] if distinct else rng.integers(0, min(20, nU), B)).astype(np.int32)
    pos = zipf(rng, B, nI).astype(np.int32)
    if grouped:
        order = np.argsort(pos, kind="stable")
        users, pos = users[order], pos[order]
    return dict(U=U, I=I, users=users, pos=pos, nU=nU, nI=nI)


# Every value of every axis with every d: B in {1, 2, T + 3, 2 T + 5} (partial row and column tiles; the column splits are more than one from
# T + 3 on), t in {2, 10}, gamma in {1, 5}, same keep | drop, any order | grouped by positive, users repeated | distinct.  Six per d, 24 cases.
#          B          t     gamma same    grouped distinct
COMBOS = ((1, 2.0, 1.0, "keep", False, False),
          (2, 10.0, 5.0, "drop", True, True),
          (T + 3, 2.0, 5.0, "drop", False, True),
          (T + 3, 10.0, 1.0, "keep", True, False),
          (2 * T + 5, 10.0, 5.0, "keep", False, False),
          (2 * T + 5, 2.0, 1.0, "drop", True, True))
CASES = tuple((d,) + c for d in DIMS for c in COMBOS)


def case_id(c):
    return "d%d-B%d-t%g-gamma%g-%s-%s-%s" % (c[0], c[1], c[2], c[3], c[4], "grouped" if c[5] else "any", "distinct" if c[6] else "rep")


def parity_case(d, B, t, gamma, same, grouped, distinct):
    """-> the case dict of make_case: the inputs of one gradient comparison, the same on the CPU and on the GPU."""
    return make_case(9000 * d + 10 * B + int(t), d, B, distinct=distinct, grouped=grouped)


def case_reference(case, dtype=torch.float64, mutant=None):
    d, B, t, gamma, same, grouped, distinct = case
    c = parity_case(*case)
    return reference(c["U"], c["I"], c["users"], c["pos"], t=t, gamma=gamma, same=same, regs=REGS, reg_div=B, dtype=dtype, mutant=mutant)


def worst(a, b):
    return max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max(), np.abs(a[2] - b[2]).max())


# ---- three whole Adam steps: d, B, lr and seed of the in-batch test's ADAM ------------------------------------------------------------------------------
ADAM = dict(d=inbatch_ref.ADAM["d"], B=inbatch_ref.ADAM["B"], lr=inbatch_ref.ADAM["lr"], seed=inbatch_ref.ADAM["seed"], t=2.0, gamma=1.0, same="keep")


def adam_case():
    """-> (case dict with the tables, [(users, pos) of step 1, 2, 3])."""
    c = make_case(ADAM["seed"], ADAM["d"], ADAM["B"])
    rng = np.random.default_rng(ADAM["seed"] + 1)
    batches = [(c["users"], c["pos"])]
    for _ in range(2):
        batches.append((rng.integers(0, 20, ADAM["B"]).astype(np.int32), zipf(rng, ADAM["B"], c["nI"]).astype(np.int32)))
    return c, batches


def adam_reference(dtype=torch.float64):
    """The three steps: dau_grads, then the project's Adam restatement -> dict(U, I, mU, vU, mI, vI), and the loss terms of every step."""
    from oracle import pda_oracle as po
    c, batches = adam_case()
    U, I = c["U"].astype(np.float64), c["I"].astype(np.float64)
    st = {k: np.zeros_like(x) for k, x in (("mU", U), ("vU", U), ("mI", I), ("vI", I))}
    terms = []
    for step, (users, pos) in enumerate(batches, 1):
        Ug, Ig = (U.astype(np.float32).astype(np.float64), I.astype(np.float32).astype(np.float64)) if dtype == torch.float32 else (U, I)
        tm, gU, gI, _ = dau_grads(Ug, Ig, users, pos, dtype=dtype, t=ADAM["t"], gamma=ADAM["gamma"], same=ADAM["same"], regs=REGS, reg_div=ADAM["B"])
        U, st["mU"], st["vU"] = po.adam_dense_decay_step(U, st["mU"], st["vU"], gU.astype(np.float64), step, ADAM["lr"])
        I, st["mI"], st["vI"] = po.adam_dense_decay_step(I, st["mI"], st["vI"], gI.astype(np.float64), step, ADAM["lr"])
        terms.append(tm)
    return dict(U=U, I=I, **st), terms
