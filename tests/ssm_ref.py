"""Restatement of the sampled-softmax contract of include/pda_hip_ssm.h for the SSM tests; it holds no test.

    ssm_terms      the loss of one batch in torch float64 (or any dtype): loss, mf, reg -- gathers, logsumexp; `mutant` breaks one clause of it
    ssm_grads      the same with autograd: the three loss terms and the dense gradients of both tables
    ssm_adam       one whole train step: ssm_grads, then the project's Adam restatement (oracle.pda_oracle.adam_dense_decay_step)
    ssm_sample     the sampler in numpy on the draw / bounded / feistel_perm of tests/sampler_ref.py
    CASES          the (d, N, norm, tau, one_row, grouped, distinct) combinations of the gradient comparison; parity_case builds their inputs
    ADAM_STEPS     the inputs of the three whole Adam steps; adam_steps_reference runs them through ssm_adam
    tolerance      the bound of a case

Written from the contract, not from the kernel.
"""
import numpy as np
import torch

import sampler_ref as sr

NU, NI = 300, 200
TOL = 1e-5
REGS = 1e-2
DIMS = (32, 64, 128, 256)
MUTANTS = ("drop_pos", "no_tau_grad", "no_proj", "reg_distinct")

# Every value of every axis with every d: N in {1, 2, 7, 64, 256}, norm in {0, 1}, tau in {1, 0.1}, B in {1, TPB + 3}, any order | grouped by
# positive, users repeated | distinct (PDA_UPD_USERS_DISTINCT).  Six combinations per d, 24 cases.
#          N  norm  tau  one_row grouped distinct
COMBOS = ((1, 0, 1.0, True, False, False),
          (2, 1, 0.1, False, True, True),
          (7, 0, 0.1, False, False, True),
          (64, 1, 1.0, False, True, False),
          (256, 1, 0.1, False, False, False),
          (256, 0, 1.0, True, True, True))
CASES = tuple((d,) + c for d in DIMS for c in COMBOS)


def tpb(d):
    """Rows per workgroup of the step kernels: 512 threads, d / 4 lanes per row."""
    return 512 // (d // 4)


def tolerance(tau):
    """1e-5 max(1, 1 / tau) absolute on every loss term and gradient element: the project's figure for quantities of this size (the BPR, DICE and
    IPS tests hold theirs to 1e-5) times 1 / tau, the factor every logit and every gradient coefficient c_k carries.  tests/test_ssm_host.py
    evaluates the contract in float32 on the inputs of the GPU tests and finds it inside a quarter of this against float64."""
    return TOL * max(1.0, 1.0 / float(tau))


def _unit(x):
    return x / torch.linalg.vector_norm(x, dim=-1, keepdim=True).clamp_min(1e-12)


def ssm_terms(U, I, users, pos, negs, *, tau, norm, regs, reg_div, B=None, mutant=None):
    """-> dict(loss, mf, reg) of 0-d tensors of U's dtype.  users / pos int64 [R], negs int64 [R, N]: the batch's VALID rows; B: the batch size
    the mean divides by (more than R when the kernel skipped a row).  mutant: one of MUTANTS -- the contract with one clause broken."""
    B = len(users) if B is None else B
    u, items = U[users], torch.cat([I[pos][:, None, :], I[negs]], dim=1)              # [R, d], [R, N + 1, d]
    uq, iq = u, items
    if norm:
        if mutant == "no_proj":        # x / |x| with |x| a constant: the gradient loses its projection term
            uq = u / torch.linalg.vector_norm(u, dim=-1, keepdim=True).clamp_min(1e-12).detach()
            iq = items / torch.linalg.vector_norm(items, dim=-1, keepdim=True).clamp_min(1e-12).detach()
        else:
            uq, iq = _unit(u), _unit(items)
    raw = torch.einsum("rd,rkd->rk", uq, iq)
    s = raw / tau
    if mutant == "no_tau_grad":        # the value of raw / tau with the gradient of raw
        s = (raw / tau).detach() + (raw - raw.detach())
    lse = torch.logsumexp(s[:, 1:] if mutant == "drop_pos" else s, dim=1)
    mf = (lse - s[:, 0]).sum() / B
    if mutant == "reg_distinct":       # every distinct item of the batch once
        seen = torch.unique(torch.cat([pos.reshape(-1), negs.reshape(-1)]))
        reg = regs * 0.5 * ((u ** 2).sum() + (I[seen] ** 2).sum()) / reg_div
    else:
        reg = regs * 0.5 * ((u ** 2).sum() + (items ** 2).sum()) / reg_div             # tf.nn.l2_loss = sum(x^2) / 2, per occurrence
    return dict(loss=mf + reg, mf=mf, reg=reg)


def ssm_grads(U, I, users, pos, negs, dtype=torch.float64, **kw):
    """numpy in, numpy out: (terms float64 [3] = loss, mf, reg; gU; gI), computed in `dtype`."""
    Ut = torch.tensor(np.asarray(U), dtype=dtype, requires_grad=True)
    It = torch.tensor(np.asarray(I), dtype=dtype, requires_grad=True)
    ix = [torch.as_tensor(np.asarray(a, dtype=np.int64)) for a in (users, pos, negs)]
    t = ssm_terms(Ut, It, *ix, **kw)
    t["loss"].backward()
    return np.array([float(t[k].detach()) for k in ("loss", "mf", "reg")]), Ut.grad.numpy(), It.grad.numpy()


def ssm_adam(U, I, state, t, lr, users, pos, negs, dtype=torch.float64, **kw):
    """One train step in float64: -> (U1, I1, state, terms).  state = dict(mU, vU, mI, vI) or None.  dtype = torch.float32: the gradients are
    taken in float32 on the tables rounded to float32 (what a float32 kernel can know), the update stays float64."""
    from oracle import pda_oracle as po
    if dtype == torch.float32:
        U, I = np.asarray(U, dtype=np.float32).astype(np.float64), np.asarray(I, dtype=np.float32).astype(np.float64)
    terms, gU, gI = ssm_grads(U, I, users, pos, negs, dtype=dtype, **kw)
    gU, gI = gU.astype(np.float64), gI.astype(np.float64)
    if state is None:
        state = {k: np.zeros_like(x, dtype=np.float64) for k, x in (("mU", U), ("vU", U), ("mI", I), ("vI", I))}
    U1, mU, vU = po.adam_dense_decay_step(np.asarray(U, dtype=np.float64), state["mU"], state["vU"], gU, t, lr)
    I1, mI, vI = po.adam_dense_decay_step(np.asarray(I, dtype=np.float64), state["mI"], state["vI"], gI, t, lr)
    return U1, I1, dict(mU=mU, vU=vU, mI=mI, vI=vI), terms


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def tables(rng, d, nU=NU, nI=NI):
    """Rows of the same length whatever d (std 0.3 sqrt(32 / d) per element: |row| ~ 1.7, u . i ~ 0.5), so the logits are of one size across d."""
    sc = 0.3 * np.sqrt(32.0 / d)
    return (rng.standard_normal((nU, d)) * sc).astype(np.float32), (rng.standard_normal((nI, d)) * sc).astype(np.float32)


def batch(rng, B, N, *, distinct=False, grouped=False, nU=NU, nI=NI):
    """users / pos int32 [B], negs int32 [B, N].  A hot positive -- the LAST item, so that a batch sorted by positive ends with its run -- fills a
    tenth of the batch (at least 5 rows of a batch of more than 5: the run crosses the boundary of a workgroup of B - 3 rows); the negatives
    come from all nI items, so they repeat inside a row (N > nI for certain) and across rows, and may equal the row's positive.  Users: distinct
    (a permutation), or drawn from 20 so that they repeat.  grouped: rows sorted by positive; otherwise shuffled as drawn."""
    users = (rng.permutation(nU)[:B] if distinct else rng.integers(0, min(20, nU), B)).astype(np.int32)
    pos = rng.integers(0, nI - 1, B).astype(np.int32)
    hot = min(B, max(5, B // 10 + 1)) if B > 1 else 0
    pos[rng.permutation(B)[:hot]] = nI - 1
    negs = rng.integers(0, nI, (B, N)).astype(np.int32)
    if grouped:
        order = np.argsort(pos, kind="stable")
        users, pos, negs = users[order], pos[order], np.ascontiguousarray(negs[order])
    return users, pos, negs


def parity_case(d, N, norm, tau, one_row, grouped, distinct):
    """-> (U, I, (users, pos, negs), B): the inputs of one gradient comparison, the same on the CPU and on the GPU."""
    B = 1 if one_row else tpb(d) + 3
    rng = np.random.default_rng(100000 * d + 100 * N + 10 * norm + int(one_row))
    U, I = tables(rng, d)
    return U, I, batch(rng, B, N, distinct=distinct, grouped=grouped), B


# The three whole Adam steps of the GPU suite: d, B, N, the learning rate, tau and the seed of tables and batches.  lr is the trainer's default
# rate: TF's Adam turns a gradient element g into a step of lr_t m / (sqrt(v) + 1e-8), which near g = 0 changes by lr_t 1e7 per unit of g -- an
# element whose gradient lies within some 1e-6 of zero moves by lr_t times O(1) for an error of 1e-7 in g, whatever computes it.  At lr = 1e-3 the
# float32 restatement of these steps stays within a quarter of the 1e-5 the tables are held to (tests/test_ssm_host.py); at 1e-2 it does not.
ADAM_STEPS = dict(d=32, B=67, N=7, lr=1e-3, tau=0.1, seed=33)


def adam_steps_case():
    """-> (U, I, [batch of step 1, 2, 3])."""
    c = ADAM_STEPS
    rng = np.random.default_rng(c["seed"])
    U, I = tables(rng, c["d"])
    return U, I, [batch(rng, c["B"], c["N"]) for _ in range(3)]


def adam_steps_reference(norm, dtype=torch.float64):
    """The three steps through ssm_adam -> dict(U, I, mU, vU, mI, vI), and the loss terms of every step."""
    c = ADAM_STEPS
    U, I, batches = adam_steps_case()
    Ur, Ir, state, terms = U.astype(np.float64), I.astype(np.float64), None, []
    for t, b in enumerate(batches, 1):
        Ur, Ir, state, tm = ssm_adam(Ur, Ir, state, t, c["lr"], *b, dtype=dtype, tau=c["tau"], norm=norm, regs=REGS, reg_div=c["B"])
        terms.append(tm)
    return dict(U=Ur, I=Ir, **state), terms


# ---- the sampler -------------------------------------------------------------------------------------------------------------------------------
def ssm_sample(seed, step, B, N, indptr, indices, *, user_pool=None, n_pool=0, users=None, neg_range):
    """pda_ssm_sample for one batch: users and positives are sampler_ref.sample's; negative j of row r tries the draws 16 + 4096 j + a,
    a = 0 .. 4095, until one is not a train item of the user (the last one stays).  -> dict(users, pos, negs [B, N], rejections [B, N])."""
    base = sr.sample(seed, step, B, indptr, indices, user_pool=user_pool, n_pool=n_pool, users=users, neg_range=neg_range)
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32)
    u = np.repeat(base["users"].astype(np.int64), N)
    r, j = np.repeat(np.arange(B, dtype=np.int64), N), np.tile(np.arange(N, dtype=np.int64), B)
    b, e = indptr[u], indptr[u + 1]
    lo, hi = int(neg_range[0]), int(neg_range[1])
    neg = np.full(B * N, lo, dtype=np.int64)
    rej = np.zeros(B * N, dtype=np.int64)
    act = np.arange(B * N)
    for a in range(sr.REJECT_CAP):
        neg[act] = lo + sr.bounded(sr.draw(seed & sr.MASK, step, r[act], 16 + 4096 * j[act] + a), hi - lo).astype(np.int64)
        act = act[sr._in_row(indices, b[act], e[act], neg[act])]
        if not act.size:
            break
        rej[act] += 1
    return dict(users=base["users"], pos=base["pos"], negs=neg.astype(np.int32).reshape(B, N), rejections=rej.reshape(B, N), neg0=base["neg"])
