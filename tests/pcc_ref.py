"""Restatement of the contract of include/pda_hip_pcc.h (the popularity-correlation regulariser, `--train pcc`) for the PCC tests;
it holds no test.

    pcc_pop        the popularity table of a count vector in numpy: (float)n_i, or log1p(n_i) in float64 then cast
    pcc_moments    the centred moments of (z, q) in torch float64 (or any dtype): n_v, zbar, qbar, Szz, Sqq, Szq, r
    pcc_terms      the loss of one batch: loss, mf, reg, pen, and the statistic
    pcc_grads      the same with autograd: the three loss terms, the dense gradients of both tables, the statistic
    pcc_adam       one whole train step: pcc_grads, then the project's Adam restatement (oracle.pda_oracle.adam_dense_decay_step)
    parity_case    the tables, the batch and the popularities the CPU and the GPU tests share for one (d, B)
    tolerance      the bound of a batch

Written from the contract, not from the kernel: gathers, centred moments, r, a mean of log-sigmoids, autograd.
"""
import math

import numpy as np
import torch

from ips_ref import COUNTS, DIMS, NI, NU, batch, lsig, tables       # noqa: F401  (the shapes of the IPS tests)

TOL = 1e-5
ONS = ("pos", "margin")
BATCHES = (2, 3, 7, 67, 2048)        # the float32 margin of the host suite (the GPU suite adds 1 and TPB + 3)


def pcc_pop(counts, mode="count"):
    counts = np.asarray(counts, dtype=np.int64)
    if mode == "count":
        return counts.astype(np.float32)
    if mode == "log":
        return np.log1p(counts.astype(np.float64)).astype(np.float32)
    raise ValueError(mode)


def pcc_moments(z, q):
    """z, q: 1-d tensors of one dtype over the VALID triplets -> dict of 0-d tensors; r = 0 by rule when n_v < 2 or a centred sum is not > 0."""
    n_v = z.numel()
    zero = z.new_zeros(())
    if n_v == 0:
        return dict(n_v=0, zbar=zero, qbar=zero, Szz=zero, Sqq=zero, Szq=zero, r=zero, by_rule=True)
    zbar, qbar = z.mean(), q.mean()
    dz, dq = z - zbar, q - qbar
    Szz, Sqq, Szq = (dz * dz).sum(), (dq * dq).sum(), (dz * dq).sum()
    by_rule = not (n_v >= 2 and float(Szz.detach()) > 0 and float(Sqq.detach()) > 0)
    r = zero if by_rule else Szq / torch.sqrt(Szz * Sqq)
    return dict(n_v=n_v, zbar=zbar, qbar=qbar, Szz=Szz, Sqq=Sqq, Szq=Szq, r=r, by_rule=by_rule)


def pcc_scores(U, I, users, pos, neg, on):
    u, p, n = U[users], I[pos], I[neg]
    sp, sn = (u * p).sum(1), (u * n).sum(1)
    return sp, sn, (sp if on == "pos" else sp - sn)


def pcc_terms(U, I, users, pos, neg, pop, *, gamma, on, regs, reg_div, B=None):
    """-> dict(loss, mf, reg, pen, stat) -- users / pos / neg: int64 tensors of the batch's VALID triplets; B: the batch size the mean divides by
    (more than len(users) when the kernel skipped a triplet); pop: tensor [n_items] of U's dtype."""
    B = len(users) if B is None else B
    u, p, n = U[users], I[pos], I[neg]
    sp, sn, z = pcc_scores(U, I, users, pos, neg, on)
    st = pcc_moments(z, pop[pos])
    bpr = -lsig(sp - sn).sum() / B
    pen = gamma * st["r"] ** 2
    mf = bpr + pen
    reg = regs * 0.5 * ((u ** 2).sum() + (p ** 2).sum() + (n ** 2).sum()) / reg_div        # tf.nn.l2_loss = sum(x^2) / 2
    return dict(loss=mf + reg, mf=mf, reg=reg, pen=pen, stat=st)


def stat_vector(st):
    """The statistic as the kernel lays it out: float64 [8] = (n_v, zbar, qbar, Szz, Sqq, Szq, r, 0)."""
    return np.array([float(torch.as_tensor(st[k]).detach()) for k in ("n_v", "zbar", "qbar", "Szz", "Sqq", "Szq", "r")] + [0.0])


def pcc_grads(U, I, users, pos, neg, pop, dtype=torch.float64, **kw):
    """numpy in, numpy out: (terms float64 [3] = loss, mf, reg; gU; gI; stat float64 [8]), computed in `dtype` (pop: the float32 table the
    kernel reads)."""
    Ut = torch.tensor(np.asarray(U), dtype=dtype, requires_grad=True)
    It = torch.tensor(np.asarray(I), dtype=dtype, requires_grad=True)
    ix = [torch.as_tensor(np.asarray(a, dtype=np.int64)) for a in (users, pos, neg)]
    t = pcc_terms(Ut, It, *ix, torch.tensor(np.asarray(pop), dtype=dtype), **kw)
    t["loss"].backward()
    return (np.array([float(t[k].detach()) for k in ("loss", "mf", "reg")]), Ut.grad.numpy().astype(np.float64),
            It.grad.numpy().astype(np.float64), stat_vector(t["stat"]))


def pcc_adam(U, I, state, t, lr, users, pos, neg, pop, **kw):
    """One train step in float64: -> (U1, I1, state, terms, stat).  state = dict(mU, vU, mI, vI) or None."""
    from oracle import pda_oracle as po
    terms, gU, gI, stat = pcc_grads(U, I, users, pos, neg, pop, **kw)
    if state is None:
        state = {k: np.zeros_like(x, dtype=np.float64) for k, x in (("mU", U), ("vU", U), ("mI", I), ("vI", I))}
    U1, mU, vU = po.adam_dense_decay_step(np.asarray(U, dtype=np.float64), state["mU"], state["vU"], gU, t, lr)
    I1, mI, vI = po.adam_dense_decay_step(np.asarray(I, dtype=np.float64), state["mI"], state["vI"], gI, t, lr)
    return U1, I1, dict(mU=mU, vU=vU, mI=mI, vI=vI), terms, stat


def parity_case(d, B):
    """-> (U, I, (users, pos, neg), pop float32): the inputs of one gradient comparison, the same on the CPU and on the GPU."""
    rng = np.random.default_rng(1000 * d + B)
    U, I = tables(rng, d)
    return U, I, batch(rng, B), pcc_pop(COUNTS)


def tolerance(gamma, stat):
    """1e-5 max(1, 4 gamma / sqrt(Szz)), Szz from the float64 restatement (stat: its float64 [8]); 1e-5 when r = 0 by rule.  |r| <= 1 and both
    standardised deviations are at most 1, so |d pen / d z_t| <= 4 gamma / sqrt(Szz), and every gradient entry is that coefficient times a
    quantity the BPR tests hold to 1e-5."""
    n_v, Szz, Sqq = stat[0], stat[3], stat[4]
    if not (n_v >= 2 and Szz > 0 and Sqq > 0):
        return TOL
    return TOL * max(1.0, 4.0 * float(gamma) / math.sqrt(Szz))
