"""Restatement of the IPS contract of include/pda_hip_ips.h for the IPS tests; it holds no test.

    ips_weights    the weights of a count vector in numpy: float64, clipped, then cast to float32
    ips_terms      the loss of one batch in torch float64 (or any dtype): loss, mf, reg
    ips_grads      the same with autograd: the three loss terms and the dense gradients of both tables
    ips_adam       one whole train step: ips_grads, then the project's Adam restatement (oracle.pda_oracle.adam_dense_decay_step)
    parity_case    the tables, the batch and the weights the CPU and the GPU tests share for one (d, B, variant)
    tolerance      the bound of a variant on a batch

Written from the contract, not from the kernel: gathers, a weighted mean of log-sigmoids, autograd.
"""
import numpy as np
import torch

NU, NI = 50, 40
TOL = 1e-5
# item i has 16 / 2^(i mod 5) train interactions: the unclipped weights are exactly 1, 2, 4, 8, 16
COUNTS = (16 // 2 ** (np.arange(NI) % 5)).astype(np.int64)
VARIANTS = {"plain": dict(clip=0.0, norm=False), "clip": dict(clip=4.0, norm=False), "clip_norm": dict(clip=4.0, norm=True)}
DIMS = (32, 64, 128, 256)
BATCHES = (1, 7, 2048)


def ips_weights(counts, clip=0.0):
    """p_i = max(n_i, 1) / max_j n_j and w_i = 1 / p_i in float64, min(w_i, clip) for clip > 0 -> (float64 weights, their float32 cast)."""
    counts = np.asarray(counts, dtype=np.int64)
    p = np.maximum(counts, 1).astype(np.float64) / np.float64(max(int(counts.max()), 1))
    w = 1.0 / p
    if clip > 0:
        w = np.minimum(w, np.float64(clip))
    return w, w.astype(np.float32)


def lsig(x):
    return torch.log(torch.sigmoid(x) + 1e-10)


def ips_terms(U, I, users, pos, neg, ipw, *, norm, regs, reg_div, B=None):
    """-> dict(loss, mf, reg) of 0-d tensors of U's dtype.  users / pos / neg: int64 tensors of the batch's VALID triplets; B: the batch size the
    unnormalised mean divides by (more than len(users) when the kernel skipped a triplet); ipw: tensor [n_items] of U's dtype."""
    B = len(users) if B is None else B
    u, p, n = U[users], I[pos], I[neg]
    x = (u * p).sum(1) - (u * n).sum(1)
    w = ipw[pos]
    mf = -(w * lsig(x)).sum() / (w.sum() if norm else B)
    reg = regs * 0.5 * ((u ** 2).sum() + (p ** 2).sum() + (n ** 2).sum()) / reg_div        # tf.nn.l2_loss = sum(x^2) / 2
    return dict(loss=mf + reg, mf=mf, reg=reg)


def ips_grads(U, I, users, pos, neg, ipw, dtype=torch.float64, **kw):
    """numpy in, numpy out: (terms float64 [3] = loss, mf, reg; gU; gI), computed in `dtype` (ipw: the float32 weights the kernel reads)."""
    Ut = torch.tensor(np.asarray(U), dtype=dtype, requires_grad=True)
    It = torch.tensor(np.asarray(I), dtype=dtype, requires_grad=True)
    ix = [torch.as_tensor(np.asarray(a, dtype=np.int64)) for a in (users, pos, neg)]
    t = ips_terms(Ut, It, *ix, torch.tensor(np.asarray(ipw), dtype=dtype), **kw)
    t["loss"].backward()
    return np.array([float(t[k].detach()) for k in ("loss", "mf", "reg")]), Ut.grad.numpy(), It.grad.numpy()


def ips_adam(U, I, state, t, lr, users, pos, neg, ipw, **kw):
    """One train step in float64: -> (U1, I1, state, terms).  state = dict(mU, vU, mI, vI) or None."""
    from oracle import pda_oracle as po
    terms, gU, gI = ips_grads(U, I, users, pos, neg, ipw, **kw)
    if state is None:
        state = {k: np.zeros_like(x, dtype=np.float64) for k, x in (("mU", U), ("vU", U), ("mI", I), ("vI", I))}
    U1, mU, vU = po.adam_dense_decay_step(np.asarray(U, dtype=np.float64), state["mU"], state["vU"], gU, t, lr)
    I1, mI, vI = po.adam_dense_decay_step(np.asarray(I, dtype=np.float64), state["mI"], state["vI"], gI, t, lr)
    return U1, I1, dict(mU=mU, vU=vU, mI=mI, vI=vI), terms


def tables(rng, d, nU=NU, nI=NI):
    return (rng.standard_normal((nU, d)) * 0.3).astype(np.float32), (rng.standard_normal((nI, d)) * 0.3).astype(np.float32)


def batch(rng, B, nU=NU, nI=NI):
    return tuple(rng.integers(0, n, B).astype(np.int32) for n in (nU, nI, nI))


def parity_case(d, B, variant):
    """-> (U, I, (users, pos, neg), ipw float32, norm): the inputs of one gradient comparison, the same on the CPU and on the GPU."""
    rng = np.random.default_rng(1000 * d + B)
    U, I = tables(rng, d)
    b = batch(rng, B)
    v = VARIANTS[variant]
    return U, I, b, ips_weights(COUNTS, v["clip"])[1], v["norm"]


def tolerance(ipw, pos, norm):
    """1e-5 for the self-normalised variant; 1e-5 max(1, w_max) for the unnormalised ones, w_max the largest weight in the batch: every term is
    w_t times a quantity the BPR and DICE tests hold to 1e-5."""
    return TOL if norm else TOL * max(1.0, float(np.asarray(ipw)[np.asarray(pos)].max()))
