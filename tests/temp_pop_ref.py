"""Float64 numpy restatement of BPRMF(t)-pop (MF/model_api.py:300-416) for the temp_pop tests: forward pass, loss, closed-form gradients
(quirk 1: the user bias only for stage-0 triplets), TF-1.14 dense-decay Adam, and the bias head of the evaluation."""
import numpy as np

B1, B2, EPS = 0.9, 0.999, 1e-8


def forward_grads(U, I, bu, Cm, users, pos, neg, temps, regs, batch_size):
    """-> ((loss, mf_loss, reg_loss), (gU, gI, gbu, gC)) in float64; duplicates summed."""
    U, I, bu, Cm = (np.asarray(x, dtype=np.float64) for x in (U, I, bu, Cm))
    users, pos, neg, temps = (np.asarray(x).astype(np.int64) for x in (users, pos, neg, temps))
    T = Cm.shape[1] - 1
    B = len(users)
    ue, pe, ne = U[users], I[pos], I[neg]
    bt = np.where(temps == 0, bu[users, 0], 0.0)
    ub = bt + 1.0
    pb = Cm[pos, T] + Cm[pos, temps]
    nb = Cm[neg, T] + Cm[neg, temps]
    x = ub * pb + (ue * pe).sum(1) - (ub * nb + (ue * ne).sum(1))
    sg = 1.0 / (1.0 + np.exp(-x))
    mf = -np.mean(np.log(sg + 1e-10))
    reg = regs * 0.5 * ((ue ** 2).sum() + (pe ** 2).sum() + (ne ** 2).sum()) / batch_size
    gg = -(1.0 / B) * sg * (1.0 - sg) / (sg + 1e-10)
    c = regs / batch_size
    gU, gI, gbu, gC = np.zeros_like(U), np.zeros_like(I), np.zeros_like(bu), np.zeros_like(Cm)
    np.add.at(gU, users, gg[:, None] * (pe - ne) + c * ue)
    np.add.at(gI, pos, gg[:, None] * ue + c * pe)
    np.add.at(gI, neg, -gg[:, None] * ue + c * ne)
    s0 = temps == 0
    np.add.at(gbu[:, 0], users[s0], (gg * (pb - nb))[s0])
    gb = gg * ub
    np.add.at(gC, (pos, np.full(B, T)), gb)
    np.add.at(gC, (pos, temps), gb)
    np.add.at(gC, (neg, np.full(B, T)), -gb)
    np.add.at(gC, (neg, temps), -gb)
    return (mf + reg, mf, reg), (gU, gI, gbu, gC)


def adam_steps(tabs, batches, regs, batch_size, lr):
    """Dense-decay Adam over the four tables for a list of (users, pos, neg, temps) batches -> (tables, losses), float64."""
    m = [np.zeros_like(x) for x in tabs]
    v = [np.zeros_like(x) for x in tabs]
    losses = []
    for step, (u, p, n, t) in enumerate(batches, 1):
        loss, grads = forward_grads(*tabs, u, p, n, t, regs, batch_size)
        losses.append(loss)
        lr_t = lr * np.sqrt(1 - B2 ** step) / (1 - B1 ** step)
        for k, g in enumerate(grads):
            m[k] = B1 * m[k] + (1 - B1) * g
            v[k] = B2 * v[k] + (1 - B2) * g * g
            tabs[k] = tabs[k] - lr_t * m[k] / (np.sqrt(v[k]) + EPS)
    return tabs, losses


def item_beta(Cm):
    """beta_i = fl(C[i, T-1] + C[i, T]) in float32."""
    Cm = np.asarray(Cm, dtype=np.float32)
    T = Cm.shape[1] - 1
    return (Cm[:, T - 1] + Cm[:, T]).astype(np.float32)


def scores_bias(s, alpha, beta):
    """h = fl(s + fl(alpha_u beta_i)), float32: s the exact fp32 chain, alpha per row, beta per column."""
    s = np.asarray(s, dtype=np.float32)
    ab = (np.asarray(alpha, dtype=np.float32)[:, None] * np.asarray(beta, dtype=np.float32)[None, :]).astype(np.float32)
    return (s + ab).astype(np.float32)
