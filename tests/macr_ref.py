"""Restatement of the MACR contract of include/pda_hip_macr.h for the MACR tests; it holds no test.

    macr_terms       the loss of one batch in torch float64 (or any dtype): loss, L_O, L_I, L_U, reg
    macr_grads       the same with autograd: the five loss terms and the gradients of both tables and of the two branch vectors
    macr_adam        one whole train step: macr_grads, then the project's Adam restatement (oracle.pda_oracle.adam_dense_decay_step)
    contract_lists   the ranking contract in numpy float32 on given chain values s: top_k(fl(s + fl(-c sig)) + mask), ties by the lower id
    model_values     the model's (y - c) s_i in float64, and the rounding bound of the contract against it
    parity_case      the tables, the branch vectors and the batch the CPU and the GPU tests share for one (d, B, kind)
    list_case        the inputs of one list comparison
    tolerance        the bound of a quantity

Written from the contract, not from the kernel: gathers, sigmoids, logs, autograd.
"""
import numpy as np
import torch

NU, NI = 64, 40
TOL = 1e-5
DIMS = (32, 64, 128, 256)
BATCHES = (1, 7, 2048)
WEIGHTS = ((0.0, 0.0), (1e-3, 1e-3), (0.5, 0.25))         # (alpha, beta)
KINDS = ("xavier", "spread")
REGS = 1e-2
EPS32 = 2.0 ** -24
C_GRID = tuple(float(c) for c in np.linspace(-1.0, 1.0, 20))
LIST_CS = (-1.0, 0.0, 0.37, 1.0)
LIST_SHAPES = ((200, 4096), (200, 300))
LIST_DIMS = (64, 256)
LIST_KS = (1, 50, 54)


def tolerance(what="loss"):
    """1e-5 absolute on every loss term and on every gradient element, gW included: the project's figure for quantities of this size.
    tests/test_macr_host.py shows that the float32 restatement stays inside a quarter of it on the inputs of the GPU tests (gW, which sums
    B terms, included: 4.1e-7 at most on a loss term, 8e-8 on a table gradient, 1.2e-8 on gW)."""
    return TOL


def macr_terms(U, I, w_item, w_user, users, pos, neg, *, alpha, beta, regs, reg_div, B=None):
    """-> dict(loss, lo, li, lu, reg) of 0-d tensors of U's dtype.  users / pos / neg: int64 tensors of the batch's VALID triplets; B: the batch size
    the means divide by (more than len(users) when the kernel skipped a triplet); w_item / w_user: tensors [d]."""
    B = len(users) if B is None else B
    u, p, n = U[users], I[pos], I[neg]
    yp, yn = (u * p).sum(1), (u * n).sum(1)
    sp, sn, su = torch.sigmoid(p @ w_item), torch.sigmoid(n @ w_item), torch.sigmoid(u @ w_user)
    ap, an = yp * sp * su, yn * sn * su

    def bce(s, z):
        return (-torch.log(s + 1e-10) - torch.log(1 - z + 1e-10)).sum() / B

    lo, li, lu = bce(torch.sigmoid(ap), torch.sigmoid(an)), bce(sp, sn), bce(su, su)
    reg = regs * 0.5 * ((u ** 2).sum() + (p ** 2).sum() + (n ** 2).sum()) / reg_div        # tf.nn.l2_loss = sum(x^2) / 2
    return dict(loss=lo + alpha * li + beta * lu + reg, lo=lo, li=li, lu=lu, reg=reg)


TERMS = ("loss", "lo", "li", "lu", "reg")


def macr_grads(U, I, w_item, w_user, users, pos, neg, dtype=torch.float64, **kw):
    """numpy in, numpy out: (terms float64 [5]; gU; gI; gW [2, d] = the gradients of w_item, w_user), computed in `dtype`."""
    leaves = [torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True) for x in (U, I, np.ravel(w_item), np.ravel(w_user))]
    ix = [torch.as_tensor(np.asarray(a, dtype=np.int64)) for a in (users, pos, neg)]
    t = macr_terms(*leaves, *ix, **kw)
    t["loss"].backward()
    g = [np.zeros(x.shape) if x.grad is None else x.grad.numpy() for x in leaves]
    return np.array([float(t[k].detach()) for k in TERMS]), g[0], g[1], np.stack([g[2], g[3]])


def macr_adam(U, I, W, state, t, lr, users, pos, neg, **kw):
    """One train step in float64: -> (U1, I1, W1, state, terms).  W float64 [2, d] = (w_item, w_user); state = dict(mU, vU, mI, vI, mW, vW) or None."""
    from oracle import pda_oracle as po
    terms, gU, gI, gW = macr_grads(U, I, W[0], W[1], users, pos, neg, **kw)
    if state is None:
        state = {k + n: np.zeros_like(x, dtype=np.float64) for n, x in (("U", U), ("I", I), ("W", W)) for k in "mv"}
    out = {}
    new = []
    for n, x, g in (("U", U, gU), ("I", I, gI), ("W", W, gW)):
        x1, m, v = po.adam_dense_decay_step(np.asarray(x, dtype=np.float64), state["m" + n], state["v" + n], g, t, lr)
        new.append(x1)
        out["m" + n], out["v" + n] = m, v
    return new[0], new[1], new[2], out, terms


# ---- the inputs of the gradient comparisons ----------------------------------------------------------------------------------------------------
def xavier(rng, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, (fan_in, fan_out)).astype(np.float32)


def tables(rng, d, nU=NU, nI=NI):
    return xavier(rng, nU, d), xavier(rng, nI, d)


def branches(rng, d):
    return xavier(rng, d, 1).ravel(), xavier(rng, d, 1).ravel()


def batch(rng, B, nU=NU, nI=NI):
    return tuple(rng.integers(0, n, B).astype(np.int32) for n in (nU, nI, nI))


def parity_case(d, B, kind="xavier"):
    """-> (U, I, w_item, w_user, (users, pos, neg)): Xavier-scale tables and branch vectors; kind "spread" scales the branch vectors so that the
    largest |row . w| of each table is logit(0.95): s_p, s_n and s_u then spread over 0.05 .. 0.95 and the branch gradients are not trivially
    equal."""
    rng = np.random.default_rng(1000 * d + B)
    U, I = tables(rng, d)
    wi, wu = branches(rng, d)
    if kind == "spread":
        top = np.log(0.95 / 0.05)
        wi = (wi * (top / np.abs(I.astype(np.float64) @ wi).max())).astype(np.float32)
        wu = (wu * (top / np.abs(U.astype(np.float64) @ wu).max())).astype(np.float32)
    return U, I, wi, wu, batch(rng, B)


# ---- the ranking -----------------------------------------------------------------------------------------------------------------------------------
def arg_topk(h, K):
    """Row-wise top-K of a matrix, best first, ties (and -inf) by the lower column: what tf.nn.top_k returns."""
    return np.argsort(-h, axis=1, kind="stable")[:, :K].astype(np.int32)


def contract_lists(s, sig, c, K, hist_rows):
    """The contract of a MACR list in numpy float32: s float32 [rows, n_items] the exact fp32 chain of u . J_i, sig float32 [n_items];
    h = fl(s + fl(-c sig)), the row's history worth -inf, top-K with ties by the lower item id.  -> (ids int32 [rows, K], h)."""
    beta = (np.float32(-c) * np.asarray(sig, dtype=np.float32)).astype(np.float32)
    h = (np.asarray(s, dtype=np.float32) + beta[None, :]).astype(np.float32)
    for r, items in enumerate(hist_rows):
        h[r, items] = -np.inf
    return arg_topk(h, K), h


def model_values(U, I, w_item, users, c, s_u=None):
    """The model's ranking value in float64 from the float32 parameters: (y_ui - c) s_i [s_u], float64 [len(users), n_items]."""
    U64, I64 = np.asarray(U, dtype=np.float64)[users], np.asarray(I, dtype=np.float64)
    v = (U64 @ I64.T - c) * (1.0 / (1.0 + np.exp(-(I64 @ np.asarray(w_item, dtype=np.float64)))))[None, :]
    return v if s_u is None else v * s_u[:, None]


def rounding_bound(U, I, w_item, users, c):
    """E float64 [len(users), n_items]: a bound on |h - v|, h the contract's float32 value fl(chain(u . J_i) + fl(-c sig_i)) and v the float64
    (y - c) s_i, with eps = 2^-24, d the row width, A = sum_k |u_k I_ik| >= |y|, s = s_i:
        |sig - s|          <= ds = eps (0.25 (d + 1) sum_k |I_ik w_k| + 4)     the float32 row dot under a slope of at most 1/4, exp, add, divide
        |chain(u.J) - sig y| <= (d + 2) eps A sig                              J rounded once per element, d products and sums
        |fl(-c sig) + c sig| <= eps |c| sig,   the last sum: eps |h|
        E = (|y| + |c|) ds + 1.01 eps ((d + 2) A s + |c| s + |v|)
    A list built from h can therefore not hold an item whose v lies more than 2 E below the K-th largest v of its row."""
    U64, I64, w = np.asarray(U, dtype=np.float64)[users], np.asarray(I, dtype=np.float64), np.asarray(w_item, dtype=np.float64)
    d = I64.shape[1]
    y, A = U64 @ I64.T, np.abs(U64) @ np.abs(I64).T
    s = 1.0 / (1.0 + np.exp(-(I64 @ w)))
    ds = EPS32 * (0.25 * (d + 1) * (np.abs(I64) @ np.abs(w)) + 4.0)
    v = (y - c) * s[None, :]
    return (np.abs(y) + abs(c)) * ds[None, :] + 1.01 * EPS32 * ((d + 2) * A * s[None, :] + abs(c) * s[None, :] + np.abs(v))


def list_case(n_users, n_items, d):
    """-> (U [n_users, d], I [n_items, d], w_item [d], users int32 [n_users], hist_rows): seeded inputs whose float64 lists are separated by far
    more than the rounding bound.  Random dense tables cannot be: the bound is about 2 d 2^-24 |y|, and the top 54 of 4 096 random values lie
    closer than that somewhere in every other row.  So the items lie along one dense direction h (|h| = 1, every entry +-1 / sqrt(d)):
    I_i = g_i h, u = t_u h, w_item = 0.16 h, plus a relative jitter of 1e-4 on every entry so that all products round.  Then y = t_u g_i and
    s_i = sigmoid(0.16 g_i) in 0.38 .. 0.62, and for 0.8 <= |t_u| <= 1.5, |g| <= 3, |c| <= 1 the value (t g - c) s(g) is strictly monotone in g
    (its slope is s [0.16 (1 - s) (t g - c) + t], of the sign of t).  g: 100 values spaced 0.015 at either end (where every list comes from: a
    value step of at least 0.38 x 0.46 x 0.015 = 2.6e-3), the rest packed into -1.2 .. 1.2; item ids are a random permutation of that order.
    The history holds 0 .. 30 random items per user; user 0 keeps only 40 unlisted items (fewer than K = 50 and 54), all from the two ends."""
    rng = np.random.default_rng(7 * n_items + d)
    h = rng.choice([-1.0, 1.0], d) / np.sqrt(d)
    ends = 0.015 * np.arange(100)
    g = np.concatenate([-3.0 + ends, np.linspace(-1.2, 1.2, n_items - 200), 3.0 - ends[::-1]])
    perm = rng.permutation(n_items)
    I = np.empty((n_items, d))
    I[perm] = g[:, None] * h[None, :]
    t = rng.uniform(0.8, 1.5, n_users) * rng.choice([-1.0, 1.0], n_users)
    U = t[:, None] * h[None, :]
    I, U = I * (1 + 1e-4 * rng.standard_normal(I.shape)), U * (1 + 1e-4 * rng.standard_normal(U.shape))
    w = 0.16 * h * (1 + 1e-4 * rng.standard_normal(d))
    hist = [np.unique(rng.integers(0, n_items, rng.integers(0, 31))) for _ in range(n_users)]
    keep = np.concatenate([perm[:20], perm[-20:]])
    hist[0] = np.setdiff1d(np.arange(n_items), keep)
    return U.astype(np.float32), I.astype(np.float32), w.astype(np.float32), np.arange(n_users, dtype=np.int32), hist


def close_rows(v, E, K, hist_rows):
    """The rows whose float64 list (the K best unlisted values) holds two adjacent values closer than the row's bound 2 max_i E."""
    bad = []
    for r, items in enumerate(hist_rows):
        x = np.delete(v[r], items)
        top = np.sort(x)[::-1][:K]
        if len(top) > 1 and np.min(top[:-1] - top[1:]) < 2 * np.delete(E[r], items).max():
            bad.append(r)
    return bad
