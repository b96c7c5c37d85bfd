"""Numpy restatement, in float64, of the WARP contract of include/pda_hip_warp.h for the WARP tests; it holds no test.

    weight_table         wtab of a (n_eligible, T, kind): a direct float64 sum per entry, no cumulative tricks
    first_violator_loop  N of every row, the definition itself: the plain loop over j
    first_violator       the same, vectorised
    sample               one batch: the user, positive and popularity columns of sampler_ref.sample, the candidates of ssm_ref.ssm_sample, the
                         float64 scores of dns_ref.scores, N, the negative, the coefficient, the masked test outputs and stat
    x_bound              the a-priori bound of the kernel's fp32 x_j = s_p - s_j against the float64 one
    admitted             the values of N a kernel within that bound may give, row by row
    step_terms / step_grads / step_adam   the loss, its gradients in closed form, and one whole train step with the oracle's Adam
    h_bound              the same bound for the step's x_t
    spread_margin        a margin, a multiple of 1/8, that spreads N over 1 .. T on given scores

The bound (x_bound).  dns_ref.scores gives, for each raw score, e_raw = 2 d 2^-24 sum_k |u_k i_k| with |s^ - s| <= e_raw for ANY order of the
fp32 sum.  x^ = fl(s_p^ - s_j^) is one more rounding: |x^ - (s_p^ - s_j^)| <= eps |s_p^ - s_j^| <= eps (|x| + e_p + e_j).  Together
    |x^ - x| <= e_p + e_j + eps (|x| + e_p + e_j).
The violation test is margin - x^ > 0 in fp32: a difference of two fp32 numbers keeps its sign when it is rounded (it is zero only for equal
operands, and differences in the denormal range are exact), so the test decides by x^ against the (fp32) margin, and a candidate whose
float64 margin - x lies farther from 0 than the bound is decided the same way by every kernel within the bound.  It is a bound, not a tuned number.
"""
import numpy as np

import dns_ref as dr
import sampler_ref as sr
import ssm_ref

EPS = dr.EPS
KINDS = ("harmonic", "log", "none")


def weight_table(n_eligible, T, kind):
    """float64 [T + 1]: wtab[0] = 0; wtab[N] from rank(N) = floor((n_eligible - 1) / N)."""
    tab = np.zeros(T + 1, dtype=np.float64)
    for N in range(1, T + 1):
        rank = (int(n_eligible) - 1) // N
        if kind == "harmonic":
            tab[N] = sum(1.0 / k for k in range(1, rank + 1))
        elif kind == "log":
            tab[N] = np.log(float(max(1, rank)))
        elif kind == "none":
            tab[N] = 1.0
        else:
            raise ValueError(kind)
    return tab


def first_violator_loop(sp, s, margin):
    """sp [B], s [B, T] -> N int64 [B]: 1 + the column of the first candidate with margin - (sp - s_j) > 0, 0 without one.  NaN: never."""
    B, T = s.shape
    N = np.zeros(B, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for r in range(B):
            for j in range(T):
                x = sp[r] - s[r, j]
                h = margin - x
                if h > 0:           # (False for a NaN)
                    N[r] = j + 1
                    break
    return N


def first_violator(sp, s, margin):
    sp, s = np.asarray(sp, dtype=np.float64), np.asarray(s, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        viol = (margin - (sp[:, None] - s)) > 0
    return np.where(viol.any(1), viol.argmax(1) + 1, 0).astype(np.int64)


def outputs_for(N, cand, score, wtab32):
    """What the call writes for a given N [B]: neg, coef (fp32), the masked cand / cand_score, stat."""
    B, T = cand.shape
    rows = np.arange(B)
    neg = np.where(N > 0, cand[rows, np.maximum(N, 1) - 1], cand[:, T - 1]).astype(np.int32)
    coef = np.where(N > 0, np.asarray(wtab32, dtype=np.float32)[N], np.float32(0)).astype(np.float32)
    keep = (N[:, None] == 0) | (np.arange(T)[None, :] < N[:, None])
    return dict(neg=neg, coef=coef, cand_out=np.where(keep, cand, -1).astype(np.int32), score_out=np.where(keep, score, 0.0),
                stat=np.array([int(N.sum()), int((N == 0).sum())], dtype=np.int64))


def sample(seed, step, B, T, margin, wtab32, U, I, indptr, indices, *, slots=None, user_pool=None, n_pool=0, users=None, neg_range,
           pop_matrix=None):
    """pda_warp_sample_f32 for one batch -> dict(users, pos, neg, trials, coef, pos_pop, neg_pop, cand [B, T], score [B, T] float64, pos_score
    [B] float64, e_cand, e_pos (the bounds of the scores), cand_out, score_out, stat, slot)."""
    base = sr.sample(seed, step, B, indptr, indices, slots=slots, user_pool=user_pool, n_pool=n_pool, users=users, neg_range=neg_range,
                     pop_matrix=pop_matrix)
    cand = ssm_ref.ssm_sample(seed, step, B, T, indptr, indices, user_pool=user_pool, n_pool=n_pool, users=users, neg_range=neg_range)["negs"]
    n_slots = 0 if pop_matrix is None else pop_matrix.shape[1]
    slot = dr.slots_of(base, seed, step, indptr, slots, n_slots)
    s, e_cand = dr.scores(U, I, base["users"], cand, dr.HEAD_RAW)
    sp, e_pos = dr.scores(U, I, base["users"], base["pos"][:, None], dr.HEAD_RAW)
    sp, e_pos = sp[:, 0], e_pos[:, 0]
    N = first_violator(sp, s, margin)
    out = dict(users=base["users"], pos=base["pos"], trials=N.astype(np.int32), pos_pop=base["pos_pop"], neg_pop=None, cand=cand, score=s,
               pos_score=sp, e_cand=e_cand, e_pos=e_pos, slot=slot, neg0=base["neg"], neg0_pop=base["neg_pop"])
    out.update(outputs_for(N, cand, s, wtab32))
    if pop_matrix is not None:
        out["neg_pop"] = pop_matrix[out["neg"].astype(np.int64), slot]
    return out


def x_bound(ref):
    """[B, T]: the bound of |x^_j - x_j| (module docstring)."""
    x = ref["pos_score"][:, None] - ref["score"]
    e = ref["e_pos"][:, None] + ref["e_cand"]
    with np.errstate(invalid="ignore"):
        return e + EPS * (np.abs(x) + e)


def undecided(ref, margin):
    """[B, T] bool: the candidates whose float64 margin - x_j lies within the bound of 0."""
    with np.errstate(invalid="ignore"):
        h = margin - (ref["pos_score"][:, None] - ref["score"])
        return np.abs(h) <= x_bound(ref)


def admitted(ref, margin):
    """-> (ok [B, T + 1] bool: ok[r, N] iff a kernel within the bound may give N for row r; blurred [B] bool: the rows that hold an undecided
    candidate before their first sure violator)."""
    B, T = ref["cand"].shape
    und = undecided(ref, margin)
    with np.errstate(invalid="ignore"):
        sure = ((margin - (ref["pos_score"][:, None] - ref["score"])) > 0) & ~und
    first_sure = np.where(sure.any(1), sure.argmax(1), T)                # column, T: none
    before = np.arange(T)[None, :] < first_sure[:, None]
    ok = np.zeros((B, T + 1), dtype=bool)
    ok[:, 1:] = und & before
    rows = np.arange(B)
    has = first_sure < T
    ok[rows[has], first_sure[has] + 1] = True
    ok[~has, 0] = True
    return ok, (und & before).any(1)


# ---- the step ------------------------------------------------------------------------------------------------------------------------------------
def step_terms_torch(U, I, users, pos, neg, coef, *, margin, regs, reg_div, B=None):
    """The stated loss in torch (any dtype), for autograd: dict(loss, mf, reg).  users / pos / neg / coef: the batch's VALID triplets."""
    import torch
    B = len(users) if B is None else B
    u, p, n = U[users], I[pos], I[neg]
    h = margin - ((u * p).sum(1) - (u * n).sum(1))
    act = (coef > 0) & (h > 0)
    mf = (coef * h)[act].sum() / B
    reg = regs * 0.5 * ((u ** 2).sum() + (p ** 2).sum() + (n ** 2).sum()) / reg_div        # tf.nn.l2_loss = sum(x^2) / 2
    return dict(loss=mf + reg, mf=mf, reg=reg)


def step_grads(U, I, users, pos, neg, coef, *, margin, regs, reg_div, B=None):
    """numpy float64, closed form: (terms [3] = loss, mf, reg; gU; gI; h [len(users)]).  d mf / d x_t = -coef_t / B on the active triplets."""
    U64, I64 = np.asarray(U, dtype=np.float64), np.asarray(I, dtype=np.float64)
    users, pos, neg = (np.asarray(a, dtype=np.int64) for a in (users, pos, neg))
    coef = np.asarray(coef, dtype=np.float64)
    B = len(users) if B is None else B
    u, p, n = U64[users], I64[pos], I64[neg]
    with np.errstate(invalid="ignore"):
        h = margin - ((u * p).sum(1) - (u * n).sum(1))
        act = (coef > 0) & (h > 0)
    mf = (coef * h)[act].sum() / B
    c = regs / reg_div
    reg = c * 0.5 * ((u ** 2).sum() + (p ** 2).sum() + (n ** 2).sum())
    g = np.where(act, -coef / B, 0.0)[:, None]
    gU, gI = np.zeros_like(U64), np.zeros_like(I64)
    np.add.at(gU, users, g * (p - n) + c * u)
    np.add.at(gI, pos, g * u + c * p)
    np.add.at(gI, neg, -g * u + c * n)
    return np.array([mf + reg, mf, reg]), gU, gI, h


def step_adam(U, I, state, t, lr, users, pos, neg, coef, **kw):
    """One train step in float64: -> (U1, I1, state, terms).  state = dict(mU, vU, mI, vI) or None."""
    from oracle import pda_oracle as po
    terms, gU, gI, _ = step_grads(U, I, users, pos, neg, coef, **kw)
    if state is None:
        state = {k: np.zeros_like(x, dtype=np.float64) for k, x in (("mU", U), ("vU", U), ("mI", I), ("vI", I))}
    U1, mU, vU = po.adam_dense_decay_step(np.asarray(U, dtype=np.float64), state["mU"], state["vU"], gU, t, lr)
    I1, mI, vI = po.adam_dense_decay_step(np.asarray(I, dtype=np.float64), state["mI"], state["vI"], gI, t, lr)
    return U1, I1, dict(mU=mU, vU=vU, mI=mI, vI=vI), terms


def h_bound(U, I, users, pos, neg):
    """[B]: the bound of the step's fp32 x_t = u.p - u.n (triplet_dots: the same d / 4-lane sums) against float64, as x_bound takes it."""
    U64, I64 = np.abs(np.asarray(U, dtype=np.float64)), np.abs(np.asarray(I, dtype=np.float64))
    users, pos, neg = (np.asarray(a, dtype=np.int64) for a in (users, pos, neg))
    d = U64.shape[1]
    e = 2.0 * d * EPS * ((U64[users] * I64[pos]).sum(1) + (U64[users] * I64[neg]).sum(1))
    Ux, Ix = np.asarray(U, dtype=np.float64), np.asarray(I, dtype=np.float64)
    x = (Ux[users] * Ix[pos]).sum(1) - (Ux[users] * Ix[neg]).sum(1)
    return e + EPS * (np.abs(x) + e)


def spread_margin(sp, s, first_round=4):
    """A margin, a multiple of 1/8, chosen from float64 scores so that N spreads over 1 .. T: among the multiples of 1/8 in the range of the
    x_j that leave at least one row without a violator, the one that splits the rows most evenly between those that close in round 0
    (1 <= N <= first_round) and the rest.  -> margin; the caller asserts what it needs of it."""
    x = sp[:, None] - s                                          # candidate j violates iff margin > x_j
    lo, hi = np.floor(np.nanmin(x) * 8.0) / 8.0, np.ceil(np.nanmax(x) * 8.0) / 8.0
    best, best_m = -1.0, float(lo)
    for m in np.arange(lo, hi + 0.125, 0.125):
        N = first_violator(sp, s, float(m))
        early = ((N >= 1) & (N <= first_round)).mean()
        if (N == 0).any() and min(early, 1.0 - early) > best:
            best, best_m = min(early, 1.0 - early), float(m)
    return best_m
