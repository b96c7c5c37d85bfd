"""Reference, rounding bound, fp32 emulation and mutants of the reference's own train step (pda_train_common.h: bpr_triplet, bpr_dloss_dx,
triplet_row_grads, the loss reduction, the SGD scatter, the first Adam step) for the train-parity tests; it holds no test.

    case / Case      the tables and the batch the CPU and the GPU tests share for one (d, B, kind)
    reference        the float64 quantities of a case, taken from oracle.pda_oracle
    bound            an a-priori bound on |fp32 kernel - reference| per element of every quantity (derived below, not measured)
    emulate_fp32     the kernel's expressions in numpy float32 in the kernel's order, occurrences summed in a given order
    shared           (case, reference, bound) computed once per process
    mutant / MUTANTS single-defect variants of the float64 reference, with what they change and where they show

Quantities (the keys of every dict here): loss = (loss, mf, reg); due, dpe, dne [B, d] per occurrence; gU, gI the summed gradients;
U_sgd, I_sgd the tables after one exact SGD step at `lr`; mU, vU, mI, vI the Adam moments after the first step from zero moments.

THE BOUND, line by line.  eps = 2^-24 (one fp32 rounding, relative), g(n) = 1.01 n eps (n roundings on one value; the 1.01 pays for the
products of (1 + eps) factors).  The library is built with -ffp-contract=off and without fast-math, so every *, +, - rounds once.  expf, logf
and the division each get ULP = 4 ulp = 8 eps: no ROCm math accuracy table is installed beside the compiler to take tighter figures from (the
documented device-library figures are 1 ulp for expf / logf and a correctly rounded division, so 4 is generous).

  row dot       ps = <u, p>: 4 products per lane summed left to right (1 product rounding + 3 sums), then log2(d / 4) ladder steps:
                  d_ps = g(4 + log2(d / 4)) A_p,   A_p = sum_k |u_k p_k|                                 (d_ns likewise)
  ELU + 1       e_p = 1 (ps > 0) or exp(ps): the error of ps enters exp(ps) relatively, expf adds ULP:
                  d_e = e_p (d_ps + ULP eps) on the exp branch; on the linear branch 0, unless |ps| <= d_ps, where the kernel may take the other
                  branch than the reference (the branches' values then differ by O(ps^2), their slopes by |ps| <= d_ps): d_e = d_ps + ULP eps
                psw = (ps + 1) q or e_p q:  d_psw = q (d_ps + eps |ps + 1|) + eps |psw|   resp.   q d_e + eps |psw|
                a_p = q e_p:                d_a = q d_e + eps |a_p|                        (plain BPR-MF: psw = ps, a_p = 1, d_a = 0)
  x             x = psw - nsw:              d_x = d_psw + d_nsw + eps |x|
  sigmoid       s = 1 / (1 + expf(-x)): expf ULP (weighted by 1 - s <= 1), the sum 1, the division ULP:   r_s = (2 ULP + 1) eps relative
  loss term     maxi = logf(s + 1e-10f): |d maxi / dx| = s (1 - s) / (s + 1e-10) <= 1; the argument carries r_s, the constant's rounding and the
                sum's (2 eps); logf adds ULP eps |maxi|:      d_maxi = h d_x + r_s + 2 eps + ULP eps |maxi|,  h = s (1 - s) / (s + 1e-10)
  d loss / dx   gg = -inv_B s (1 - s) / (s + 1e-10f), |d log gg / dx| <= 1 (it is 1 - 2 s - h).  Relative: d_x; s in the numerator and in the
                denominator (2 r_s, no cancellation claimed); the constant, the sum s + 1e-10f, the difference 1 - s, the two products and
                inv_B = 1.f / B (6 eps); the division (ULP eps).  Absolute: 1 - s cancels, so the error s r_s of s stays absolute in it:
                  d_gg = |gg| (d_x + 2 r_s + (6 + ULP) eps) + inv_B (s r_s + FLUSH)
                FLUSH = 6e-29: where fp32 expf overflows or underflows (|x| > 88.7) the kernel's gg is exactly 0 and the reference's is below
                e^-88 / 1e-10 = 6e-29 per unit of 1 / B; added everywhere, it is far below every other term.
  gp, gn        gp = gg a_p:                d_gp = d_gg |a_p| + |gg| d_a + eps |gp|
  row grads     due_k = gp p_k - gn n_k + c u_k, c = regs / reg_div formed in fp32 (both roundings and the division: 3 eps): three products,
                two sums and c's error are at most 6 roundings on T_k = |gp p_k| + |gn n_k| + |c u_k|:
                  d_due = d_gp |p_k| + d_gn |n_k| + g(6) T_k;   dpe, dne the same with their two terms
  loss sums     mf = -inv_B sum maxi, reg = c 0.5 sum sq: any order inside a workgroup (at most max(14, TPB) sums deep: 6 shuffle steps, 8 waves),
                any order of the workgroups' atomics (n_wg = ceil(B / TPB) + 2, the 2 for a batch split over two launches), inv_B, the product:
                  d_mf  = inv_B sum d_maxi + g(max(14, TPB) + n_wg + 3) inv_B sum |maxi|
                  d_reg = g(6 + max(14, TPB) + n_wg + 4) reg      (6: the square and the 5 sums inside a lane; 4: c and the two products)
                  d_loss = d_mf + d_reg + g(n_wg + 1) (inv_B sum |maxi| + reg)
  summed        gU[r] = sum over the n occurrences of row r (gI: positives and negatives together):
                  d_sum = sum d_occ + g(n - 1) sum (|occ| + d_occ)                       for any order of the atomics
  SGD step      x1 = x - lr sum: the products -lr occ (1, and lr's own rounding to fp32: 1), n sums in any order onto x, and two spare roundings
                for the planned step, which forms (sum + n c row) lr before it subtracts:
                  d_x1 = lr sum d_occ + g(n + 3) lr sum (|occ| + d_occ) + g(n) |x|
  first Adam    m = (1 - b1) G, v = (1 - b2) G G with b1 = 0.9f, b2 = 0.999f: 1.f - b is exact, b's rounding (b eps absolute) is 9 eps resp.
                999 eps of 1 - b; one product for m, two for v:
                  d_m = 0.1 d_G + g(10) 0.1 |G|;   d_v = 0.001 (2 |G| d_G + d_G^2) + g(1001) 0.001 G^2;   idle rows: exactly 0
"""
import numpy as np

from oracle import pda_oracle as po

NU, NI = 64, 40
REGS = 1e-2
DIMS = (32, 64, 128, 256)
KINDS = ("spread", "negative_dots", "hot", "unshared", "saturated")
EPS32 = 2.0 ** -24
ULP = 8.0                 # 4 ulp in units of eps = half an ulp: the budget of one expf, logf or division
FLUSH = 6e-29
QUANTITIES = ("loss", "due", "dpe", "dne", "gU", "gI", "U_sgd", "I_sgd", "mU", "vU", "mI", "vI")
ORDERS = ("given", "reversed", "shuffled")
SAT_X = (-30.0, -100.0, 40.0)     # x of the three hand-built triplets of kind "saturated" (about: see _saturate)


def tpb(d):
    """Triplets per workgroup of the step kernels (512 threads, d / 4 lanes per triplet)."""
    return 2048 // d


def batches(d):
    t = tpb(d)
    return (1, t - 1, t + 1, 3 * t + 5)


def gpu_cases():
    """Every (d, B, kind) of the GPU list: all d x B x kinds, and d = 64, B = 2048 (many workgroups, dozens of occurrences per row)."""
    out = [(d, B, kind) for d in DIMS for B in batches(d) for kind in KINDS]
    return out + [(64, 2048, "spread"), (64, 2048, "hot")]


def g_(n):
    return 1.01 * n * EPS32


class Case:
    """U, I float32 tables the forward pass reads; users / pos / neg int32 [B]; pp / pn float32 [B] the popularity weights of the PD / PDA head
    (heads(False) = plain BPR-MF); regs, reg_div, mean_div; Um / Im: the tables that take an update where they are not U / I (bf16 masters)."""

    def __init__(self, U, I, users, pos, neg, pp, pn, regs=REGS, reg_div=None, mean_div=None, Um=None, Im=None, sat=()):
        self.U, self.I = np.ascontiguousarray(U, dtype=np.float32), np.ascontiguousarray(I, dtype=np.float32)
        self.users, self.pos, self.neg = (np.ascontiguousarray(a, dtype=np.int32) for a in (users, pos, neg))
        self.pp, self.pn = np.ascontiguousarray(pp, dtype=np.float32), np.ascontiguousarray(pn, dtype=np.float32)
        self.B, self.d = len(self.users), self.U.shape[1]
        self.regs, self.reg_div = regs, float(self.B if reg_div is None else reg_div)
        self.mean_div = float(self.B if mean_div is None else mean_div)
        self.Um, self.Im = (self.U if Um is None else Um), (self.I if Im is None else Im)
        self.sat = tuple(sat)            # positions of the saturated triplets (x = SAT_X[j] at sat[j])
        assert self.users.max() < self.U.shape[0] and max(self.pos.max(), self.neg.max()) < self.I.shape[0] and min(
            self.users.min(), self.pos.min(), self.neg.min()) >= 0, "ids are always inside the tables"

    def heads(self, pop):
        return (self.pp, self.pn) if pop else (None, None)

    def take(self, order):
        """The same tables with the batch reordered (or cut): a stable sort by positive, one shard's part."""
        return Case(self.U, self.I, self.users[order], self.pos[order], self.neg[order], self.pp[order], self.pn[order], self.regs, self.reg_div,
                    self.mean_div, self.Um, self.Im)

    def with_tables(self, U, I, Um=None, Im=None):
        return Case(U, I, self.users, self.pos, self.neg, self.pp, self.pn, self.regs, self.reg_div, self.mean_div, Um, Im, self.sat)


def _saturate(U, I, d, rng):
    """Users 0..2 and items 0..5 by hand, along one dense direction h (every entry +-1 / sqrt(d), relative jitter 1e-3 so that all products
    round): u = r h, p = a h, n = b h give ps = r a, ns = r b.  With both heads (the weights of these triplets are 1):
        (u0, i0, i1): ps = -1, ns =  30: x = -31 plain, exp(-1) - 31  = -30.6 with popularity: the + 1e-10 decides the gradient
        (u1, i2, i3): ps = -1, ns = 100: x = -101 plain, -100.6 with popularity: fp32 expf(-x) overflows, the gradient is exactly 0
        (u2, i4, i5): ps = 40, ns =  -1: x = +41 plain, 41 - exp(-1) = +40.6 with popularity: 1 - s vanishes in fp32"""
    h = rng.choice([-1.0, 1.0], d) / np.sqrt(d)
    jit = lambda: 1.0 + 1e-3 * rng.standard_normal(d)      # noqa: E731
    for u, (r, a, b) in enumerate(((5.0, -0.2, 6.0), (10.0, -0.1, 10.0), (5.0, 8.0, -0.2))):
        U[u], I[2 * u], I[2 * u + 1] = r * h * jit(), a * h * jit(), b * h * jit()


def case(d, B, kind, distinct_users=False, shards=1):
    """64 users and 40 items so that rows repeat (more where the kind cannot live there: `unshared` and distinct users need B user rows,
    `unshared` 2 B item rows).  shards > 1: triplet t takes both items from the item range of shard t * shards // B.
        spread          0.3 N(0, 1): both ELU branches occur
        negative_dots   user rows positive, item rows negative: every u.p and u.n is below 0
        hot             one positive on 30 % of the batch, repeated users (unless distinct_users)
        unshared        distinct users, no item row occurs twice anywhere in the batch
        saturated       _saturate's three triplets at the positions 0, B // 2, B - 1 (as many as are distinct) among ordinary ones"""
    assert kind in KINDS
    rng = np.random.default_rng(100000 * KINDS.index(kind) + 1000 * d + B + (7 if distinct_users else 0) + 13 * (shards - 1))
    per_shard = -(-B // shards)
    nU = max(NU, B) if (distinct_users or kind == "unshared") else NU
    nI = NI if kind != "unshared" else max(NI, 2 * per_shard * shards)
    nI = -(-nI // shards) * shards
    per = nI // shards
    U = (0.3 * rng.standard_normal((nU, d))).astype(np.float32)
    I = (0.3 * rng.standard_normal((nI, d))).astype(np.float32)
    if kind == "negative_dots":
        U, I = np.abs(U) + np.float32(0.01), -np.abs(I) - np.float32(0.01)
    lo = (np.arange(B) * shards // B) * per
    users = (rng.permutation(nU)[:B] if (distinct_users or kind == "unshared") else rng.integers(0, nU, B))
    if kind == "unshared":
        pos, neg = np.empty(B, np.int64), np.empty(B, np.int64)
        for s in range(shards):
            t = np.flatnonzero(lo == s * per)
            perm = s * per + rng.permutation(per)
            pos[t], neg[t] = perm[:len(t)], perm[len(t):2 * len(t)]
    else:
        pos, neg = lo + rng.integers(0, per, B), lo + rng.integers(0, per, B)
    if kind == "hot":
        hot = rng.random(B) < 0.3
        pos[hot] = lo[hot] + 7
    pp, pn = (rng.uniform(0, 1, B) ** 0.22).astype(np.float32), (rng.uniform(0, 1, B) ** 0.22).astype(np.float32)
    sat = ()
    if kind == "saturated":
        assert shards == 1
        _saturate(U, I, d, rng)
        sat = tuple(sorted({0, B // 2, B - 1}))
        users, pos, neg = np.where(users < 3, users + 3, users), np.where(pos < 6, pos + 6, pos), np.where(neg < 6, neg + 6, neg)
        for j, t in enumerate(sat):
            users[t], pos[t], neg[t], pp[t], pn[t] = j, 2 * j, 2 * j + 1, 1.0, 1.0
    return Case(U, I, users, pos, neg, pp, pn, sat=sat)


def saturated_single(d, j):
    """The one-triplet batch of _saturate's triplet j (x = SAT_X[j])."""
    c = case(d, 3, "saturated")
    return Case(c.U, c.I, [j], [2 * j], [2 * j + 1], [1.0], [1.0], sat=(None,) * j + (0,))


def occurrences(c):
    """n_occ per row: (users [nU], items [nI], positives and negatives together)."""
    return np.bincount(c.users, minlength=c.U.shape[0]), np.bincount(np.concatenate([c.pos, c.neg]), minlength=c.I.shape[0])


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------------------
def _finish(c, loss, due, dpe, dne, lr):
    """The summed quantities from the per-occurrence gradients, by the oracle's own functions."""
    nU, nI = c.U.shape[0], c.I.shape[0]
    gU, gI = po.dense_grads(nU, nI, c.users, c.pos, c.neg, due, dpe, dne)
    z = np.zeros_like
    _, mU, vU = po.adam_dense_decay_step(z(gU), z(gU), z(gU), gU, 1, 0.0)
    _, mI, vI = po.adam_dense_decay_step(z(gI), z(gI), z(gI), gI, 1, 0.0)
    return dict(loss=np.asarray(loss, dtype=np.float64), due=due, dpe=dpe, dne=dne, gU=gU, gI=gI,
                U_sgd=po.sgd_step(c.Um.astype(np.float64), gU, lr), I_sgd=po.sgd_step(c.Im.astype(np.float64), gI, lr), mU=mU, vU=vU, mI=mI, vI=vI)


def reference(c, pop, lr=0.05):
    """The float64 quantities of a case from oracle.pda_oracle (bpr_forward, bpr_loss, bpr_grads, dense_grads, sgd_step, train_step).  The
    oracle's mean is over len(batch); a shard's part (mean_div != B) rescales the two terms that carry it."""
    pp, pn = c.heads(pop)
    fw = po.bpr_forward(c.U, c.I, c.users, c.pos, c.neg, pp, pn)
    loss, mf, reg = po.bpr_loss(fw, c.regs, c.reg_div)
    due, dpe, dne = po.bpr_grads(fw, c.regs, c.reg_div, pp, pn)
    if c.mean_div != c.B:
        k = c.B / c.mean_div
        cc = c.regs / c.reg_div
        mf = mf * k
        loss = mf + reg
        due, dpe, dne = ((g - cc * fw[r]) * k + cc * fw[r] for g, r in ((due, "ue"), (dpe, "pe"), (dne, "ne")))
    out = _finish(c, (loss, mf, reg), due, dpe, dne, lr)
    if c.mean_div == c.B and c.Um is c.U:          # the whole step once more through the oracle's own train_step
        U1, I1, _, _ = po.train_step(c.U, c.I, c.users, c.pos, c.neg, pp, pn, c.regs, c.reg_div, lr, optimizer="sgd")
        _, _, st, _ = po.train_step(c.U, c.I, c.users, c.pos, c.neg, pp, pn, c.regs, c.reg_div, lr, optimizer="adam")
        assert np.array_equal(U1, out["U_sgd"]) and np.array_equal(I1, out["I_sgd"]) and all(np.array_equal(st[k], out[k]) for k in st)
    return out


# ---- the bound ---------------------------------------------------------------------------------------------------------------------------------
def _sum_rows(n, idx, vals):
    out = np.zeros((n,) + vals.shape[1:])
    np.add.at(out, idx, vals)
    return out


def bound(c, pop, lr=0.05, tables=True):
    """The module docstring's derivation in float64 -> dict of arrays shaped like reference()'s.  tables=False: without the SGD tables and the
    Adam moments (large tables: the summed gradients alone cost half)."""
    pp, pn = c.heads(pop)
    fw = po.bpr_forward(c.U, c.I, c.users, c.pos, c.neg, pp, pn)
    ue, pe, ne, ps, ns = (fw[k] for k in ("ue", "pe", "ne", "ps", "ns"))
    d, B, inv_B = c.d, c.B, 1.0 / c.mean_div
    n_dot = 4 + np.log2(d / 4)
    d_ps, d_ns = g_(n_dot) * (np.abs(ue * pe)).sum(1), g_(n_dot) * (np.abs(ue * ne)).sum(1)

    def head(s, d_s, q):
        if q is None:
            return s, d_s, np.ones_like(s), np.zeros_like(s)
        q = q.astype(np.float64)
        lin = s > 0
        e = np.where(lin, 1.0, np.exp(np.minimum(s, 0.0)))
        d_e = np.where(lin & (np.abs(s) > d_s), 0.0, e * (d_s + ULP * EPS32))
        sw = np.where(lin, s + 1.0, e) * q
        d_sw = np.where(lin & (np.abs(s) > d_s), q * (d_s + EPS32 * np.abs(s + 1.0)), q * np.maximum(d_e, d_s + EPS32 * np.abs(s + 1.0))) + EPS32 * np.abs(sw)
        a = q * e
        return sw, d_sw, a, q * d_e + EPS32 * np.abs(a)

    psw, d_psw, a_p, d_ap = head(ps, d_ps, pp)
    nsw, d_nsw, a_n, d_an = head(ns, d_ns, pn)
    x = psw - nsw
    d_x = d_psw + d_nsw + EPS32 * np.abs(x)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-x))
    r_s = (2 * ULP + 1) * EPS32
    h = s * (1.0 - s) / (s + 1e-10)
    maxi = np.log(s + 1e-10)
    d_maxi = h * d_x + r_s + 2 * EPS32 + ULP * EPS32 * np.abs(maxi)
    gg = inv_B * h
    d_gg = gg * (d_x + 2 * r_s + (6 + ULP) * EPS32) + inv_B * (s * r_s + FLUSH)
    gp, gn = gg * a_p, gg * a_n
    d_gp, d_gn = d_gg * a_p + gg * d_ap + EPS32 * gp, d_gg * a_n + gg * d_an + EPS32 * gn
    cc = c.regs / c.reg_div
    col = lambda v: v[:, None]                 # noqa: E731
    A = np.abs
    b = dict(due=col(d_gp) * A(pe) + col(d_gn) * A(ne) + g_(6) * (col(gp) * A(pe) + col(gn) * A(ne) + cc * A(ue)),
             dpe=col(d_gp) * A(ue) + g_(6) * (col(gp) * A(ue) + cc * A(pe)),
             dne=col(d_gn) * A(ue) + g_(6) * (col(gn) * A(ue) + cc * A(ne)))
    t, n_wg = tpb(d), -(-B // tpb(d)) + 2
    sum_maxi, reg = inv_B * A(maxi).sum(), cc * 0.5 * ((ue ** 2).sum() + (pe ** 2).sum() + (ne ** 2).sum())
    d_mf = inv_B * d_maxi.sum() + g_(max(14, t) + n_wg + 3) * sum_maxi
    d_reg = g_(6 + max(14, t) + n_wg + 4) * reg
    b["loss"] = np.array([d_mf + d_reg + g_(n_wg + 1) * (sum_maxi + reg), d_mf, d_reg])
    # the summed quantities: |occ| from the reference's own per-occurrence gradients
    rg = reference_grads(c, pop)
    due, dpe, dne = (A(g) for g in rg)
    nU, nI = c.U.shape[0], c.I.shape[0]
    occ_u, occ_i = occurrences(c)
    items = np.concatenate([c.pos, c.neg])
    for name, n, idx, occ, d_occ, n_occ, x0 in (("U", nU, c.users, due, b["due"], occ_u, c.Um),
                                                ("I", nI, items, np.concatenate([dpe, dne]), np.concatenate([b["dpe"], b["dne"]]), occ_i, c.Im)):
        s_d, s_abs = _sum_rows(n, idx, d_occ), _sum_rows(n, idx, occ + d_occ)
        k = n_occ[:, None].astype(np.float64)
        d_G = s_d + g_(1) * np.maximum(k - 1, 0) * s_abs
        if tables:
            G = A(_sum_rows(n, idx, np.concatenate(rg[1:]) if name == "I" else rg[0]))
        b["g" + name] = d_G
        if not tables:
            continue
        b[name + "_sgd"] = lr * s_d + g_(1) * (k + 3) * lr * s_abs * (k > 0) + g_(1) * k * A(x0.astype(np.float64))
        b["m" + name] = 0.1 * d_G + g_(10) * 0.1 * G
        b["v" + name] = 0.001 * (2 * G * d_G + d_G ** 2) + g_(1001) * 0.001 * G * G
    return b


def reference_grads(c, pop):
    """(due, dpe, dne) of reference(), without the rest."""
    pp, pn = c.heads(pop)
    fw = po.bpr_forward(c.U, c.I, c.users, c.pos, c.neg, pp, pn)
    due, dpe, dne = po.bpr_grads(fw, c.regs, c.reg_div, pp, pn)
    if c.mean_div != c.B:
        k, cc = c.B / c.mean_div, c.regs / c.reg_div
        due, dpe, dne = ((g - cc * fw[r]) * k + cc * fw[r] for g, r in ((due, "ue"), (dpe, "pe"), (dne, "ne")))
    return due, dpe, dne


_SHARED = {}


def shared(d, B, kind, pop, lr=0.05, **kw):
    """(case, reference, bound) of one case: computed once per process, shared among the tests that need it, arrays read-only."""
    key = (d, B, kind, pop, lr) + tuple(sorted(kw.items()))
    if key not in _SHARED:
        c = case(d, B, kind, **kw)
        ref, bnd = reference(c, pop, lr), bound(c, pop, lr)
        for a in list(ref.values()) + list(bnd.values()):
            a.setflags(write=False)
        _SHARED[key] = (c, ref, bnd)
    return _SHARED[key]


# ---- the fp32 emulation ------------------------------------------------------------------------------------------------------------------------
F = np.float32


def _dot_lanes(a, b):
    """[B, d] x [B, d] -> [B, d / 4]: dot4 of every lane, the 4 products summed left to right."""
    a, b = a.reshape(len(a), -1, 4), b.reshape(len(b), -1, 4)
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]) + a[..., 3] * b[..., 3]


def _ladder(v):
    """The xor-shuffle ladder over the d / 4 lanes: offsets d / 8, ..., 1 (every lane ends with the same bits)."""
    while v.shape[1] > 1:
        o = v.shape[1] // 2
        v = v[:, :o] + v[:, o:]
    return v[:, 0]


def _order(n, how, seed=5):
    if how == "given":
        return np.arange(n)
    if how == "reversed":
        return np.arange(n)[::-1]
    return np.random.default_rng(seed).permutation(n)


def _seq_sum(vals):
    acc = F(0)
    for v in vals:
        acc = F(acc + v)
    return acc


def emulate_fp32(c, pop, lr=0.05, order="given"):
    """bpr_triplet / bpr_dloss_dx / triplet_row_grads, the loss reduction, the atomics of the SGD and the gradient scatter and adam_moments as the
    kernels write them, every intermediate a float32; `order`: the order in which the occurrences (and the workgroups' loss shares) are summed."""
    pp, pn = c.heads(pop)
    ue, pe, ne = c.U[c.users], c.I[c.pos], c.I[c.neg]
    B, d = c.B, c.d
    with np.errstate(over="ignore", under="ignore"):
        ps, ns = _ladder(_dot_lanes(ue, pe)), _ladder(_dot_lanes(ue, ne))
        ap = an = np.ones(B, F)
        psw, nsw = ps, ns
        if pop:
            ep = np.where(ps > 0, F(1), np.exp(ps))
            en = np.where(ns > 0, F(1), np.exp(ns))
            psw, nsw = np.where(ps > 0, ps + F(1), ep) * pp, np.where(ns > 0, ns + F(1), en) * pn
            ap, an = pp * ep, pn * en
        x = psw - nsw
        inv_B, cc = F(1) / F(c.mean_div), F(c.regs) / F(c.reg_div)
        sg = F(1) / (F(1) + np.exp(-x))
        maxi = np.log(sg + F(1e-10))
        gg = -inv_B * sg * (F(1) - sg) / (sg + F(1e-10))
    gp, gn = (gg * ap)[:, None], (gg * an)[:, None]
    due = gp * pe - gn * ne + cc * ue
    dpe = gp * ue + cc * pe
    dne = -gn * ue + cc * ne
    sq = (_dot_lanes(ue, ue) + _dot_lanes(pe, pe)) + _dot_lanes(ne, ne)
    assert all(a.dtype == F for a in (ps, x, sg, maxi, gg, due, dpe, dne, sq))
    # the loss: lanes in `order` inside a workgroup, workgroups in `order`
    t = tpb(d)
    acc = np.zeros(3, F)
    blocks = [(k, min(k + t, B)) for k in range(0, B, t)]
    for k in _order(len(blocks), order):
        a, z = blocks[k]
        o = _order(z - a, order, seed=k)
        sm, ss = _seq_sum(maxi[a:z][o]), _seq_sum(sq[a:z][o].ravel())
        mf, rg = F(-sm * inv_B), F(cc * F(0.5) * ss)
        acc = (acc + np.array([mf + rg, mf, rg], F)).astype(F)
    out = dict(loss=acc, due=due, dpe=dpe, dne=dne)
    nlr = F(-lr)
    o = _order(B, order)
    o2 = _order(2 * B, order)
    items, gi = np.concatenate([c.pos, c.neg]), np.concatenate([dpe, dne])
    for name, tab, idx, g, oo in (("U", c.Um, c.users, due, o), ("I", c.Im, items, gi, o2)):
        G, X = np.zeros(tab.shape, F), tab.astype(F).copy()
        step = g * nlr
        for i in oo:
            G[idx[i]] += g[i]
            X[idx[i]] += step[i]
        out["g" + name], out[name + "_sgd"] = G, X
        m = F(0.9) * np.zeros_like(G) + (F(1) - F(0.9)) * G
        v = F(0.999) * np.zeros_like(G) + (F(1) - F(0.999)) * G * G
        out["m" + name], out["v" + name] = m, v
    assert all(a.dtype == F for a in out.values())
    return out


# ---- the mutants -------------------------------------------------------------------------------------------------------------------------------
def _model(c, pop, lr, mut=None):
    """The reference's formulas once more in float64 with one switch per mutant; _model(c, pop, lr, None) is reference(c, pop, lr) (asserted by
    tests/test_train_parity_host.py), so a mutant differs from the reference by its defect alone."""
    pp, pn = c.heads(pop)
    U, I = c.U.astype(np.float64), c.I.astype(np.float64)
    ue, pe, ne = U[c.users], I[c.pos], I[c.neg]
    ps, ns = (ue * pe).sum(1), (ue * ne).sum(1)
    B = c.B
    if pop:
        qp, qn = pp.astype(np.float64), (pp if mut == "neg_pop_is_pos_pop" else pn).astype(np.float64)
        elu1 = (lambda s: s + 1.0) if mut == "elu_branch_at_ge" else po.elu_plus_one
        de = (lambda s: np.ones_like(s)) if mut == "elu_grad_one" else (lambda s: np.where(s > 0, 1.0, np.exp(np.minimum(s, 0.0))))
        psw, nsw = elu1(ps) * qp, elu1(ns) * qn
        a_p, a_n = (de(ps), de(ns)) if mut == "pop_missing_in_grad" else (qp * de(ps), qn * de(ns))
    else:
        psw, nsw, a_p, a_n = ps, ns, np.ones(B), np.ones(B)
    x = psw - nsw
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        s = 1.0 / (1.0 + np.exp(-x))
        inv_B = 1.0 / ((c.mean_div + 1) if mut == "mean_over_wrong_B" else c.mean_div)
        mf = -inv_B * np.log(s + 1e-10).sum()
        g = -inv_B * s * (1.0 - s) / (s if mut == "no_eps" else s + 1e-10)
    cc = c.regs / c.reg_div
    reg = cc * (1.0 if mut == "reg_loss_without_half" else 0.5) * ((ue ** 2).sum() + (pe ** 2).sum() + (ne ** 2).sum())
    l2 = {"no_l2_grad": 0.0, "l2_twice": 2.0}.get(mut, 1.0) * cc
    k = 1.0 + 1e-3 if mut == "scale_1e-3" else 1.0
    sgn = 1.0 if mut == "neg_row_sign" else -1.0
    due = k * ((g * a_p)[:, None] * pe - (g * a_n)[:, None] * ne + l2 * ue)
    dpe = k * ((g * a_p)[:, None] * ue + l2 * pe)
    dne = k * (sgn * (g * a_n)[:, None] * ue + l2 * ne)
    if mut is None:
        return _finish(c, (mf + reg, mf, reg), due, dpe, dne, lr)
    nU, nI = U.shape[0], I.shape[0]
    gU, gI = np.zeros((nU, c.d)), np.zeros((nI, c.d))
    if mut == "dup_last_wins":
        gU[c.users] = due                    # numpy's fancy assignment: the last occurrence stays
        gI[np.concatenate([c.pos, c.neg])] = np.concatenate([dpe, dne])
    else:
        gU, gI = po.dense_grads(nU, nI, c.users, c.pos, c.neg, due, dpe, dne)
    out = dict(loss=np.array([mf + reg, mf, reg]), due=due, dpe=dpe, dne=dne, gU=gU, gI=gI,
               U_sgd=c.Um.astype(np.float64) - (0.0 if mut == "user_row_not_updated" else lr) * gU, I_sgd=c.Im.astype(np.float64) - lr * gI)
    for n, G in (("U", gU), ("I", gI)):
        out["m" + n] = (1.0 if mut == "m_without_1mb1" else 0.1) * G
        out["v" + n] = 0.001 * (G if mut == "v_from_g_not_g2" else G * G)
    return out


def mutant(c, pop, name, lr=0.05):
    assert name in MUTANTS
    return _model(c, pop, lr, name)


GRADS = ("due", "dpe", "dne", "gU", "gI", "U_sgd", "I_sgd", "mU", "vU", "mI", "vI")
ALL = "all"
# name -> changes: the quantities the defect moves; kinds: where it shows; case: (d, B, kind, pop) of the GPU list on which
# |mutant - reference| > 10 bound holds on every changed quantity; everywhere: the changed quantities of which the defect touches every
# element of the batch's rows (ALL: each of them)
MUTANTS = {
    "no_l2_grad": dict(changes=GRADS, kinds=KINDS, case=(64, 101, "spread", True), everywhere=ALL),
    "l2_twice": dict(changes=GRADS, kinds=KINDS, case=(64, 101, "spread", True), everywhere=ALL),
    "scale_1e-3": dict(changes=GRADS, kinds=KINDS, case=(64, 1, "spread", False), everywhere=ALL),
    "no_eps": dict(changes=("due", "dpe", "dne", "gU", "gI", "U_sgd", "I_sgd", "mU", "vU", "mI", "vI"), kinds=("saturated",),
                   case=(64, 33, "saturated", True), everywhere=()),
    "elu_grad_one": dict(changes=GRADS, kinds=("negative_dots", "spread", "hot", "unshared"), case=(128, 17, "negative_dots", True), everywhere=()),
    "elu_branch_at_ge": dict(changes=("loss",) + GRADS, kinds=("negative_dots", "spread", "hot", "unshared"), case=(128, 17, "negative_dots", True),
                             everywhere=()),
    "neg_pop_is_pos_pop": dict(changes=("loss",) + GRADS, kinds=KINDS, case=(32, 65, "spread", True), everywhere=()),
    "pop_missing_in_grad": dict(changes=GRADS, kinds=KINDS, case=(32, 65, "spread", True), everywhere=()),
    "mean_over_wrong_B": dict(changes=("loss",) + GRADS, kinds=KINDS, case=(256, 7, "spread", False), everywhere=ALL),
    "dup_last_wins": dict(changes=("gU", "gI", "U_sgd", "I_sgd", "mU", "vU", "mI", "vI"), kinds=("spread", "hot", "negative_dots", "saturated"),
                          case=(64, 101, "hot", True), everywhere=()),
    "user_row_not_updated": dict(changes=("U_sgd",), kinds=KINDS, case=(128, 53, "unshared", True), everywhere=("U_sgd",)),
    "neg_row_sign": dict(changes=("dne", "gI", "I_sgd", "mI", "vI"), kinds=KINDS, case=(32, 63, "spread", False), everywhere=("dne",)),
    "reg_loss_without_half": dict(changes=("loss",), kinds=KINDS, case=(64, 2048, "spread", True), everywhere=()),
    "v_from_g_not_g2": dict(changes=("vU", "vI"), kinds=KINDS, case=(64, 33, "hot", True), everywhere=ALL),
    "m_without_1mb1": dict(changes=("mU", "mI"), kinds=KINDS, case=(64, 33, "hot", True), everywhere=ALL),
}
