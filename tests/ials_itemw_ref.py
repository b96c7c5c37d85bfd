"""float64 restatement of item-weighted iALS (include/pda_hip_ials_itemw.h) in numpy: the weights, the objective, both sides of
both solvers, the fp32-order emulation of the scaled Gram matrix and of the row systems that the exact tests compare bit for bit, and the
a-priori bounds the GPU suite holds the kernels to.  Nothing here calls the library; everything that the unweighted model already has comes
from tests/ials_ref.py and tests/ialspp_ref.py.

As there, the parameters of a call are what the kernels receive: fp32 tables, alpha0 rounded to fp32, lam_row fp32, and the two new inputs
scale (s, fp32 [n_items]) and alpha_row (fp32 [n_items]); "exact" means exact arithmetic on those inputs.  The two sides of the model then
see weights that differ by one rounding: the user side weighs item i by alpha32(alpha0) float64(s_i)^2, the item side by float64(alpha_row[i])
= fl32(alpha0 w_i).  `user_item_alpha` and `item_alpha` name the two; the objective the GPU suite follows is written in the first.
"""
import numpy as np

import ials_ref as ir
import ialspp_ref as pr
from ials_ref import CHUNK, GRAM_ROWS, U32, alpha32, gamma

ITEM_POWER_MAX = 4.0


# ---- the weights ------------------------------------------------------------------------------------------------------------------------------
def item_weights(counts, beta, alpha0):
    """q = (c + 1)^beta / sum, float64; s = fl32(sqrt(n q)); w = float64(s)^2; alpha_row = fl32(alpha0 w) -> dict(q, s, w, alpha_row)."""
    p = (np.asarray(counts, dtype=np.float64) + 1.0) ** float(beta)
    q = p / p.sum()
    s = np.sqrt(float(len(q)) * q).astype(np.float32)
    w = s.astype(np.float64) ** 2
    return dict(q=q, s=s, w=w, alpha_row=(float(alpha0) * w).astype(np.float32))


def lam_row_items(deg, n_users, lam, alpha0, nu, w):
    """fl32(lambda * float64(n_i + alpha0 w_i n_users)^nu)."""
    return (float(lam) * np.power(np.asarray(deg, dtype=np.float64) + float(alpha0) * np.asarray(w, dtype=np.float64) * n_users, float(nu))).astype(np.float32)


def user_item_alpha(alpha0, s):
    """The weight of item i as the user side and the loss see it: alpha32(alpha0) float64(s_i)^2."""
    return alpha32(alpha0) * np.asarray(s, dtype=np.float32).astype(np.float64) ** 2


def item_alpha(alpha_row):
    """The weight of item i as the item side sees it: float64(alpha_row[i])."""
    return np.asarray(alpha_row, dtype=np.float32).astype(np.float64)


# ---- the model --------------------------------------------------------------------------------------------------------------------------------
def objective(X, Y, eu, ei, a_items, lam_u, lam_i):
    """L(X, Y) in float64 -> (L, fit, reg), a_items [n_items] the weight alpha0 w_i of item i's pairs:
    fit = sum_S (x.y - 1)^2 + sum_u sum_i a_i (x_u.y_i)^2, the second computed as sum((X^T X) * (Y^T diag(a) Y))."""
    X, Y, a = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64), np.asarray(a_items, dtype=np.float64)
    s = np.einsum("ij,ij->i", X[eu], Y[ei])
    fit = ((s - 1.0) ** 2).sum() + np.sum((X.T @ X) * (Y.T @ (a[:, None] * Y)))
    reg = (np.asarray(lam_u, dtype=np.float64) * (X * X).sum(1)).sum() + (np.asarray(lam_i, dtype=np.float64) * (Y * Y).sum(1)).sum()
    return fit + reg, fit, reg


def gram_w(Y, s):
    """G_w = sum_i (s_i y_i)(s_i y_i)^T exactly (float64 on the inputs)."""
    Ys = np.asarray(Y, dtype=np.float64) * np.asarray(s, dtype=np.float32).astype(np.float64)[:, None]
    return Ys.T @ Ys


def user_half_sweep(up, ui, Y, s, alpha0, lam_u, rows=None):
    """x_u = (alpha0 G_w + sum y y^T + lam_u I)^-1 sum y: ials_ref's row solve handed G_w."""
    Y = np.asarray(Y, dtype=np.float64)
    Gw = gram_w(Y, s)
    n = len(up) - 1
    X = np.full((n, Y.shape[1]), np.nan)
    for r in (range(n) if rows is None else rows):
        A, b = ir.normal_equations(up, ui, Y, alpha0, lam_u, r, Gw)
        X[r] = np.linalg.solve(A, b)
    return X


def item_half_sweep(ip, ii, X, alpha_row, lam_i, rows=None):
    """y_i = (alpha_i G + sum x x^T + lam_i I)^-1 sum x with G = X^T X and alpha_i = float64(alpha_row[i])."""
    X = np.asarray(X, dtype=np.float64)
    G = X.T @ X
    n = len(ip) - 1
    Y = np.full((n, X.shape[1]), np.nan)
    for r in (range(n) if rows is None else rows):
        A, b = ir.normal_equations(ip, ii, X, float(alpha_row[r]), lam_i, r, G)
        Y[r] = np.linalg.solve(A, b)
    return Y


def epoch(X, Y, up, ui, ip, ii, alpha0, s, alpha_row, lam_u, lam_i):
    """The exact solver's epoch: the user half-sweep against G_w, then the item half-sweep with alpha_row -> (X', Y') float64."""
    X1 = user_half_sweep(up, ui, Y, s, alpha0, lam_u)
    return X1, item_half_sweep(ip, ii, X1, alpha_row, lam_i)


def block_pass(X, e, indptr, indices, pos, Z, alpha, lam, p0, k, scale=None, rows=None):
    """ialspp_ref.block_pass of the weighted model: scale given (the user side) -> G = G_w and alpha the scalar alpha0; scale None (the item
    side) -> G = Z^T Z and alpha the fp32 vector alpha_row (a scalar is let through: the unweighted pass)."""
    X, e, Z = np.array(X, dtype=np.float64), np.array(e, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    G = Z.T @ Z if scale is None else gram_w(Z, scale)
    for r in (range(len(indptr) - 1) if rows is None else rows):
        a, b = int(indptr[r]), int(indptr[r + 1])
        where = np.arange(a, b) if pos is None else pos[a:b]
        X[r], e[where], _ = pr.block_step(X[r], e[where], Z[indices[a:b]], G, _alpha_of(alpha, r), lam[r], p0, k)
    return X, e


def block_epoch(X, Y, up, ui, ip, ii, alpha0, s, alpha_row, lam_u, lam_i, k):
    """One iALS++ epoch of the weighted model -> (X', Y', e') float64."""
    X, Y = np.array(X, dtype=np.float64), np.array(Y, dtype=np.float64)
    perm = pr.pair_perm(up, ui, ip, ii)
    e = pr.predictions(X, Y, up, ui)
    for p0 in range(0, X.shape[1], k):
        X, e = block_pass(X, e, up, ui, None, Y, alpha0, lam_u, p0, k, scale=s)
        Y, e = block_pass(Y, e, ip, ii, perm, X, alpha_row, lam_i, p0, k)
    return X, Y, e


def _alpha_of(alpha, r):
    return float(alpha) if np.ndim(alpha) == 0 else float(np.asarray(alpha)[r])


# ---- the stated order in fp32 -------------------------------------------------------------------------------------------------------------------
def scaled32(Z32, s32):
    """z'_c[j] = fl(s_c z_c[j]): one fp32 multiplication per element."""
    return (np.asarray(Z32, dtype=np.float32) * np.asarray(s32, dtype=np.float32)[:, None]).astype(np.float32)


def gram_scaled32(Z32, s32):
    """G_w in the stated order: the chains of ials_ref.gram32 on the scaled rows."""
    return ir.gram32(scaled32(Z32, s32))


def normal32(indptr, indices, Z32, G32, alpha_row32, lam, r, chunk=CHUNK):
    """(A_r, b_r) fp32 in the stated order with the row's own alpha: ials_ref.normal32 reads alpha as a scalar, here it is alpha_row32[r]."""
    return ir.normal32(indptr, indices, Z32, G32, np.float32(alpha_row32[r]), lam, r, chunk)


def system32(indptr, indices, pos, Z32, G32, x32, e32, alpha_row32, lam, r, p0, k, chunk=CHUNK):
    """(H_r, g_r) fp32 in the stated order with the row's own alpha (ialspp_ref.system32 with alpha_row32[r] for the scalar)."""
    return pr.system32(indptr, indices, pos, Z32, G32, x32, e32, np.float32(alpha_row32[r]), lam, r, p0, k, chunk)


# ---- the a-priori bound of a row's solution ----------------------------------------------------------------------------------------------------
# ials_ref.row_bounds with the two changes of the weighted model; its derivation stands as it is written there.
#   scale given (the user side): G is G_w, exact on the inputs (s, Z).  An entry of the computed G_w is the chain of ials_ref over products
#     fl(s z_i) fl(s z_j): each factor carries one more rounding, (1 + d1)(1 + d2), so the Gram term takes gamma_{GRAM_ROWS + NB + 3 + 2} on
#     P_all = |diag(s) Z|^T |diag(s) Z|.  Nothing else changes: b and the sum over S_r read the unscaled rows.
#   alpha a vector (the item side): row r reads alpha[r] where it read the scalar -- an input, so no new error.
# dZ (the propagated error of the half-sweep before) is taken as in ials_ref; it is supported on the unscaled side only, which is where the
# epoch test needs it (the item side reads the X the user side wrote).
def row_bounds(indptr, indices, Z, alpha, lam, rows, scale=None, chunk=CHUNK, dZ=None):
    Z = np.asarray(Z, dtype=np.float64)
    n, d = Z.shape
    assert scale is None or dZ is None
    sc = np.ones(n) if scale is None else np.asarray(scale, dtype=np.float32).astype(np.float64)
    Zs = Z * sc[:, None]
    G = Zs.T @ Zs
    Zabs = np.abs(Z) if dZ is None else np.abs(Z) + np.asarray(dZ, dtype=np.float64)[:, None]
    Zsabs = Zabs * sc[:, None]
    P_all = Zsabs.T @ Zsabs
    nb = -(-n // GRAM_ROWS)
    g_gram = gamma(GRAM_ROWS + nb + 3 + (0 if scale is None else 2))
    eta_solve = d * gamma(3 * d + 1) / (1.0 - d * gamma(d + 1))
    if dZ is not None:
        dz = np.asarray(dZ, dtype=np.float64)
        dG1 = 2.0 * np.linalg.norm(Z, 2) * np.linalg.norm(dz) + np.linalg.norm(dz) ** 2
    out = {k: np.zeros(len(rows)) for k in ("kappa", "eta", "bound", "xnorm", "lmax", "lmin")}
    X = np.zeros((len(rows), d))
    for t, r in enumerate(rows):
        a0 = alpha32(_alpha_of(alpha, r))
        cols = indices[indptr[r]:indptr[r + 1]]
        nr = len(cols)
        C = max(1, -(-nr // chunk))
        A, b = ir.normal_equations(indptr, indices, Z, a0, lam, r, G)
        za = Zabs[cols]
        E = gamma(min(nr, chunk) + C + 2) * (za.T @ za) + g_gram * a0 * P_all + gamma(2) * float(lam[r]) * np.eye(d)
        sv = np.linalg.svd(A, compute_uv=False)
        eta_form = np.linalg.norm(E, 2) / sv[0]
        eta_b, prop = 0.0, 0.0
        bn = np.linalg.norm(b)
        if nr:
            eta_b = gamma(min(nr, chunk) + C) * np.linalg.norm(za.sum(0)) / bn
            if dZ is not None:
                zn = np.linalg.norm(Z[cols], axis=1)
                prop = (a0 * dG1 + np.sum(2.0 * zn * dz[cols] + dz[cols] ** 2)) / sv[0] + dz[cols].sum() / bn
        elif dZ is not None:
            prop = a0 * dG1 / sv[0]
        eta = eta_form + (1.0 + eta_form) * eta_solve + eta_b + prop
        kappa = sv[0] / sv[-1]
        X[t] = np.linalg.solve(A, b)
        out["kappa"][t], out["eta"][t], out["lmax"][t], out["lmin"][t], out["xnorm"][t] = kappa, eta, sv[0], sv[-1], np.linalg.norm(X[t])
        out["bound"][t] = kappa * eta / (1.0 - kappa * eta) if kappa * eta < 1.0 else np.inf
    out["x"] = X
    return out


# ---- the a-priori bound of a block pass ---------------------------------------------------------------------------------------------------------
# ialspp_ref.pass_bounds of the weighted model, row by row through ialspp_ref.step_bounds, whose derivation stands as written there.
#   scale given (the user side): G = G_w and P_all = |diag(s) Z|^T |diag(s) Z|; the two more roundings of the scaled rows enter by handing
#     step_bounds P_all (1 + 2 / n) (1 - n u) / (1 - (n + 2) u) with n = GRAM_ROWS + NB + 3: gamma_n times that is gamma_{n + 2} P_all in
#     H, and in g, where the Gram term's gamma_m has m > n, gamma_m (1 + 2 / n) >= gamma_{m + 2}.  The error of the table held fixed (dz) is not
#     supported with a scale: a pass is held from the state the kernels left, as the unweighted suite holds it.
#   alpha a vector (the item side): row r reads alpha[r], an input.
def pass_bounds(X, e, indptr, indices, pos, Z, alpha, lam, p0, k, scale=None, rows=None, chunk=CHUNK, dz=None, dX=None, de=None):
    X, e, Z = np.array(X, dtype=np.float64), np.array(e, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    n, n_z = len(indptr) - 1, Z.shape[0]
    assert scale is None or dz is None
    sc = np.ones(n_z) if scale is None else np.asarray(scale, dtype=np.float32).astype(np.float64)
    Zs = Z * sc[:, None]
    G = Zs.T @ Zs
    Zabs = np.abs(Z) if dz is None or not np.isfinite(dz).all() else np.abs(Z) + np.asarray(dz, dtype=np.float64)[:, None]
    P_all = (Zabs * sc[:, None]).T @ (Zabs * sc[:, None])
    if scale is not None:
        m = GRAM_ROWS + -(-n_z // GRAM_ROWS) + 3
        P_all = P_all * (gamma(m + 2) / gamma(m))
    Znorm = np.linalg.norm(Z, 2)
    dX = np.zeros(n) if dX is None else np.array(dX, dtype=np.float64)
    de = np.zeros(len(e)) if de is None else np.array(de, dtype=np.float64)
    out = dict(err=np.zeros(n), lmax=np.zeros(n), lmin=np.zeros(n), xnorm=np.zeros(n), delta_norm=np.zeros(n), drift=np.array(de, dtype=np.float64))
    for r in (range(n) if rows is None else rows):
        a, b = int(indptr[r]), int(indptr[r + 1])
        where = np.arange(a, b) if pos is None else pos[a:b]
        s = pr.step_bounds(X[r], e[where], indices[a:b], Z, G, P_all, _alpha_of(alpha, r), lam[r], p0, k, chunk, dz, dX[r], de[where], Znorm)
        zn = np.linalg.norm(Z[indices[a:b]][:, p0:p0 + k], axis=1)
        out["drift"][where] = pr.cache_drift_bound(de[where], zn, np.linalg.norm(X[r, p0:p0 + k]), np.linalg.norm(s["delta"]), s["err"],
                                                   np.abs(s["e"]) + s["de"], k)
        out["xnorm"][r] = np.linalg.norm(X[r])
        X[r], e[where], dX[r], de[where] = s["x"], s["e"], s["dx"], s["de"]
        out["err"][r], out["lmax"][r], out["lmin"][r], out["delta_norm"][r] = s["err"], s["lmax"], s["lmin"], np.linalg.norm(s["delta"])
    out.update(X=X, e=e, dX=dX, de=de)
    return out


# ---- what a step may raise the objective by ----------------------------------------------------------------------------------------------------------
# The unweighted suites allow a half-sweep (a pass) sum_r lambda_max(A_r) err_r^2: the objective is quadratic in the rows being solved, with
# its minimum at the exact row solutions and Hessian A_r, and err_r bounds the distance of the computed row from that minimum.  The user side
# of the weighted model is exactly that, at the objective's own weights.  The item side is handed alpha_row[i] = fl32(alpha0 w_i) where the
# objective (written in the user side's weights) has a_i = alpha32(alpha0) s_i^2: its exact row solution is the minimiser of a system that
# differs by dA = da_i G (block: dH = da_i G[pi, pi], dg = da_i G[pi, :] y), |da_i| <= u a_i.  From A' x' = b, A x = b:
#     |x - x'| <= |da| |G|_2 |x| / (lambda_min - |da| |G|_2)       (block: |delta - delta'| <= |da| |G|_2 (|y| + |delta|) / (lambda_min - |da| |G|_2))
# so the distance from the objective's minimum is at most err + that, under a Hessian of at most lambda_max + |da| |G|_2.  |G|_2 bounds the norm
# of every submatrix of G.  The extra term is of the order of u: far below err, but not nothing.
def item_allowance(lmax, lmin, err, da, Gnorm, xnorm, delta_norm=None):
    shift = np.abs(da) * Gnorm
    assert (lmin > shift).all()
    moved = shift * (xnorm if delta_norm is None else xnorm + delta_norm) / (lmin - shift)
    return float(np.sum((lmax + shift) * (err + moved) ** 2))


# ---- the a-priori bound of the objective's sums ----------------------------------------------------------------------------------------------------
# ials_ref.loss_bound with G_w for G: P_all = |diag(s) Y|^T |diag(s) Y| and two more roundings in the Gram term (the scaled rows), gamma_{GRAM_ROWS +
# NB + 2 d + 1 + 2}; every other term is as derived there.  The reference is objective() at a_items = user_item_alpha(alpha0, s).
def loss_bound(X, Y, up, ui, alpha0, s, lam_u, L):
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    d = X.shape[1]
    Ysa = np.abs(Y) * np.asarray(s, dtype=np.float32).astype(np.float64)[:, None]
    P_all = Ysa.T @ Ysa
    nb = -(-Y.shape[0] // GRAM_ROWS)
    total = 0.0
    for r in range(X.shape[0]):
        cols = ui[up[r]:up[r + 1]]
        nr = len(cols)
        x = X[r]
        if nr:
            rc = Y[cols] @ x - 1.0
            e = gamma(d) * (np.abs(Y[cols]) @ np.abs(x))
            D = (1.0 + U32) * e + U32 * np.abs(rc)
            total += (1.0 + gamma(nr + 1)) * np.sum((2.0 * np.abs(rc) + D) * D) + gamma(nr + 1) * np.sum(rc ** 2)
        total += alpha32(alpha0) * gamma(GRAM_ROWS + nb + 2 * d + 1 + 2) * (np.abs(x) @ P_all @ np.abs(x))
        total += gamma(d + 1) * float(lam_u[r]) * (x @ x)
    return total + 1e-12 * abs(L)


# ---- the inputs the GPU suite and the host suite share ---------------------------------------------------------------------------------------------
BETA = 0.5


def bound_counts(n=ir.N_OTHER):
    """The item counts of the bound tests: floor(2000 / (1 + a permutation of the ids)), Zipf-shaped with the ranks shuffled over the ids."""
    return np.floor(2000.0 / (1.0 + np.random.default_rng(5).permutation(n))).astype(np.int64)


def bound_inputs(alpha0, n_rows=len(ir.ROW_LENGTHS)):
    """The weights of the bound tests on ials_ref.length_graph() at BETA -> dict(s [N_OTHER] for the side solved against G_w; w_rows and
    alpha_rows [n_rows] for the side solved with its own alpha: the weights at n_rows evenly spaced ranks of w, smallest and largest included,
    dealt to the rows in a fixed shuffled order)."""
    iw = item_weights(bound_counts(), BETA, alpha0)
    order = np.argsort(iw["w"], kind="stable")[np.linspace(0, len(iw["w"]) - 1, n_rows).astype(np.int64)]
    pick = order[np.random.default_rng(6).permutation(n_rows)]
    return dict(s=iw["s"], w=iw["w"], w_rows=iw["w"][pick], alpha_rows=iw["alpha_row"][pick])


def pow2_scale(n, seed=3):
    """s in {1/2, 1, 2}: a scaled eighths row is a table of sixteenths, every product a multiple of 1/256."""
    return np.float32(2.0) ** np.random.default_rng(seed).integers(-1, 2, n).astype(np.float32)


def pow2_alpha(n, seed=4):
    """alpha_row in {1/4, 1/2, 1}: fl(alpha G) is exact."""
    return np.float32(2.0) ** np.random.default_rng(seed).integers(-2, 1, n).astype(np.float32)
