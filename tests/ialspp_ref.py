"""float64 restatement of iALS++ (include/pda_hip_ialspp.h) in numpy: the block step, a pass, an epoch and pair_perm, the
fp32-order emulation of (H, g) that the exact test compares bit for bit, and the a-priori error bounds the GPU suite holds the kernels to.
Nothing here calls the library.  The objective, the CSRs, lam_row and the work lists are those of tests/ials_ref.py.

As there, the parameters of a call are what the kernels receive: fp32 tables, an fp32 prediction cache, alpha0 rounded to fp32, lam_row fp32;
"exact" means exact arithmetic on those inputs.
"""
import numpy as np

import ials_ref as ir
from ials_ref import CHUNK, GRAM_ROWS, U32, alpha32, gamma

EMBED_SIZES = (32, 64, 128, 256)
BLOCK_SIZES = (32, 64, 128)


def parts(k):
    """The number of parts the product G[pi, :] x is cut into (the header: 2 at k = 32 or 128, 4 at k = 64)."""
    return {32: 2, 64: 4, 128: 2}[k]


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
def pair_perm(up, ui, ip, ii):
    """perm[q] = the position in the user CSR (up, ui) of the pair at position q of the item CSR (ip, ii), by plain loops and a dictionary."""
    where = {}
    for u in range(len(up) - 1):
        for p in range(int(up[u]), int(up[u + 1])):
            where[(u, int(ui[p]))] = p
    perm = np.zeros(len(ii), dtype=np.int64)
    for i in range(len(ip) - 1):
        for q in range(int(ip[i]), int(ip[i + 1])):
            perm[q] = where[(int(ii[q]), i)]
    return perm


def predictions(X, Y, up, ui):
    """e[p] = x_u(p) . y_i(p) in the user CSR's pair order, float64."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    rows = np.repeat(np.arange(len(up) - 1), np.diff(up))
    return np.einsum("ij,ij->i", X[rows], Y[ui])


def block_system(x, e_row, Zr, G, alpha0, lam_r, p0, k):
    """(H, g) of one block step, exactly: x the row [d], e_row its cached predictions, Zr its partners' rows [n_r, d], G = Z^T Z."""
    x, Zr = np.asarray(x, dtype=np.float64), np.asarray(Zr, dtype=np.float64)
    a0, zs = alpha32(alpha0), Zr[:, p0:p0 + k]
    H = zs.T @ zs + a0 * G[p0:p0 + k, p0:p0 + k] + float(lam_r) * np.eye(k)
    g = zs.T @ (np.asarray(e_row, dtype=np.float64) - 1.0) + a0 * (G[p0:p0 + k, :] @ x) + float(lam_r) * x[p0:p0 + k]
    return H, g


def block_step(x, e_row, Zr, G, alpha0, lam_r, p0, k):
    """One block step -> (x', e_row', delta)."""
    H, g = block_system(x, e_row, Zr, G, alpha0, lam_r, p0, k)
    delta = np.linalg.solve(H, g)
    x1 = np.array(x, dtype=np.float64)
    x1[p0:p0 + k] -= delta
    return x1, np.asarray(e_row, dtype=np.float64) - np.asarray(Zr, dtype=np.float64)[:, p0:p0 + k] @ delta, delta


def block_pass(X, e, indptr, indices, pos, Z, alpha0, lam, p0, k, rows=None):
    """One pass of the block over the given rows (default: all) -> (X', e') as float64 copies; pos: CSR position -> position in e (None: the
    identity, the user side)."""
    X, e, Z = np.array(X, dtype=np.float64), np.array(e, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    G = Z.T @ Z
    for r in (range(len(indptr) - 1) if rows is None else rows):
        a, b = int(indptr[r]), int(indptr[r + 1])
        where = np.arange(a, b) if pos is None else pos[a:b]
        X[r], e[where], _ = block_step(X[r], e[where], Z[indices[a:b]], G, alpha0, lam[r], p0, k)
    return X, e


def epoch(X, Y, up, ui, ip, ii, alpha0, lam_u, lam_i, k):
    """One iALS++ epoch: e from the tables; for each block ascending the user pass, then the item pass -> (X', Y', e') float64."""
    X, Y = np.array(X, dtype=np.float64), np.array(Y, dtype=np.float64)
    perm = pair_perm(up, ui, ip, ii)
    e = predictions(X, Y, up, ui)
    for p0 in range(0, X.shape[1], k):
        X, e = block_pass(X, e, up, ui, None, Y, alpha0, lam_u, p0, k)
        Y, e = block_pass(Y, e, ip, ii, perm, X, alpha0, lam_i, p0, k)
    return X, Y, e


# ---- the stated order in fp32 -----------------------------------------------------------------------------------------------------------------
def _chain32(zs32, w32):
    """sum z z^T and sum w z over the given fp32 slices in order onto zero, one rounding per term (the fmaf chains of the header; see
    ials_ref._chain32 for why a float64 sum rounded to fp32 stands for fmaf on the exact test's inputs)."""
    k = zs32.shape[1]
    H, g = np.zeros((k, k), dtype=np.float32), np.zeros(k, dtype=np.float32)
    for z, w in zip(zs32, w32):
        z64 = z.astype(np.float64)
        H = (H.astype(np.float64) + np.outer(z64, z64)).astype(np.float32)
        g = (g.astype(np.float64) + float(w) * z64).astype(np.float32)
    return H, g


def system32(indptr, indices, pos, Z32, G32, x32, e32, alpha0, lam, r, p0, k, chunk=CHUNK):
    """(H_r, g_r) fp32 in the order the header states: w = fl(e - 1); the chunks' chains, the chunks in order onto zero; H = fl(fl(S + fl(alpha0
    G[pi, pi])) + lam on the diagonal); t in parts(k) chains over consecutive columns, the parts in order onto zero; g = fl(fl(s + fl(alpha0 t)) +
    fl(lam x_pi))."""
    d = Z32.shape[1]
    a, b = int(indptr[r]), int(indptr[r + 1])
    where = np.arange(a, b) if pos is None else pos[a:b]
    zs = Z32[indices[a:b]][:, p0:p0 + k]
    w = (e32[where] - np.float32(1.0)).astype(np.float32)
    if b - a <= chunk:
        S, s = _chain32(zs, w)
    else:
        S, s = np.zeros((k, k), dtype=np.float32), np.zeros(k, dtype=np.float32)
        for c in range(0, b - a, chunk):
            Sc, sc = _chain32(zs[c:c + chunk], w[c:c + chunk])
            S, s = (S + Sc).astype(np.float32), (s + sc).astype(np.float32)
    a0, lam_r = np.float32(alpha0), np.float32(lam[r])
    H = (S + (a0 * G32[p0:p0 + k, p0:p0 + k]).astype(np.float32)).astype(np.float32)
    H[np.diag_indices(k)] = (H[np.diag_indices(k)] + lam_r).astype(np.float32)
    Q = parts(k)
    seg = d // Q
    t = np.zeros(k, dtype=np.float32)
    for q in range(Q):
        tq = np.zeros(k, dtype=np.float32)
        for j in range(q * seg, (q + 1) * seg):
            tq = (tq.astype(np.float64) + G32[j, p0:p0 + k].astype(np.float64) * float(x32[j])).astype(np.float32)
        t = (t + tq).astype(np.float32)
    g = ((s + (a0 * t).astype(np.float32)).astype(np.float32) + (lam_r * x32[p0:p0 + k]).astype(np.float32)).astype(np.float32)
    return H, g


# ---- the inputs of the exact test ----------------------------------------------------------------------------------------------------------------------
def exact_inputs(d, n_rows, n_other, seed=2):
    """The exact test's tables: eighths tables and a dyadic lam_row.  The table being solved holds -1/8, 0 and 1/8 only: G x is a sum over all
    d coordinates of entries as large as n_other / 4, and at d = 256 over the 8 232 rows of the GPU test the full range of ials_ref.eighths_table
    would leave the sum of its absolute terms above 2^24 grid units (exact_headroom)."""
    g = np.random.default_rng(seed)
    Z = ir.eighths_table(n_other, d, seed)
    X = (np.random.default_rng(seed + 1).integers(-1, 2, (n_rows, d)) / 8.0).astype(np.float32)
    lam = (np.arange(n_rows) % 5 * 0.25 + 0.5).astype(np.float32)
    return Z, X, lam, g


def exact_headroom(indptr, indices, Z, X, e, a0, lam, p0, k):
    """The largest sum of absolute values of the terms of any entry of (H, g), in units of the finest grid any partial sum lives on: below
    2^24 every partial sum of every order is exactly representable in fp32.  Grids: z z' 1/64, alpha0 G 1/256 (alpha0 a multiple of 1/4),
    (e - 1) z 1/32, G x 1/512, alpha0 G x 1/2048, lam x 1/32."""
    Za, Xa = np.abs(Z.astype(np.float64)), np.abs(X.astype(np.float64))
    Pall = Za.T @ Za
    worst = 0.0
    for r in range(len(indptr) - 1):
        cols = indices[indptr[r]:indptr[r + 1]]
        za = Za[cols][:, p0:p0 + k]
        H = za.T @ za + a0 * Pall[p0:p0 + k, p0:p0 + k] + lam[r]
        g = za.T @ np.abs(e[indptr[r]:indptr[r + 1]].astype(np.float64) - 1.0) + a0 * (Pall[p0:p0 + k] @ Xa[r]) + lam[r] * Xa[r, p0:p0 + k]
        worst = max(worst, H.max() * 256, g.max() * 2048, (Pall[p0:p0 + k] @ Xa[r]).max() * 512)
    return worst


# ---- the a-priori bound of a block step ---------------------------------------------------------------------------------------------------------
# The computed delta^ solves (H + dH) delta^ = g + dg exactly, (H, g) the exact system of the reference inputs.  From delta^ - delta =
# H^-1 (dg - dH delta^):
#     |delta^ - delta|_2  <=  (|dg|_2 + |dH|_2 |delta|_2) / (lambda_min(H) - |dH|_2)                                   =: err
# an ABSOLUTE bound: near convergence g cancels to almost nothing, so nothing here is relative to |g|.
# (1) Forming, with the rule of ials_ref.row_bounds (a sum of n terms in any order, one rounding per operation: gamma_n sum |terms|; an fmaf
#     chain rounds less).  With n_c = min(n_r, CHUNK), C chunks, NB Gram blocks and Q parts:
#       H_ij:  gamma_{n_c + C + 2} P_r[i, j]  +  gamma_{GRAM_ROWS + NB + 3} alpha0 P_all[pi, pi][i, j]  +  gamma_2 lam_r on the diagonal
#       g_i:   w_c = fl(e_c - 1) is one more rounding per term:   gamma_{n_c + C + 3} sum_c |e_c - 1| |z_c[i]|
#              t = G[pi, :] x with G as computed, its chains, its parts, the product by alpha0, the two final additions:
#                                                                 gamma_{GRAM_ROWS + NB + d / Q + Q + 3} alpha0 (P_all[pi, :] |x|)[i]
#              lam_r x_i: the product and the last addition:      gamma_2 lam_r |x_i|
#     P_r = sum_c |z_{c,pi}| |z_{c,pi}|^T, P_all = |Z|^T |Z|.  The 2-norm of an entrywise bound bounds the 2-norm.
# (2) Solving: Cholesky and two substitutions at width k, as in ials_ref: |dH_solve|_2 <= k gamma_{3k+1} / (1 - k gamma_{k+1}) (|H|_2 + |dH_form|_2).
# (3) Inputs that differ from the reference's (all optional; they are how an epoch's error is carried from pass to pass):
#       dz [n_z]: |z^_c - z_c|_2 per row of Z;  dx: |x^_r - x_r|_2;  de [n_r]: |e^_c - e_c| per pair of the row.  With dG = 2 |Z|_2 |dz|_2 + |dz|_2^2:
#       |dH_in|_2 <= sum_c (2 |z_{c,pi}| dz_c + dz_c^2) + alpha0 dG
#       |dg_in|_2 <= sum_c (de_c (|z_{c,pi}| + dz_c) + |e_c - 1| dz_c) + alpha0 (|G[pi, :]|_2 dx + dG (|x| + dx)) + lam_r dx
#     and the magnitudes of (1) are taken at |Z| + dz, |x| + dx (as |x| entrywise plus dx on every entry) and |e - 1| + de.
# The results: x'_pi = fl(x_pi - delta^): dx' = dx + err + u (|x_pi| + dx + |delta| + err);
#   e'_c = fl(e^_c - dot^), dot^ the k-term product sum (gamma_{k+1}, any order):
#   de'_c = de_c + (|z_{c,pi}| + dz_c) err + dz_c |delta| + gamma_{k+1} (|z_{c,pi}| + dz_c) (|delta| + err) + u (|e'_c| + de_c + (|z_{c,pi}| + dz_c) err)
def step_bounds(x, e_row, cols, Z, G, P_all, alpha0, lam_r, p0, k, chunk=CHUNK, dz=None, dx=0.0, de=None, Znorm=None):
    """One row's block step and its bound -> dict(H, g, delta, x, e, err, dx, de, lmin, lmax).  P_all = (|Z| + dz)^T (|Z| + dz)."""
    Z = np.asarray(Z, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    e_row = np.asarray(e_row, dtype=np.float64)
    n_z, d = Z.shape
    a0, lam_r = alpha32(alpha0), float(lam_r)
    nr = len(cols)
    Zr = Z[cols]
    zs = Zr[:, p0:p0 + k]
    H, g = block_system(x, e_row, Zr, G, alpha0, lam_r, p0, k)
    delta = np.linalg.solve(H, g)
    dzr = np.zeros(nr) if dz is None else np.asarray(dz, dtype=np.float64)[cols]
    der = np.zeros(nr) if de is None else np.asarray(de, dtype=np.float64)
    if not (np.isfinite(dx) and np.isfinite(der).all() and np.isfinite(dzr).all() and (dz is None or np.isfinite(dz).all())):
        x1 = x.copy()                    # a bound that has already run away says nothing about this step either
        x1[p0:p0 + k] -= delta
        inf = np.full(nr, np.inf)
        return dict(H=H, g=g, delta=delta, x=x1, e=e_row - zs @ delta, err=np.inf, dx=np.inf, de=inf, lmin=np.nan, lmax=np.nan, dH=np.inf, dg=np.inf)
    dG = 0.0
    if dz is not None:
        dzn = np.linalg.norm(dz)
        dG = 2.0 * (np.linalg.norm(Z, 2) if Znorm is None else Znorm) * dzn + dzn ** 2
    za = np.abs(zs) + dzr[:, None]
    xa = np.abs(x) + dx
    wa = np.abs(e_row - 1.0) + der
    nb, C, Q = -(-n_z // GRAM_ROWS), max(1, -(-nr // chunk)), parts(k)
    nc = min(nr, chunk)
    E_H = gamma(nc + C + 2) * (za.T @ za) + gamma(GRAM_ROWS + nb + 3) * a0 * P_all[p0:p0 + k, p0:p0 + k] + gamma(2) * lam_r * np.eye(k)
    E_g = gamma(nc + C + 3) * (za.T @ wa) + gamma(GRAM_ROWS + nb + d // Q + Q + 3) * a0 * (P_all[p0:p0 + k, :] @ xa) + gamma(2) * lam_r * xa[p0:p0 + k]
    sv = np.linalg.eigvalsh(H)
    lmin, lmax = float(sv[0]), float(sv[-1])
    dH_form = np.linalg.norm(E_H, 2)
    eta_solve = k * gamma(3 * k + 1) / (1.0 - k * gamma(k + 1))
    zn = np.linalg.norm(zs, axis=1)
    dH = dH_form + (lmax + dH_form) * eta_solve + np.sum(2.0 * zn * dzr + dzr ** 2) + a0 * dG
    dg = np.linalg.norm(E_g) + np.sum(der * (zn + dzr) + np.abs(e_row - 1.0) * dzr) \
        + a0 * (np.linalg.norm(G[p0:p0 + k, :], 2) * dx + dG * (np.linalg.norm(x) + dx)) + lam_r * dx
    dn = float(np.linalg.norm(delta))
    err = (dg + dH * dn) / (lmin - dH) if lmin > dH else np.inf
    x1 = x.copy()
    x1[p0:p0 + k] -= delta
    e1 = e_row - zs @ delta
    dx1 = dx + err + U32 * (np.linalg.norm(x[p0:p0 + k]) + dx + dn + err)
    de1 = der + (zn + dzr) * err + dzr * dn + gamma(k + 1) * (zn + dzr) * (dn + err) + U32 * (np.abs(e1) + der + (zn + dzr) * err)
    return dict(H=H, g=g, delta=delta, x=x1, e=e1, err=err, dx=dx1, de=de1, lmin=lmin, lmax=lmax, dH=dH, dg=dg)


def pass_bounds(X, e, indptr, indices, pos, Z, alpha0, lam, p0, k, rows=None, chunk=CHUNK, dz=None, dX=None, de=None):
    """block_pass with its bounds, row by row -> dict(X, e float64 results; dX [n_rows] and de [nnz] the bounds of the results (the entries of
    rows not listed keep what came in); err [n_rows] the bound of delta, lmax [n_rows], delta_norm [n_rows]; drift [nnz]: cache_drift_bound
    of every pair, meaningful when the reference inputs ARE the stored tables (dz, dX nothing) and de bounds |e^ - x . z|)."""
    X, e, Z = np.array(X, dtype=np.float64), np.array(e, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    n = len(indptr) - 1
    G = Z.T @ Z
    Zabs = np.abs(Z) if dz is None or not np.isfinite(dz).all() else np.abs(Z) + np.asarray(dz, dtype=np.float64)[:, None]
    P_all = Zabs.T @ Zabs
    Znorm = np.linalg.norm(Z, 2)
    dX = np.zeros(n) if dX is None else np.array(dX, dtype=np.float64)
    de = np.zeros(len(e)) if de is None else np.array(de, dtype=np.float64)
    out = dict(err=np.zeros(n), lmax=np.zeros(n), delta_norm=np.zeros(n), drift=np.array(de, dtype=np.float64))
    for r in (range(n) if rows is None else rows):
        a, b = int(indptr[r]), int(indptr[r + 1])
        where = np.arange(a, b) if pos is None else pos[a:b]
        s = step_bounds(X[r], e[where], indices[a:b], Z, G, P_all, alpha0, lam[r], p0, k, chunk, dz, dX[r], de[where], Znorm)
        zn = np.linalg.norm(Z[indices[a:b]][:, p0:p0 + k], axis=1)
        out["drift"][where] = cache_drift_bound(de[where], zn, np.linalg.norm(X[r, p0:p0 + k]), np.linalg.norm(s["delta"]), s["err"],
                                                np.abs(s["e"]) + s["de"], k)
        X[r], e[where], dX[r], de[where] = s["x"], s["e"], s["dx"], s["de"]
        out["err"][r], out["lmax"][r], out["delta_norm"][r] = s["err"], s["lmax"], np.linalg.norm(s["delta"])
    out.update(X=X, e=e, dX=dX, de=de)
    return out


def predict_bound(X, Y, up, ui):
    """|e^ - e| per pair for pda_ialspp_predict_f32: a dot product of d terms, products rounded, any order: gamma_d |x| . |y|."""
    X, Y = np.abs(np.asarray(X, dtype=np.float64)), np.abs(np.asarray(Y, dtype=np.float64))
    rows = np.repeat(np.arange(len(up) - 1), np.diff(up))
    return gamma(X.shape[1]) * np.einsum("ij,ij->i", X[rows], Y[ui])


def epoch_bounds(X32, Y32, up, ui, ip, ii, alpha0, lam_u, lam_i, k, chunk=CHUNK):
    """The restatement's epoch from the fp32 tables, with the bound of every pass carried into the next -> dict(X, Y, e, dX, dY, de).
    Every pass multiplies what it is handed by about sum_c |z_c| / lambda_min(H) (a worst case: every error aligned), so the bound is of use
    for the two passes of k = d -- there it is the bound ials_ref.row_bounds carries from the user side into the item side -- and runs away to
    infinity within four passes.  An epoch of more than one block is therefore held pass by pass, each from the state the kernels left."""
    perm = pair_perm(up, ui, ip, ii)
    X, Y = np.array(X32, dtype=np.float64), np.array(Y32, dtype=np.float64)
    e = predictions(X, Y, up, ui)
    de = predict_bound(X, Y, up, ui)
    dX, dY = np.zeros(X.shape[0]), np.zeros(Y.shape[0])
    for p0 in range(0, X.shape[1], k):
        o = pass_bounds(X, e, up, ui, None, Y, alpha0, lam_u, p0, k, None, chunk, dY if dY.any() else None, dX, de)
        X, e, dX, de = o["X"], o["e"], o["dX"], o["de"]
        o = pass_bounds(Y, e, ip, ii, perm, X, alpha0, lam_i, p0, k, None, chunk, dX, dY, de)
        Y, e, dY, de = o["X"], o["e"], o["dX"], o["de"]
    return dict(X=X, Y=Y, e=e, dX=dX, dY=dY, de=de)


def cache_drift_bound(de, zs_norm, x_block_norm, delta_norm, err, e_new, k):
    """How far a pair's cached prediction can move away from the prediction of the STORED tables in one block step (the reference here is the
    fp32 table the kernel wrote, so the error of delta itself cancels: the same delta^ goes into x and into e).  e'_true - e'^ = (e_true - e^)
    + z_pi . (fl(x_pi - delta^) - (x_pi - delta^)) + (z_pi . delta^ - dot^) + the rounding of the subtraction:
        de' <= de + |z_pi| u (|x_pi| + |delta^|) + gamma_{k+1} |z_pi| |delta^| + u |e'^|,      |delta^| <= |delta| + err."""
    dn = delta_norm + err
    return de + zs_norm * U32 * (x_block_norm + dn) + gamma(k + 1) * zs_norm * dn + U32 * (np.abs(e_new) + de + zs_norm * dn)
