"""float64 restatement of the iALS baseline (include/pda_hip_ials.h) in numpy: the objective, the row-wise half-sweep with
np.linalg.solve, the work list, the chunk-ordered fp32 sums of (A, b) that the exact test compares bit for bit, and the a-priori error
bounds the GPU suite holds the kernels to.  Nothing here calls the library.

The parameters of a call are what the kernels receive: the fp32 tables, alpha0 ROUNDED to fp32 (it crosses the ABI as a float) and lam_row
fp32 [n_rows] (rounded once on the host).  "Exact" below means exact arithmetic on those inputs.
"""
import numpy as np

U32 = 2.0 ** -24          # unit roundoff of fp32
CHUNK = 4096              # PDA_IALS_CHUNK and PDA_IALS_GRAM_ROWS as this restatement states them; the host suite checks them against _lib
GRAM_ROWS = 256


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u) for fp32."""
    k = np.asarray(k, dtype=np.float64)
    return k * U32 / (1.0 - k * U32)


def alpha32(alpha0):
    return float(np.float32(alpha0))


# ---- the model --------------------------------------------------------------------------------------------------------------------------------
def dedup_pairs(users, items, n_items):
    key = np.unique(np.asarray(users, dtype=np.int64) * n_items + np.asarray(items, dtype=np.int64))
    return key // n_items, key % n_items


def csr(rows, cols, n_rows):
    """(indptr int64, indices int32 ascending within a row) of DISTINCT pairs."""
    o = np.lexsort((cols, rows))
    indptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=indptr[1:])
    return indptr, np.asarray(cols)[o].astype(np.int32)


def lam_row(deg, n_other, lam, alpha0, nu):
    """fl32(lambda * float64(n_r + alpha0 n_other)^nu): alpha0 here is the flag's float64 value (the host computes it before rounding)."""
    return (float(lam) * np.power(np.asarray(deg, dtype=np.float64) + float(alpha0) * n_other, float(nu))).astype(np.float32)


def objective(X, Y, eu, ei, alpha0, lam_u, lam_i):
    """L(X, Y) in float64 -> (L, fit, reg): fit = sum_S (x.y - 1)^2 + alpha0 sum_all (x.y)^2, computed as alpha0 tr(X^T X Y^T Y)."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    s = np.einsum("ij,ij->i", X[eu], Y[ei])
    fit = ((s - 1.0) ** 2).sum() + alpha32(alpha0) * np.sum((X.T @ X) * (Y.T @ Y))
    reg = (np.asarray(lam_u, dtype=np.float64) * (X * X).sum(1)).sum() + (np.asarray(lam_i, dtype=np.float64) * (Y * Y).sum(1)).sum()
    return fit + reg, fit, reg


def normal_equations(indptr, indices, Z, alpha0, lam, r, G=None):
    """(A_r, b_r) exactly (float64 on the given inputs)."""
    Z = np.asarray(Z, dtype=np.float64)
    if G is None:
        G = Z.T @ Z
    zr = Z[indices[indptr[r]:indptr[r + 1]]]
    return alpha32(alpha0) * G + zr.T @ zr + float(lam[r]) * np.eye(Z.shape[1]), zr.sum(0)


def half_sweep(indptr, indices, Z, alpha0, lam, rows=None):
    """x_r = A_r^{-1} b_r for every row (or the given ones; the others come back as NaN), float64 [n_rows, d]."""
    Z = np.asarray(Z, dtype=np.float64)
    G = Z.T @ Z
    n = len(indptr) - 1
    X = np.full((n, Z.shape[1]), np.nan)
    for r in (range(n) if rows is None else rows):
        A, b = normal_equations(indptr, indices, Z, alpha0, lam, r, G)
        X[r] = np.linalg.solve(A, b)
    return X


def epoch(X, Y, up, ui, ip, ii, alpha0, lam_u, lam_i):
    """The user half-sweep, then the item half-sweep on its result -> (X', Y') float64."""
    X1 = half_sweep(up, ui, Y, alpha0, lam_u)
    return X1, half_sweep(ip, ii, X1, alpha0, lam_i)


# ---- the work list ----------------------------------------------------------------------------------------------------------------------------
def work_list(indptr, chunk=CHUNK):
    """(work [n_work, 4] = row, first, end, slot; long_rows [n_long, 3] = row, first slot, chunks; n_slots), written as plain loops: rows of
    at most `chunk` pairs whole with slot -1, longer ones in chunks with consecutive slots; sorted by falling length, stable."""
    work, long_rows, slot = [], [], 0
    for r in range(len(indptr) - 1):
        a, b = int(indptr[r]), int(indptr[r + 1])
        if b - a <= chunk:
            work.append((r, a, b, -1))
            continue
        n = -(-(b - a) // chunk)
        long_rows.append((r, slot, n))
        for j in range(n):
            work.append((r, a + j * chunk, min(a + (j + 1) * chunk, b), slot + j))
        slot += n
    work.sort(key=lambda w: -(w[2] - w[1]))
    return np.array(work, dtype=np.int64).reshape(-1, 4), np.array(long_rows, dtype=np.int64).reshape(-1, 3), slot


# ---- the stated order in fp32 -------------------------------------------------------------------------------------------------------------------
def _chain32(rows32):
    """sum z z^T and sum z over the given fp32 rows in order onto zero, one rounding per term (the fmaf chain of the header): the product of two
    fp32 is exact in float64 and the sum is rounded to fp32 -- equal to fmaf wherever the float64 sum is itself exact, which the exact test's
    inputs guarantee (every partial sum is a small multiple of 1/64)."""
    d = rows32.shape[1]
    A, b = np.zeros((d, d), dtype=np.float32), np.zeros(d, dtype=np.float32)
    for z in rows32:
        z64 = z.astype(np.float64)
        A = (A.astype(np.float64) + np.outer(z64, z64)).astype(np.float32)
        b = (b + z).astype(np.float32)
    return A, b


def gram32(Z32):
    """G in the stated order: chains over blocks of GRAM_ROWS rows, the blocks added in order onto zero."""
    d = Z32.shape[1]
    G = np.zeros((d, d), dtype=np.float32)
    for k in range(0, Z32.shape[0], GRAM_ROWS):
        G = (G + _chain32(Z32[k:k + GRAM_ROWS])[0]).astype(np.float32)
    return G


def normal32(indptr, indices, Z32, G32, alpha0, lam, r, chunk=CHUNK):
    """(A_r, b_r) fp32 in the stated order: the chunks' chains, the chunks in order onto zero (a row of one chunk: the chain itself), then
    fl(fl(S + fl(alpha0 G)) + lambda_r on the diagonal)."""
    d = Z32.shape[1]
    a, e = int(indptr[r]), int(indptr[r + 1])
    if e - a <= chunk:
        S, b = _chain32(Z32[indices[a:e]])
    else:
        S, b = np.zeros((d, d), dtype=np.float32), np.zeros(d, dtype=np.float32)
        for k in range(a, e, chunk):
            Sc, bc = _chain32(Z32[indices[k:min(k + chunk, e)]])
            S, b = (S + Sc).astype(np.float32), (b + bc).astype(np.float32)
    A = (S + (np.float32(alpha0) * G32).astype(np.float32)).astype(np.float32)
    A[np.diag_indices(d)] = (A[np.diag_indices(d)] + np.float32(lam[r])).astype(np.float32)
    return A, b


# ---- the a-priori bound of a row's solution -------------------------------------------------------------------------------------------------------
# The computed x^ solves (A + dA) x^ = b + db exactly, A and b the exact normal equations of the inputs.  Then (Higham 2002, Thm 7.2 with
# E = A, f = b, and |b| <= |A| |x|)
#     |x^ - x|_2 / |x|_2  <=  kappa eta / (1 - kappa eta),      kappa = cond_2(A),  eta = |dA|_2 / |A|_2 + |db|_2 / |b|_2.
# dA has two parts.
# (1) Forming A.  Every sum of k terms evaluated in ANY order with one rounding per operation has an error of at most gamma_k sum |terms|
#     (an fmaf chain rounds less, not more).  Entry (i, j):
#       the chunk's chain over n_c <= CHUNK pairs, the C chunks of the row, the two final additions:   gamma_{min(n_r, CHUNK) + C + 2} P_r[i, j]
#       alpha0 G: G's chain over GRAM_ROWS rows, its NB blocks, the product by alpha0, the two final additions:
#                                                                                                  gamma_{GRAM_ROWS + NB + 3} alpha0 P_all[i, j]
#       lambda_r: the last addition                                                                  gamma_2 lambda_r on the diagonal
#     with P_r = sum_{c in S_r} |z_c| |z_c|^T and P_all = |Z|^T |Z| (entrywise absolute values).  The 2-norm of an entrywise bound bounds the
#     2-norm: eta_form = | gamma P_r + gamma alpha0 P_all + gamma_2 lambda_r I |_2 / |A|_2.  In the same way
#     eta_b = gamma_{min(n_r, CHUNK) + C} | sum_c |z_c| |_2 / |b|_2.
# (2) Solving.  Cholesky and the two substitutions (Higham Thm 10.3, 10.4): (A^ + dA2) x^ = b^ with |dA2| <= gamma_{3 d + 1} |L^| |L^|^T, and
#     (10.7) | |L^| |L^|^T |_2 <= d (1 - d gamma_{d + 1})^-1 |A^|_2, so eta_solve = d gamma_{3 d + 1} / (1 - d gamma_{d + 1}) relative to
#     |A^|_2 <= (1 + eta_form) |A|_2.
# eta = eta_form + (1 + eta_form) eta_solve + eta_b.  Everything is evaluated in float64 on the test's own inputs.
# dZ (optional, per row of Z): a bound on the 2-norm of the difference between the rows the kernel read and the rows Z given here -- the
# propagated error of the half-sweep before.  It enters as a further backward error, |dA| <= alpha0 (2 |Z|_2 |dZ|_F + |dZ|_F^2) +
# sum_c (2 |z_c| dz_c + dz_c^2) and |db| <= sum_c dz_c, and the magnitudes of part (1) are taken at |Z| + dZ.
def row_bounds(indptr, indices, Z, alpha0, lam, rows, chunk=CHUNK, dZ=None):
    Z = np.asarray(Z, dtype=np.float64)
    n, d = Z.shape
    a0 = alpha32(alpha0)
    G = Z.T @ Z
    Zabs = np.abs(Z) if dZ is None else np.abs(Z) + np.asarray(dZ, dtype=np.float64)[:, None]
    P_all = Zabs.T @ Zabs
    nb = -(-n // GRAM_ROWS)
    g_gram = gamma(GRAM_ROWS + nb + 3)
    eta_solve = d * gamma(3 * d + 1) / (1.0 - d * gamma(d + 1))
    if dZ is not None:
        dz = np.asarray(dZ, dtype=np.float64)
        dG = a0 * (2.0 * np.linalg.norm(Z, 2) * np.linalg.norm(dz) + np.linalg.norm(dz) ** 2)
    out = {k: np.zeros(len(rows)) for k in ("kappa", "eta", "bound", "xnorm", "lmax")}
    X = np.zeros((len(rows), d))
    for t, r in enumerate(rows):
        cols = indices[indptr[r]:indptr[r + 1]]
        nr = len(cols)
        C = max(1, -(-nr // chunk))
        A, b = normal_equations(indptr, indices, Z, alpha0, lam, r, G)
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
                prop = (dG + np.sum(2.0 * zn * dz[cols] + dz[cols] ** 2)) / sv[0] + dz[cols].sum() / bn
        eta = eta_form + (1.0 + eta_form) * eta_solve + eta_b + prop
        kappa = sv[0] / sv[-1]
        X[t] = np.linalg.solve(A, b)
        out["kappa"][t], out["eta"][t], out["lmax"][t], out["xnorm"][t] = kappa, eta, sv[0], np.linalg.norm(X[t])
        out["bound"][t] = kappa * eta / (1.0 - kappa * eta) if kappa * eta < 1.0 else np.inf
    out["x"] = X
    return out


# ---- the a-priori bound of the objective's sums ----------------------------------------------------------------------------------------------------
# pda_ials_loss_f32 at fp32 tables (X, Y) against objective() at the same tables.  Per user row, with u the unit roundoff:
#   a dot product of d terms, products rounded, any order:        |s^ - s| <= gamma_d |x| . |y_c|  =: e_c
#   r = s - 1 (one rounding):                                      |r^ - r| <= (1 + u) e_c + u |r|  =: D_c
#   r^2 (one rounding), the n_r terms in a chain:                  |fit^ - fit| <= (1 + gamma_{n_r + 1}) sum_c (2 |r_c| + D_c) D_c + gamma_{n_r + 1} sum_c r_c^2
#   x^T G x: G as computed (gamma_{GRAM_ROWS + NB} P_all), t = G x (gamma_{d + 1}), q = t . x (gamma_d):
#                                                                  |q^ - q| <= gamma_{GRAM_ROWS + NB + 2 d + 1} |x|^T P_all |x|
#   lam_r |x|^2: gamma_{d + 1} lam_r |x|^2
# The float64 reductions over the rows and the item side's regulariser (float64 from the fp32 table) add at most n 2^-53 relative: 1e-12 L.
def loss_bound(X, Y, up, ui, alpha0, lam_u, L):
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    d = X.shape[1]
    P_all = np.abs(Y).T @ np.abs(Y)
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
        total += alpha32(alpha0) * gamma(GRAM_ROWS + nb + 2 * d + 1) * (np.abs(x) @ P_all @ np.abs(x))
        total += gamma(d + 1) * float(lam_u[r]) * (x @ x)
    return total + 1e-12 * abs(L)


# ---- the inputs the GPU suite and the host suite share ---------------------------------------------------------------------------------------------
ROW_LENGTHS = (0, 1, 2, 31, 32, 33, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5)
N_OTHER = 2 * CHUNK + 40
PARAMS = ((0.1, 0.05, 1.0), (0.01, 1e-3, 0.0), (1.0, 1e-5, 0.0))          # (alpha0, lambda, nu)
TABLES = ("gauss0.05", "gauss0.3", "gauss1", "rank4")


def length_graph(seed=7, lengths=ROW_LENGTHS, n_other=N_OTHER):
    """The pairs of a side whose rows have exactly the given lengths, columns drawn without replacement -> (rows, cols)."""
    g = np.random.default_rng(seed)
    rows = np.concatenate([np.full(n, r, dtype=np.int64) for r, n in enumerate(lengths)])
    cols = np.concatenate([np.sort(g.choice(n_other, n, replace=False)) for n in lengths]).astype(np.int64)
    return rows, cols


def eighths_table(n, d, seed):
    """Multiples of 1/8 with |k| <= 4: every product is a multiple of 1/64 and every sum of the exact test is exact in fp32."""
    return (np.random.default_rng(seed).integers(-4, 5, (n, d)) / 8.0).astype(np.float32)


def table(kind, n, d, seed=11):
    """Gaussian tables of three scales and a correlated one: rank 4 plus unit noise, the rank-4 part scaled so that the four strong directions
    of Z^T Z carry about twice the noise floor whatever d.  That is as much correlation as the condition kappa eta < 0.1 leaves room for: eta is
    about 0.015 on the longest rows (their b = sum z cancels: | sum |z| | / | sum z | ~ sqrt(n_r)), so kappa has to stay below about 6."""
    g = np.random.default_rng(seed)
    if kind.startswith("gauss"):
        return (g.standard_normal((n, d)) * float(kind[5:])).astype(np.float32)
    B, Cm = g.standard_normal((n, 4)), g.standard_normal((4, d)) * np.sqrt(1.0 / d)
    return (0.3 * (B @ Cm + g.standard_normal((n, d)))).astype(np.float32)
