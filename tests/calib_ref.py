"""numpy restatement of include/pda_hip_calib.h ("5w. Calibrated popularity"): the profile, the list counts and the selection.
The divergences are float64, one operation at a time and each group's terms added in ascending g; the relevance and x are separate fp32
operations; and at every step the selection is the naive arg-max over ALL unpicked candidates -- not the G-way merge of group sub-lists the
kernel runs, which `merge_row` restates on its own so that the shortcut is tested and not assumed.

The device's log / log2 and numpy's need not agree in the last bit, so a row is flagged FRAGILE when some divergence it evaluated lies within
2^-40 of a boundary of the 2^-20 grid (|D 2^20 - (floor(D 2^20) + 0.5)| < 2^-20): there the grid point may legitimately differ."""
import numpy as np

f32 = np.float32
GRID = 1048576.0            # 2^20
DQ_MAX = 8388608.0          # 2^23
MARGIN = 2.0 ** -20         # of D 2^20 around a half-integer: D within 2^-40 of a boundary


def group_bytes(idx, item_group, G):
    """-> int64, the shape of idx: the group of each entry, G for an id outside the catalogue or an item whose byte is >= G."""
    idx = np.asarray(idx, np.int64)
    item_group = np.asarray(item_group, np.uint8)
    inside = (idx >= 0) & (idx < len(item_group))
    gb = item_group[np.clip(idx, 0, len(item_group) - 1)].astype(np.int64)
    return np.where(inside & (gb < G), gb, G)


def valid_prefix(cand_idx, cand_val, item_group, G):
    """-> n_valid int64 [R]: the position of the first candidate whose id is outside the catalogue, whose value is not finite or whose item
    has no group (N if none)."""
    bad = (group_bytes(cand_idx, item_group, G) >= G) | ~np.isfinite(cand_val)
    return np.where(bad.any(axis=1), bad.argmax(axis=1), cand_idx.shape[1]).astype(np.int64)


def profile_ref(hist_rows, item_group, G):
    """-> int32 [R, G]: each row's distinct in-catalogue history entries per group.  hist_rows None: zeros cannot be sized -- pass rows."""
    out = np.zeros((len(hist_rows), G), np.int32)
    for r, h in enumerate(hist_rows):
        gb = group_bytes(np.unique(np.asarray(h, np.int64)), item_group, G)
        out[r] = np.bincount(gb, minlength=G + 1)[:G]
    return out


def list_counts_ref(idx, item_group, G, Ks):
    """-> int32 [R, nK, G]: the entries of each group among the first Ks[j] columns."""
    gb = group_bytes(idx, item_group, G)
    out = np.zeros((gb.shape[0], len(Ks), G), np.int32)
    for j, k in enumerate(Ks):
        for g in range(G):
            out[:, j, g] = (gb[:, :k] == g).sum(axis=1)
    return out


def relevance(cand_val, n_valid):
    """-> p f32 [R, N]: min-max normalised over the valid prefix (0 behind it, and everywhere when the range is 0 or not finite)."""
    R, N = cand_val.shape
    p = np.zeros((R, N), f32)
    with np.errstate(all="ignore"):
        for r in range(R):
            nv = int(n_valid[r])
            if nv == 0:
                continue
            v = cand_val[r, :nv].astype(f32)
            lo = v[nv - 1]
            rng = f32(v[0] - lo)
            if rng != 0 and np.isfinite(rng):
                p[r, :nv] = (v - lo).astype(f32) / rng
    return p


def divergences(prof, n, t, div="js", alpha=0.01, dtype=np.float64):
    """-> D [R, G] in `dtype`: D[r, c] = the divergence between row r's profile and the list of t + 1 items that its picks n[r] (per group, t
    in all) become with one more item of group c.  prof, n: integer counts [R, G].  H = 0: zeros.  One operation at a time, every group's
    terms added in ascending g; (1 - alpha) is one float64 whatever the dtype."""
    prof, n = np.asarray(prof, np.int64), np.asarray(n, np.int64)
    R, G = prof.shape
    H = prof.sum(axis=1)
    some = H > 0
    half, zero = dtype(0.5), dtype(0.0)
    with np.errstate(all="ignore"):
        pi = np.where(some[:, None], prof.astype(dtype) / np.where(some, H, 1).astype(dtype)[:, None], zero)      # [R, G]
        a, oma = dtype(alpha), dtype(1.0 - float(alpha))
        s = np.zeros((R, G), dtype)                                                                               # [R, c]
        eye = np.eye(G, dtype=np.int64)
        for g in range(G):
            q = (n[:, g:g + 1] + eye[g][None, :]).astype(dtype) / dtype(t + 1)                                    # [R, c]
            pg = pi[:, g:g + 1]
            if div == "js":
                m = half * (pg + q)
                ta = np.where(pg > 0, pg * np.log2(np.where(pg > 0, pg / m, 1)), zero)
                tb = np.where(q > 0, q * np.log2(np.where(q > 0, q / m, 1)), zero)
                s = s + (ta + tb)
            else:
                qs = oma * q + a * pg
                s = s + np.where(pg > 0, pg * np.log(np.where(pg > 0, pg / qs, 1)), zero)
        D = half * s if div == "js" else s
    return np.where(some[:, None], D, zero).astype(dtype)


def quantise(D):
    """-> (D32 f32, fragile bool), the shape of D: the divergences on the 2^-20 grid, and whether D lies within 2^-40 of a grid boundary."""
    y = np.asarray(D, np.float64) * GRID
    dq = np.clip(np.rint(y), 0.0, DQ_MAX)
    fragile = (np.abs(y - (np.floor(y) + 0.5)) < MARGIN) & (y > -1.0) & (y < DQ_MAX + 1.0)      # (outside: clamped whatever the last bit)
    return (dq.astype(np.int64).astype(f32) * f32(2.0 ** -20)).astype(f32), fragile


def calib_ref(cand_idx, cand_val, prof, item_group, G, lam, K, div="js", alpha=0.01):
    """-> (idx int32 [R, K], val f32 [R, K], dv f32 [R, K], fragile bool [R])."""
    cand_idx = np.asarray(cand_idx, np.int32)
    cand_val = np.asarray(cand_val, f32)
    prof = np.asarray(prof, np.int64)
    R, N = cand_idx.shape
    n_valid = valid_prefix(cand_idx, cand_val, item_group, G)
    L, W = f32(lam), f32(1.0 - float(lam))
    wp = (W * relevance(cand_val, n_valid)).astype(f32)
    avail = np.arange(N)[None, :] < n_valid[:, None]
    cat = np.minimum(group_bytes(cand_idx, item_group, G), G - 1)          # (behind the prefix: never picked)
    n = np.zeros((R, G), np.int64)
    out_idx = np.full((R, K), -1, np.int32)
    out_val = np.full((R, K), -np.inf, f32)
    out_div = np.full((R, K), -np.inf, f32)
    fragile = np.zeros(R, bool)
    rows = np.arange(R)
    for t in range(K):
        d32, fr = quantise(divergences(prof, n, t, div, alpha))            # [R, G]
        pen = (L * d32).astype(f32)
        x = (wp - np.take_along_axis(pen, cat, axis=1)).astype(f32)        # every candidate, then the unpicked ones
        j = np.where(avail, x, -np.inf).argmax(axis=1)                     # ties: the smallest position
        live = avail[rows, j]
        fragile |= live & fr.any(axis=1)                                   # (a row behind its last pick evaluates nothing)
        rl, jl = rows[live], j[live]
        out_idx[rl, t] = cand_idx[rl, jl]
        out_val[rl, t] = x[rl, jl]
        out_div[rl, t] = d32[rl, cat[rl, jl]]
        n[rl, cat[rl, jl]] += 1
        avail[rl, jl] = False
    return out_idx, out_val, out_div, fragile


def merge_row(cand_idx, cand_val, prof_row, item_group, G, lam, K, div="js", alpha=0.01):
    """One row by the merge of its G group sub-lists: the selection the kernel runs -> (idx [K], val [K], dv [K])."""
    cand_idx = np.asarray(cand_idx, np.int32)[None, :]
    cand_val = np.asarray(cand_val, f32)[None, :]
    nv = int(valid_prefix(cand_idx, cand_val, item_group, G)[0])
    L, W = f32(lam), f32(1.0 - float(lam))
    p = relevance(cand_val, np.array([nv]))[0]
    gb = group_bytes(cand_idx[0], item_group, G)
    lists = [[] for _ in range(G)]
    for v in range(nv):
        if len(lists[gb[v]]) < K:                                           # only the first K members of a group can be picked
            lists[gb[v]].append((f32(W * p[v]), v))
    n = np.zeros(G, np.int64)
    out_idx, out_val, out_div = np.full(K, -1, np.int32), np.full(K, -np.inf, f32), np.full(K, -np.inf, f32)
    for t in range(min(K, nv)):
        d32 = quantise(divergences(np.asarray(prof_row)[None, :], n[None, :], t, div, alpha))[0][0]
        best = None
        for c in range(G):
            if n[c] < len(lists[c]):
                wpc, pos = lists[c][n[c]]
                x = f32(wpc - f32(L * d32[c]))
                if best is None or x > best[0] or (x == best[0] and pos < best[1]):
                    best = (x, pos, c)
        x, pos, c = best
        out_idx[t], out_val[t], out_div[t] = cand_idx[0, pos], x, d32[c]
        n[c] += 1
    return out_idx, out_val, out_div
