"""numpy restatement of the xQuAD contract of include/pda_hip_xquad.h ("5e. xQuAD"): every operation a separate fp32 operation,
and at every step the naive arg-max over ALL unpicked candidates -- not the merge of two category sub-lists the kernel runs, which
`merge_row` restates on its own so that the shortcut is tested and not assumed."""
import numpy as np

f32 = np.float32


def valid_prefix(cand_idx, cand_val, n_items):
    """-> n_valid int64 [R]: the position of the first candidate whose id is outside [0, n_items) or whose value is not finite (N if none)."""
    ok = (cand_idx >= 0) & (cand_idx < n_items) & np.isfinite(cand_val)
    bad = ~ok
    return np.where(bad.any(axis=1), bad.argmax(axis=1), cand_idx.shape[1]).astype(np.int64)


def profile(hist_rows, is_head):
    """-> q f32 [R, 2]: q[:, 0] the long-tail share, q[:, 1] the head share of each row's distinct in-catalogue history entries (0, 0 for none)."""
    n_items = len(is_head)
    q = np.zeros((len(hist_rows), 2), f32)
    for r, h in enumerate(hist_rows):
        h = np.unique(np.asarray(h, np.int64))
        h = h[(h >= 0) & (h < n_items)]
        H = len(h)
        if H:
            H1 = int((is_head[h] != 0).sum())
            q[r, 1] = f32(H1) / f32(H)
            q[r, 0] = f32(H - H1) / f32(H)
    return q


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


def coverage(n, t, variant):
    """cov f32 of the categories whose pick counts are n (any shape) after t picks."""
    n = np.asarray(n)
    if variant == "binary":
        return (n == 0).astype(f32)
    if t == 0:
        return np.ones(n.shape, f32)
    return (f32(1) - (n.astype(f32) / f32(t)).astype(f32)).astype(f32)


def xquad_ref(cand_idx, cand_val, is_head, hist_rows, lam, K, variant="smooth"):
    """-> (idx int32 [R, K], val f32 [R, K]).  hist_rows: one list of item ids per row (any order, duplicates allowed), or None."""
    cand_idx = np.asarray(cand_idx, np.int32)
    cand_val = np.asarray(cand_val, f32)
    is_head = np.asarray(is_head, np.uint8)
    R, N = cand_idx.shape
    n_items = len(is_head)
    n_valid = valid_prefix(cand_idx, cand_val, n_items)
    q = profile(hist_rows, is_head) if hist_rows is not None else np.zeros((R, 2), f32)
    L, W = f32(lam), f32(1.0 - float(lam))
    avail = np.arange(N)[None, :] < n_valid[:, None]
    cat = np.where(avail, is_head[np.clip(cand_idx, 0, n_items - 1)] != 0, False).astype(np.int64)
    wp = (W * relevance(cand_val, n_valid)).astype(f32)
    n = np.zeros((R, 2), np.int64)
    out_idx = np.full((R, K), -1, np.int32)
    out_val = np.full((R, K), -np.inf, f32)
    rows = np.arange(R)
    for t in range(K):
        bonus = (L * (q * coverage(n, t, variant)).astype(f32)).astype(f32)          # [R, 2]
        x = (wp + np.take_along_axis(bonus, cat, axis=1)).astype(f32)                  # every candidate, then the unpicked ones
        xm = np.where(avail, x, -np.inf)
        j = xm.argmax(axis=1)                                                          # ties: the smallest position
        live = avail[rows, j]
        out_idx[live, t] = cand_idx[rows[live], j[live]]
        out_val[live, t] = x[rows[live], j[live]]
        n[rows[live], cat[rows[live], j[live]]] += 1
        avail[rows[live], j[live]] = False
    return out_idx, out_val


def merge_row(cand_idx, cand_val, is_head, hist_row, lam, K, variant="smooth"):
    """One row by the merge of its two category sub-lists (fp32 scalars): the selection the kernel runs."""
    cand_idx = np.asarray(cand_idx, np.int32)[None, :]
    cand_val = np.asarray(cand_val, f32)[None, :]
    is_head = np.asarray(is_head, np.uint8)
    nv = int(valid_prefix(cand_idx, cand_val, len(is_head))[0])
    q = profile([hist_row], is_head)[0] if hist_row is not None else np.zeros(2, f32)
    L, W = f32(lam), f32(1.0 - float(lam))
    p = relevance(cand_val, np.array([nv]))[0]
    lists = [[], []]
    for v in range(nv):
        c = int(is_head[cand_idx[0, v]] != 0)
        if len(lists[c]) < K:                                                          # only the first K members of a category can be picked
            lists[c].append((f32(W * p[v]), v))
    n = [0, 0]
    out_idx = np.full(K, -1, np.int32)
    out_val = np.full(K, -np.inf, f32)
    for t in range(min(K, nv)):
        cov = coverage(np.array(n), t, variant)
        x = [None, None]
        for c in (0, 1):
            if n[c] < len(lists[c]):
                x[c] = f32(lists[c][n[c]][0] + f32(L * f32(q[c] * cov[c])))
        if x[0] is None:
            c = 1
        elif x[1] is None:
            c = 0
        elif x[1] > x[0] or (x[1] == x[0] and lists[1][n[1]][1] < lists[0][n[0]][1]):
            c = 1
        else:
            c = 0
        out_idx[t] = cand_idx[0, lists[c][n[c]][1]]
        out_val[t] = x[c]
        n[c] += 1
    return out_idx, out_val


def prefix_end_search(valid, base):
    """The kernel's search for the end of the valid prefix behind position `base` (a multiple of 64 below N, every position before it valid):
    one probe of 64 evenly spaced positions, one of the at most 14 positions between two of them.  valid: bool [N], no True behind a False."""
    N = len(valid)
    s = (N - base + 63) >> 6
    j = 0
    while j < 64 and base + j * s < N and valid[base + j * s]:
        j += 1
    if j == 0:
        return base
    at = base + (j - 1) * s
    k = 0
    while k < s - 1 and at + 1 + k < N and valid[at + 1 + k]:
        k += 1
    return at + 1 + k
