"""The shared cases of tests/test_calib_host.py and tests/test_gpu_calib.py: one generator, fixed seeds, and the float64 reference of every case
computed once per process.  67 rows (the last workgroup is partial), candidates as in tests/test_gpu_xquad.py (distinct ids, values descending,
every other case rounded to halves: many ties), histories of 0 .. 40 entries with duplicates drawn from a long-tailed count vector, groups cut
from that count vector.  Every (N, K) shape runs every G with both divergences; lambda cycles through its five values over them."""
import functools

import numpy as np

from calib_ref import calib_ref, profile_ref

f32 = np.float32
N_ITEMS = 5000
ROWS, N_USERS = 67, 150
LAMBDAS = (0.0, 0.1, 0.5, 0.9, 1.0)
GROUPS = (2, 3, 8)
DIVS = ("js", "kl")
ALPHA = 0.01
MAX_FRAGILE = 2                       # rows of a case that may be left out as fragile
SHAPES = [(N, K) for N in (1, 50, 63, 64, 65, 100, 1000, 1024) for K in (1, 20, 50, 64) if K <= N]
CASES = [(N, K, G, div, LAMBDAS[(i + j) % 5]) for i, (N, K) in enumerate(SHAPES) for j, (G, div) in enumerate((G, d) for G in GROUPS for d in DIVS)]
CASE_IDS = ["N%d-K%d-G%d-%s-lam%g" % c for c in CASES]


def long_tail_counts(rng, n_items=N_ITEMS):
    """int64 [n_items]: train counts with a long tail (a Zipf-like law over a random order of the items, a few items without any entry)."""
    c = np.floor(4000.0 / (1.0 + np.arange(n_items)) ** 0.9).astype(np.int64)
    return c[rng.permutation(n_items)]


def groups_of(counts, G):
    """uint8 [n_items]: G groups of roughly equal train interactions, the most popular items first (pda_amd.calib.cut_groups)."""
    from pda_amd.calib import cut_groups
    return cut_groups(counts, [(i + 1) / G for i in range(G - 1)])


def candidates(rng, R, N, n_items=N_ITEMS, ties=True):
    """Distinct ids per row, values descending (rounded to halves: many ties)."""
    idx = np.argsort(rng.random((R, n_items)), axis=1)[:, :N].astype(np.int32)
    val = -np.sort(-rng.standard_normal((R, N)).astype(f32) * f32(2), axis=1)
    if ties:
        val = (np.round(val * 2) / 2).astype(f32)
    return idx, val


def histories(rng, n_rows, counts):
    """Rows of 0 .. 40 entries drawn in proportion to the counts, some of them twice or three times."""
    p = counts / counts.sum()
    out = []
    for r in range(n_rows):
        h = rng.choice(len(counts), size=rng.integers(0, 41), p=p)
        if r % 3 == 0 and len(h):
            h = np.concatenate([h, h[:3], h[:1]])
        out.append(h)
    return out


@functools.lru_cache(maxsize=None)
def case(N, K, G, div, lam):
    """-> dict: the inputs of a case and its reference (`want` = idx, val, dv; `fragile` bool [ROWS]).  Read-only: shared between tests."""
    rng = np.random.default_rng(100000 * N + 1000 * K + 100 * G + 10 * DIVS.index(div) + LAMBDAS.index(lam))
    counts = long_tail_counts(rng)
    item_group = groups_of(counts, G)
    idx, val = candidates(rng, ROWS, N, ties=(SHAPES.index((N, K)) + GROUPS.index(G) + DIVS.index(div)) % 2 == 0)
    users = rng.permutation(N_USERS)[:ROWS].astype(np.int32)
    hist = histories(rng, N_USERS, counts)
    rows = [hist[u] for u in users]
    prof = profile_ref(rows, item_group, G)
    wi, wv, wd, fragile = calib_ref(idx, val, prof, item_group, G, lam, K, div, ALPHA)
    out = dict(N=N, K=K, G=G, div=div, lam=lam, item_group=item_group, idx=idx, val=val, users=users, hist=hist, rows=rows, prof=prof,
               want=(wi, wv, wd), fragile=fragile)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
