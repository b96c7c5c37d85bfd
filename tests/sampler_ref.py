"""Numpy restatement of the device triplet sampler (pda_amd/csrc/pda_sample.h, sample_one) for the sampler tests.

    mix64, draw, bounded   the counter-based RNG: splitmix64 of (seed, step, row, draw index), uint64 wrap-around
    feistel_rounds         how many Feistel rounds a pool of n users gets (FOUR_ROUNDS: the rule before the small-pool fix)
    feistel_perm           the keyed permutation of [0, n) with cycle walking, over the still-active rows only
    sample_users           the users of a batch when the sampler draws them itself
    sample                 one batch: users, pos, neg, pos_pop, neg_pop and, beyond what the kernel writes, the drawn row
                           position (-1: empty row) and the number of rejected negatives
    stream_batches         DeviceSampler's stream (steps 1, 2, ...) from a loaded dataset, on the host

Everything is vectorised over (step, row) pairs; seeds and steps may be Python ints of any size, reduced mod 2^64.
"""
import numpy as np

u64 = np.uint64
MASK = (1 << 64) - 1
REJECT_CAP = 4096            # negatives tried before the kernel keeps what it drew last (a train item, then)
SMALL_HALF_BITS = 4          # Feistel halves of at most this many bits (pools <= 256) get EXTRA_ROUNDS more rounds
EXTRA_ROUNDS = 12
FOUR_ROUNDS = lambda hb: 4   # noqa: E731  (the rule of the parent algorithm)


def mix64(z):
    """splitmix64 finaliser on a uint64 array (or a Python int -> Python int)."""
    if isinstance(z, int):
        z = (z + 0x9E3779B97F4A7C15) & MASK
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        return z ^ (z >> 31)
    z = np.asarray(z, dtype=u64)
    if z.ndim == 0:
        return u64(mix64(int(z)))
    with np.errstate(over="ignore"):
        z = z + u64(0x9E3779B97F4A7C15)         # (two temporaries for the whole chain: this is the tests' inner loop)
        t = z >> u64(30)
        t ^= z
        t *= u64(0xBF58476D1CE4E5B9)
        np.right_shift(t, u64(27), out=z)
        z ^= t
        z *= u64(0x94D049BB133111EB)
        np.right_shift(z, u64(31), out=t)
        t ^= z
    return t


def _steps(step):
    """Python int(s) of any size -> uint64 array, reduced mod 2^64."""
    if isinstance(step, np.ndarray) and step.dtype == u64:
        return step
    return np.array([int(s) & MASK for s in np.atleast_1d(np.asarray(step, dtype=object)).ravel()], dtype=u64).reshape(np.shape(step))


def draw(seed, step, rows, k):
    """uint64 array holding the 32-bit draw number k (scalar or array) of each (step, row)."""
    with np.errstate(over="ignore"):
        h = mix64(u64(seed & MASK) ^ (np.atleast_1d(_steps(step)) * u64(0xD1B54A32D192ED03)))
    word = (np.asarray(rows, dtype=u64) << u64(32)) | np.asarray(k, dtype=u64)
    return mix64(h ^ word) >> u64(32)


def bounded(r, n):
    """(r * n) >> 32 for 32-bit r and n (array or scalar)."""
    return (np.asarray(r, dtype=u64) * np.asarray(n, dtype=u64)) >> u64(32)


def half_bits(n):
    bits = 1
    while (1 << bits) < n:
        bits += 1
    return (bits + 1) // 2


def feistel_rounds(hb):
    return 4 + (EXTRA_ROUNDS if hb <= SMALL_HALF_BITS else 0)


def feistel_perm(x, n, key, rounds=feistel_rounds):
    """x (array of positions < n) -> their images under the keyed permutation of [0, n); key: one uint64, or one per position."""
    hb = half_bits(n)
    hm = u64((1 << hb) - 1)
    n_rounds = rounds(hb)
    x = np.array(x, dtype=u64).ravel()
    key = np.broadcast_to(np.asarray(key, dtype=u64), x.shape)
    act = np.arange(x.size)
    while act.size:
        l, r, ka = x[act] >> u64(hb), x[act] & hm, key[act]
        for rnd in range(n_rounds):
            f = mix64(ka ^ u64(rnd << 40) ^ r) & hm
            l, r = r, l ^ f
        x[act] = (l << u64(hb)) | r
        act = act[x[act] >= u64(n)]
    return x.astype(np.int64)


def _in_row(indices, b, e, n):
    """Lower-bound search of n[i] in indices[b[i]:e[i]] (ascending rows), like the kernel's: is it there?"""
    lo, hi = b.copy(), e.copy()
    while True:
        open_ = lo < hi
        if not open_.any():
            break
        mid = (lo + hi) >> 1
        less = np.zeros(len(n), dtype=bool)
        less[open_] = indices[mid[open_]] < n[open_]
        lo = np.where(open_ & less, mid + 1, lo)
        hi = np.where(open_ & ~less, mid, hi)
    hit = lo < e
    hit[hit] = indices[lo[hit]] == n[hit]
    return hit


def sample_users(seed, step, rows, B, n_pool, user_pool=None, rounds=feistel_rounds):
    """The users the sampler itself draws (gen_users != 0) for the (step, row) pairs: distinct inside a step while
    B <= n_pool (the keyed permutation), with replacement above."""
    r = np.asarray(rows, dtype=np.int64)
    step = np.broadcast_to(np.atleast_1d(_steps(step)), r.shape)
    if B <= n_pool:
        x = feistel_perm(r, n_pool, mix64(u64(seed & MASK) ^ mix64(step)), rounds).reshape(r.shape)
    else:
        x = bounded(draw(seed, step, r, 7), n_pool).astype(np.int64)
    return x if user_pool is None else np.asarray(user_pool)[x].astype(np.int64)


def sample(seed, step, B, indptr, indices, *, slots=None, user_pool=None, n_pool=0, users=None, neg_range, pop_matrix=None,
           rounds=feistel_rounds, rows=None):
    """sample_one for rows of a batch of B: all of them at one step, or the (step, row) pairs given as two arrays of equal
    length (many steps in one call).  users given: gen_users = 0 (indexed by row).
    -> dict(users, pos, neg, pos_pop, neg_pop, idx, rejections); the pops are None without a pop_matrix."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int32)
    r = np.arange(B, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    seed, step = seed & MASK, np.broadcast_to(np.atleast_1d(_steps(step)), r.shape)
    if users is None:
        u = sample_users(seed, step, r, B, n_pool, user_pool, rounds)
    else:
        u = np.asarray(users, dtype=np.int64)[r]
    b, e = indptr[u], indptr[u + 1]
    ln = e - b
    n_slots = 0 if pop_matrix is None else pop_matrix.shape[1]
    empty = ln == 0
    idx = np.where(empty, -1, bounded(draw(seed, step, r, 0), np.maximum(ln, 0)).astype(np.int64))
    at = np.where(empty, 0, b + idx)
    has = indices.size > 0
    pos = np.where(empty, 0, indices[at] if has else 0).astype(np.int32)
    slot = np.zeros(len(r), dtype=np.int64)
    if n_slots > 0:
        slot[empty] = bounded(draw(seed, step[empty], r[empty], 1), n_slots).astype(np.int64)
    if slots is not None and has:
        slot[~empty] = np.asarray(slots)[at[~empty]]
    lo, hi = int(neg_range[0]), int(neg_range[1])
    neg = np.full(len(r), lo, dtype=np.int64)
    rej = np.zeros(len(r), dtype=np.int64)
    act = np.arange(len(r))
    for k in range(REJECT_CAP):
        neg[act] = lo + bounded(draw(seed, step[act], r[act], 16 + k), hi - lo).astype(np.int64)
        act = act[_in_row(indices, b[act], e[act], neg[act])]
        if not act.size:
            break
        rej[act] += 1
    out = dict(users=u.astype(np.int32), pos=pos, neg=neg.astype(np.int32), pos_pop=None, neg_pop=None, idx=idx, rejections=rej)
    if pop_matrix is not None:
        out["pos_pop"] = pop_matrix[pos.astype(np.int64), slot]
        out["neg_pop"] = pop_matrix[neg, slot]
    return out


def stream_batches(data, n, *, seed=2020, with_pop=False, rounds=feistel_rounds):
    """The first n batches of sampler.DeviceSampler(data, ...) (steps 1 .. n), each as sample()'s dict."""
    indptr, indices, slots = (t.numpy() for t in data.train_csr("cpu"))
    pool = np.fromiter(data.train_user_list.keys(), dtype=np.int32)
    pop = np.ascontiguousarray(data.expo_popularity, dtype=np.float32) if with_pop else None
    return [sample(seed, s, data.batch_size, indptr, indices, slots=slots if with_pop else None, user_pool=pool, n_pool=len(pool),
                   neg_range=(0, data.n_items), pop_matrix=pop, rounds=rounds) for s in range(1, n + 1)]
