"""The device sampler against its numpy restatement (tests/sampler_ref.py), bit for bit on every output, at the pools, batch sizes,
rows, ranges, steps and seeds where an index or a width can go wrong.  tests/test_sampler_distribution.py tests the restatement's
distribution against the reference protocol; together they hold the kernel to it.  Every case is one launch."""
import numpy as np
import pytest
import torch

import sampler_ref as sr

pytestmark = pytest.mark.gpu

TOP = 0x9E3779B97F4A7C15          # a seed with the top bit set
KEYS = ("users", "pos", "neg", "pos_pop", "neg_pop")


def to(dev, *arrs):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


def csr_of(rows):
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    flat = np.concatenate([np.asarray(r, np.int32) for r in rows]) if indptr[-1] else np.zeros(0, np.int32)
    return indptr, flat.astype(np.int32)


def random_rows(rng, n_users, n_items, max_len, empty_every=0):
    rows = [np.sort(rng.permutation(n_items)[:rng.integers(1, max_len + 1)]).astype(np.int32) for _ in range(n_users)]
    if empty_every:
        for u in range(0, n_users, empty_every):
            rows[u] = np.zeros(0, np.int32)
    return rows


def same(got, ref, what=""):
    """Every output equal, floats by their bits, no row left out."""
    for k, g in zip(KEYS, got):
        r = ref[k]
        assert (g is None) == (r is None), (what, k)
        if g is None:
            continue
        g = g.cpu().numpy()
        assert g.shape == r.shape and g.dtype == r.dtype, (what, k, g.shape, r.shape, g.dtype, r.dtype)
        bad = np.flatnonzero(g.view(np.int32) != r.view(np.int32))
        assert bad.size == 0, "%s: %s differs in %d of %d rows, first at row %d: kernel %r, restatement %r" % (
            what, k, bad.size, g.size, bad[0], g[bad[0]], r[bad[0]])


def check(dev, indptr, indices, B, *, seed, step, neg_range, slots=None, pop=None, pool=None, n_pool=0, users=None, what=""):
    from pda_amd import ops
    n_rows = len(indptr) - 1
    ids = users if users is not None else pool if pool is not None else np.arange(n_pool)
    assert 0 <= np.min(ids) and np.max(ids) < n_rows and (pool is None or len(pool) >= n_pool)       # nothing is read out of bounds
    assert 0 <= neg_range[0] < neg_range[1] and (pop is None or (neg_range[1] <= pop.shape[0] and indices.max(initial=0) < pop.shape[0]))
    assert slots is None or pop is None or slots.max(initial=0) < pop.shape[1]
    ip, ix, sl, pm, pl, us = to(dev, indptr, indices, slots, pop, pool, users)
    got = ops.sample_triplets(ip, ix, B, seed=seed, step=step, users=us, user_pool=pl, n_pool=n_pool, train_slots=sl,
                              neg_range=neg_range, pop_matrix=pm)
    torch.cuda.synchronize()
    ref = sr.sample(seed, step, B, indptr, indices, slots=slots, user_pool=pool, n_pool=n_pool, users=users, neg_range=neg_range,
                    pop_matrix=pop)
    same(got, ref, what)
    return ref


@pytest.fixture(scope="module")
def world():
    """70 000 users (every pool below fits), 300 items, rows of 1 .. 40 items, every 11th row empty, slots and a pop matrix."""
    rng = np.random.default_rng(2020)
    n_users, n_items, T = 70000, 300, 7
    lens = rng.integers(1, 41, n_users)
    lens[::11] = 0
    gaps = rng.integers(1, 8, (n_users, 40))
    items = np.cumsum(gaps, axis=1) - 1 + rng.integers(0, 20, n_users)[:, None]          # ascending, distinct, below 300
    assert items.max() < n_items
    indptr = np.zeros(n_users + 1, np.int64)
    indptr[1:] = np.cumsum(lens)
    indices = items[np.arange(40)[None, :] < lens[:, None]].astype(np.int32)
    slots = rng.integers(0, T, len(indices)).astype(np.int32)
    pop = rng.uniform(0, 1, (n_items, T)).astype(np.float32)
    return dict(indptr=indptr, indices=indices, slots=slots, pop=pop, n_users=n_users, n_items=n_items)


POOLS = [1, 2, 3, 4, 5, 8, 9, 31, 32, 33, 64, 65, 1000, 1024, 1025, 65537]


@pytest.mark.parametrize("n_pool", POOLS)
def test_pools_and_batches_around_them(dev, world, n_pool):
    """B = n_pool, B < n_pool (distinct users: the keyed permutation with its cycle walk) and B > n_pool (with replacement), with a
    user_pool and without.  Pools of at most 256 users take the sixteen-round permutation, the others the four-round one."""
    w = world
    perm = np.random.default_rng(n_pool).permutation(w["n_users"])[:n_pool].astype(np.int32)
    sizes = {n_pool, max(1, n_pool // 2), max(1, n_pool - 1), n_pool + 1, 2 * n_pool + 3}
    for j, B in enumerate(sorted(sizes)):
        for pool in (None, perm):
            ref = check(dev, w["indptr"], w["indices"], B, seed=2020 + j, step=j + 1, neg_range=(0, w["n_items"]), slots=w["slots"], pop=w["pop"],
                        pool=pool, n_pool=n_pool, what="pool %d, B %d, user_pool %s" % (n_pool, B, pool is not None))
            distinct = len(set(ref["users"].tolist())) == B
            assert distinct if B <= n_pool else not distinct           # (B > n_pool cannot be distinct)


@pytest.mark.parametrize("B", [1, 37, 2048, 4096])
def test_batch_sizes(dev, world, B):
    w = world
    for pop in (None, w["pop"]):
        check(dev, w["indptr"], w["indices"], B, seed=B, step=3, neg_range=(0, w["n_items"]), slots=w["slots"], pop=pop, n_pool=5000,
              what="B %d, pop %s" % (B, pop is not None))


def test_given_users_with_repeated_ids(dev, world):
    w = world
    users = np.random.default_rng(1).integers(0, 50, 300).astype(np.int32)       # every id several times, empty rows among them
    ref = check(dev, w["indptr"], w["indices"], 300, seed=5, step=9, neg_range=(0, w["n_items"]), slots=w["slots"], pop=w["pop"], users=users,
                what="given users")
    assert np.array_equal(ref["users"], users)
    lens = np.diff(w["indptr"])[:50]
    u = max((int(c), v) for v, c in enumerate(np.bincount(users, minlength=50)) if lens[v] >= 8)[1]
    assert len(set(ref["idx"][users == u].tolist())) > 1                          # the draw belongs to the batch row, not to the user


def test_empty_rows_with_and_without_slots(dev):
    """An empty row gives pos 0 and, with a pop matrix, a time slot drawn from [0, n_slots); without one nothing else is read."""
    rows = [np.zeros(0, np.int32)] * 5 + [np.array([2, 5], np.int32)] + [np.zeros(0, np.int32)] * 4
    indptr, indices = csr_of(rows)
    pop = np.random.default_rng(0).uniform(0, 1, (12, 6)).astype(np.float32)
    slots = np.array([1, 4], np.int32)
    for p, s in ((None, None), (pop, slots), (pop, None)):
        ref = check(dev, indptr, indices, 10, seed=TOP, step=2, neg_range=(0, 12), slots=s, pop=p, n_pool=10, what="empty rows")
        assert np.all(ref["pos"][ref["idx"] < 0] == 0) and (ref["idx"] < 0).sum() == 9


def test_the_same_item_twice_under_different_slots(dev):
    rows = [np.array([3, 3, 7, 7, 7, 9], np.int32), np.array([0, 0], np.int32), np.array([4], np.int32)]
    indptr, indices = csr_of(rows)
    slots = np.array([0, 4, 1, 2, 3, 0, 2, 5, 1], np.int32)
    pop = np.arange(12 * 6, dtype=np.float32).reshape(12, 6)                       # pop identifies (item, slot)
    users = np.tile(np.arange(3, dtype=np.int32), 40)
    ref = check(dev, indptr, indices, 120, seed=77, step=1, neg_range=(0, 12), slots=slots, pop=pop, users=users, what="repeated items")
    slot_drawn = ref["pos_pop"].astype(np.int64) % 6
    assert {0, 4} <= set(slot_drawn[ref["pos"] == 3].tolist())                     # both entries of item 3 come up, each with its slot
    assert np.array_equal(ref["neg_pop"], pop[ref["neg"], slot_drawn])


def test_a_row_that_leaves_one_negative(dev):
    n_items = 64
    rows = [np.delete(np.arange(n_items, dtype=np.int32), 41), np.delete(np.arange(n_items, dtype=np.int32), 0),
            np.delete(np.arange(n_items, dtype=np.int32), n_items - 1)]
    indptr, indices = csr_of(rows)
    users = np.tile(np.arange(3, dtype=np.int32), 20)
    ref = check(dev, indptr, indices, 60, seed=3, step=1 << 32, neg_range=(0, n_items), users=users, what="one negative left")
    assert np.array_equal(ref["neg"], np.array([41, 0, n_items - 1], np.int32)[users])
    assert 0 < ref["rejections"].max() < sr.REJECT_CAP


def test_negative_range_of_one_item(dev, world):
    w = world
    ref = check(dev, w["indptr"], w["indices"], 64, seed=8, step=4, neg_range=(299, 300), slots=w["slots"], pop=w["pop"], n_pool=64,
                what="span 1")
    assert np.all(ref["neg"] == 299) and ref["rejections"].max() == 0              # (no row of the world reaches item 299)


def test_shard_range_inside_a_heavy_row_but_two_items(dev):
    """Item-parallel training: negatives from the rank's shard [lo, hi); a heavy user owns all of it but two items."""
    lo, hi, n_items = 1000, 1512, 4000
    heavy = np.setdiff1d(np.arange(900, 1700, dtype=np.int32), np.array([lo, hi - 1], np.int32))
    light = np.array([5, 1100, 3999], np.int32)
    indptr, indices = csr_of([heavy, light, np.zeros(0, np.int32)])
    users = np.array([0, 1, 2, 0, 0, 1, 0, 2] * 8, np.int32)
    ref = check(dev, indptr, indices, 64, seed=TOP + 1, step=(1 << 40) + 3, neg_range=(lo, hi), users=users, what="shard range")
    assert set(ref["neg"][users == 0].tolist()) == {lo, hi - 1}
    assert ref["neg"].min() >= lo and ref["neg"].max() < hi and 1100 not in ref["neg"][users == 1]


@pytest.mark.parametrize("seed,step", [(2020, 1 << 32), (2020, (1 << 32) + 1), (TOP, (1 << 47) + 12345), ((1 << 64) - 1, (1 << 63) + 9),
                                       (1 << 63, (1 << 64) - 1), (0, 0)])
def test_large_steps_and_seeds(dev, world, seed, step):
    w = world
    check(dev, w["indptr"], w["indices"], 512, seed=seed, step=step, neg_range=(0, w["n_items"]), slots=w["slots"], pop=w["pop"], n_pool=3000,
          what="seed %#x step %#x" % (seed, step))
    check(dev, w["indptr"], w["indices"], 40, seed=seed, step=step, neg_range=(0, w["n_items"]), n_pool=33, what="seed %#x step %#x, pool 33" % (seed, step))


def test_two_million_entries(dev):
    """Row offsets far beyond any row length: the late rows start past entry 2 000 000."""
    rng = np.random.default_rng(6)
    n_users, L, n_items = 21000, 100, 4200
    items = (np.cumsum(rng.integers(1, 40, (n_users, L)), axis=1) + rng.integers(0, 200, n_users)[:, None]).astype(np.int32)
    assert items.max() < n_items
    indptr = np.arange(n_users + 1, dtype=np.int64) * L
    indices = items.ravel()
    assert indptr[-1] > 2000000
    pool = np.arange(n_users - 4096, n_users, dtype=np.int32)                      # the users whose rows lie last
    ref = check(dev, indptr, indices, 4096, seed=12, step=7, neg_range=(0, n_items), pool=pool, n_pool=4096, what="2.1 M entries")
    assert indptr[ref["users"].astype(np.int64)].min() >= 1600000


def test_a_row_that_covers_the_whole_negative_range(dev):
    """The reference would loop for ever; the kernel gives up after 4096 rejected draws and returns the last one, a train item of
    that user (include/pda_hip.h).  The call returns, the negative lies in the range and equals the restatement's."""
    lo, hi = 10, 42
    rows = [np.arange(0, 50, dtype=np.int32), np.array([1, 2], np.int32), np.arange(lo, hi, dtype=np.int32)]
    indptr, indices = csr_of(rows)
    users = np.array([0, 1, 2, 1, 0], np.int32)
    ref = check(dev, indptr, indices, 5, seed=99, step=1, neg_range=(lo, hi), users=users, what="no negative exists")
    assert np.array_equal(ref["rejections"], np.array([sr.REJECT_CAP, 0, sr.REJECT_CAP, 0, sr.REJECT_CAP]))
    assert ref["neg"].min() >= lo and ref["neg"].max() < hi


# ---- the other entry points on the same extreme inputs ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def extreme():
    """A pool of 33 of 60 users behind a user_pool (the sixteen-round permutation with cycle walking), B = 33, empty rows, a row with a
    repeated item, a heavy row that owns the negative range but two items, slots and pops, a top-bit seed, steps from 2^33 + 1."""
    rng = np.random.default_rng(11)
    n_users, n_items, T = 60, 96, 5
    rows = random_rows(rng, n_users, n_items, 12, empty_every=7)
    rows[3] = np.array([4, 4, 4, 50, 50, 51], np.int32)
    rows[10] = np.setdiff1d(np.arange(8, 90, dtype=np.int32), np.array([16, 70], np.int32))
    indptr, indices = csr_of(rows)
    pool = np.array([3, 10, 0] + [u for u in rng.permutation(n_users).tolist() if u not in (3, 10, 0)][:30], np.int32)
    assert len(set(pool.tolist())) == 33
    return dict(indptr=indptr, indices=indices, slots=rng.integers(0, T, len(indices)).astype(np.int32),
                pop=rng.uniform(0, 1, (n_items, T)).astype(np.float32), pool=pool, n_pool=33, B=33, neg_range=(16, 71), seed=TOP,
                step=(1 << 33) + 1, n_users=n_users, n_items=n_items)


def _extreme_on(dev, x):
    ip, ix, sl, pm, pl = to(dev, x["indptr"], x["indices"], x["slots"], x["pop"], x["pool"])
    return ip, ix, dict(user_pool=pl, n_pool=x["n_pool"], train_slots=sl, neg_range=x["neg_range"], pop_matrix=pm)


def _extreme_ref(x, step):
    return sr.sample(x["seed"], step, x["B"], x["indptr"], x["indices"], slots=x["slots"], user_pool=x["pool"], n_pool=x["n_pool"],
                     neg_range=x["neg_range"], pop_matrix=x["pop"])


def _bufs(dev, *shape):
    return (torch.empty(shape, dtype=torch.int32, device=dev), torch.empty(shape, dtype=torch.int32, device=dev),
            torch.empty(shape, dtype=torch.int32, device=dev), torch.empty(shape, device=dev), torch.empty(shape, device=dev))


def test_extreme_inputs_through_sample_triplets_into(dev, extreme):
    from pda_amd import ops
    x = extreme
    ip, ix, kw = _extreme_on(dev, x)
    ctr = torch.tensor([x["step"], 0], dtype=torch.int64, device=dev)
    out = ops.sample_triplets_into(_bufs(dev, x["B"]), ip, ix, seed=x["seed"], step_dev=ctr, parity=0, **kw)
    torch.cuda.synchronize()
    same(out, _extreme_ref(x, x["step"]), "sample_triplets_into")
    assert ctr.tolist() == [x["step"], x["step"] + 1]


def test_extreme_inputs_through_sample_batches_into(dev, extreme):
    from pda_amd import ops
    x = extreme
    ip, ix, kw = _extreme_on(dev, x)
    n = 3
    ctr = torch.tensor([0, x["step"]], dtype=torch.int64, device=dev)
    out = ops.sample_batches_into(_bufs(dev, n, x["B"]), ip, ix, seed=x["seed"], step_dev=ctr, parity=1, **kw)
    torch.cuda.synchronize()
    for j in range(n):
        same([t[j] for t in out], _extreme_ref(x, x["step"] + j), "sample_batches_into, batch %d" % j)
    assert ctr.tolist() == [x["step"] + n, x["step"]]


def test_extreme_inputs_through_the_step_that_samples_the_next_batch(dev, extreme):
    from pda_amd import ops
    x = extreme
    ip, ix, kw = _extreme_on(dev, x)
    rng = np.random.default_rng(2)
    U, I = to(dev, (rng.standard_normal((x["n_users"], 64)) * 0.1).astype(np.float32), (rng.standard_normal((x["n_items"], 64)) * 0.1).astype(np.float32))
    first = _extreme_ref(x, x["step"])
    cur = to(dev, *(first[k] for k in KEYS))
    nxt = _bufs(dev, x["B"])
    ctr = torch.tensor([x["step"] + 1, 0], dtype=torch.int64, device=dev)
    ops.bpr_step_and_sample(U, I, *cur, regs=1e-2, reg_div=x["B"], lr=0.05, next_out=nxt, train_indptr=ip, train_indices=ix, seed=x["seed"],
                            step_dev=ctr, parity=0, **kw)
    torch.cuda.synchronize()
    same(nxt, _extreme_ref(x, x["step"] + 1), "bpr_step_and_sample, next batch")
    assert ctr.tolist() == [x["step"] + 1, x["step"] + 2]


def test_the_triplet_sampler_has_no_cap_on_the_batch_where_the_ssm_sampler_has_one(dev, world):
    """B = 2^22 + 1: one row more than pda_ssm_sample takes (its [B, N] block is indexed in 32 bits).  The triplet sampler draws it; rows at
    both ends and in the middle equal the restatement.  The SSM sampler refuses it as an invalid argument."""
    from pda_amd import _lib, ops
    w = world
    B, n_pool, seed, step = (1 << 22) + 1, 5000, TOP, 5
    ip, ix = to(dev, w["indptr"], w["indices"])
    got = ops.sample_triplets(ip, ix, B, seed=seed, step=step, n_pool=n_pool, neg_range=(0, w["n_items"]))
    torch.cuda.synchronize()
    rows = np.concatenate([np.arange(64), np.arange(B // 2, B // 2 + 64), np.arange(B - 64, B)])
    ref = sr.sample(seed, step, B, w["indptr"], w["indices"], n_pool=n_pool, neg_range=(0, w["n_items"]), rows=rows)
    same([None if t is None else t[torch.from_numpy(rows).to(dev)] for t in got], ref, "B = 2^22 + 1")
    with pytest.raises(_lib.PdaHipError, match="invalid argument"):
        ops.ssm_sample(ip, ix, B, 1, seed=seed, step=step, neg_range=(0, w["n_items"]), n_pool=n_pool)
    u, p, n = ops.ssm_sample(ip, ix, 64, 1, seed=seed, step=step, neg_range=(0, w["n_items"]), n_pool=n_pool)      # (the call itself is sound)
    assert n.shape == (64, 1)
