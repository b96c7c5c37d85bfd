"""The dense call's exact warm-up as a score kernel and a select kernel (warm_score5_kernel, warm_select5_kernel in
pda_score_topk_v4.hip) against the one-kernel warm-up it replaces (warm4_kernel, PDA_WARM_ONE_KERNEL=1) and the exact kernel (impl="v1").

Every case asserts, bit for bit: the keys of the two warm-ups and of impl="v1"; the user image, the padded norms and the K-th values of the
warm-up's rows in the two workspaces; tiles_scored >= tiles_dense; and the witness (workspace + 32: 0 = warm4_kernel, 5 = the two kernels).
The identity word of the sweep is asserted to be the huge geometry's on every call that sweeps.

The library's plan gives the huge geometry to blocks of 4 096 users and more (pda_score_topk_plan).  The small blocks below -- no multiple
of 32, 256 or 1 024 users -- ask for it with PDA_SCORE_LISTS=huge and their own split count, as tests/test_gpu_score_topk.py -k k4huge
does; test_through_the_plan runs one block as the plan itself lays it out.

A wave of warm_score5_kernel runs a second unit of 32 users only in blocks of more than 8 waves x 256 workgroups x 32 = 65 536 users (one
workgroup per CU, the units dealt out over workgroups first), a third one beyond 131 072: test_second_and_third_pass has those blocks, on a
catalogue of 320 items.  In the blocks of 1 000 .. 17 067 users every wave runs one unit or none."""
import numpy as np
import pytest
import torch

from decided_tail_cases import csr

pytestmark = pytest.mark.gpu
K = 50
F = np.float32


@pytest.fixture(autouse=True)
def checked(monkeypatch):
    monkeypatch.setenv("PDA_CHECK_SWEEP_ERRORS", "1")
    for k in ("PDA_SCORE_LISTS", "PDA_SCORE_KERNEL", "PDA_HUGE_SPLITS", "PDA_SCORE_IMPL", "PDA_SCORE_PRUNE", "PDA_WARM_PER_SPLIT", "PDA_WARM_ONE_KERNEL",
              "PDA_WARM_MASK_TABLE", "PDA_WARM_TILES"):
        monkeypatch.delenv(k, raising=False)


def flat_case(rng, nU, nI, d, max_hist=20):
    """Popularities that fall slowly and never tie (most rows are appended to behind the warm-up); histories of up to max_hist items."""
    U = (rng.standard_normal((nU, d)) * 0.3).astype(F)
    I = (rng.standard_normal((nI, d)) * 0.3).astype(F)
    pop = (0.5 + 0.5 * rng.permutation(nI) / nI).astype(F)
    assert len(np.unique(pop)) == nI
    rows = [np.unique(rng.integers(0, nI, rng.integers(0, max_hist + 1))).astype(np.int32) for _ in range(nU)]
    return U, I, pop, rows


def bf16_exact(x):
    return torch.from_numpy(x).bfloat16().float().numpy()


def hist_of(dev, rows, users, by_user):
    from pda_amd import ops
    ip, ix = csr(rows if by_user else [rows[u] for u in users])
    return ops.HistoryCSR(torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev), by_user=by_user)


def both_warm_ups(dev, monkeypatch, U, I, pop, rows, users, by_user=True, bf16=False, n_splits=1, through_plan=False, two_kernels=True, sweeps=True,
                  ref_rows=None):
    """Runs the dense call with the two-kernel warm-up, with PDA_WARM_ONE_KERNEL=1 and the exact kernel; asserts everything the module's
    docstring lists.  n_splits: forced together with the huge geometry, unless through_plan.  two_kernels: what the witness of the default
    call must say.  ref_rows: the rows compared with impl="v1" (None: all).  -> (merged keys, reference keys, stats of the default call)"""
    from pda_amd import ops
    nU, nI, d = len(users), I.shape[0], U.shape[1]
    Uf, If, pt = torch.from_numpy(U).to(dev), torch.from_numpy(I).to(dev), torch.from_numpy(pop).to(dev)
    Ut, It = (Uf.bfloat16(), If.bfloat16()) if bf16 else (Uf, If)
    ut = torch.from_numpy(np.asarray(users, dtype=np.int32)).to(dev)
    h = hist_of(dev, rows, users, by_user) if rows is not None else None
    if through_plan:
        plan = ops.score_plan(nU, nI, d, K, ops.HEAD_POP, "order", bf16, h)
        assert plan["kernel"] == "v4" and plan["early_stop"] & 128, plan
        ns_arg = 0
    else:
        monkeypatch.setenv("PDA_SCORE_LISTS", "huge")
        ns_arg = n_splits

    def call(one_kernel):
        if one_kernel:
            monkeypatch.setenv("PDA_WARM_ONE_KERNEL", "1")
        else:
            monkeypatch.delenv("PDA_WARM_ONE_KERNEL", raising=False)
        st = {}
        got = ops.score_topk_keys(Ut, It, ut, K, ops.HEAD_POP, pt, h, 0, ns_arg, impl="v2", prune="order", stats=st)
        torch.cuda.synchronize()
        assert int(st["error"][0]) == 0
        if sweeps:
            ident = ops.kernel_identity(st["kernel_id"][0])
            assert ident["generation"] == 4 and ident["geometry"] == "huge" and ident["d"] == d and ident["bf16"] == bf16, ident
        assert int(st["tiles_scored"][0]) >= st["tiles_dense"], (int(st["tiles_scored"][0]), st["tiles_dense"])
        return got, st

    new, st_new = call(False)
    old, st_old = call(True)
    monkeypatch.delenv("PDA_WARM_ONE_KERNEL", raising=False)
    assert int(st_new["warm_kernels"][0]) == (5 if two_kernels else 0), int(st_new["warm_kernels"][0])
    assert int(st_old["warm_kernels"][0]) == 0
    assert new.shape == old.shape and st_new["n_splits"] == st_old["n_splits"]
    assert torch.equal(new, old), int((new != old).sum())
    ref = ops.topk_merge(ops.score_topk_keys(Uf, If, ut, K, ops.HEAD_POP, pt, h, 0, impl="v1"), want="keys")
    merged = ops.topk_merge(new, want="keys")
    if ref_rows is None:
        assert torch.equal(merged, ref), int((merged != ref).sum())
    else:
        sel = torch.from_numpy(np.asarray(ref_rows)).to(dev)
        assert torch.equal(merged[sel], ref[sel]), int((merged[sel] != ref[sel]).sum())
    if sweeps:
        # the user image, the padded norms, the K-th values of the warm-up's rows (split 0) and, under a shared warm-up, the seed
        S = st_new["n_splits"]
        o_img, o_norm, o_kth, n_pad = ops.huge_image_offsets(nU, nI, d, S)
        wn, wo = st_new["workspace"], st_old["workspace"]
        assert wn.numel() == wo.numel()
        assert torch.equal(wn[o_img:o_img + n_pad * 2 * d], wo[o_img:o_img + n_pad * 2 * d])
        assert torch.equal(wn[o_norm:o_norm + 4 * n_pad], wo[o_norm:o_norm + 4 * n_pad])
        assert torch.equal(wn[o_kth:o_kth + 4 * nU], wo[o_kth:o_kth + 4 * nU])
        if S > 1:
            o_seed = o_kth - (4 * nU + 255) // 256 * 256             # (the seed lies in front of the K-th values, 256-byte aligned)
            assert torch.equal(wn[o_seed:o_seed + 4 * nU], wo[o_seed:o_seed + 4 * nU])
            assert torch.equal(wn[o_seed:o_seed + 4 * nU], wn[o_kth:o_kth + 4 * nU])
    return merged, ref, st_new


# user counts that are no multiple of 32, 256 or 1 024 (2 050: 68 units in 68 workgroups, a ragged last one); d and table
# type; the history by user id (the table of all users) and by block row (warm_mask4_kernel in front); two catalogues
@pytest.mark.parametrize("nI", [700, 1500])
@pytest.mark.parametrize("by_user", [True, False])
@pytest.mark.parametrize("d,bf16", [(64, False), (128, False), (64, True), (128, True)])
@pytest.mark.parametrize("nU", [1000, 1100, 2050])
def test_small_blocks(dev, monkeypatch, nU, d, bf16, by_user, nI):
    rng = np.random.default_rng(nU + d + nI + (7 if bf16 else 0) + (1 if by_user else 0))
    nT = nU + 300
    U, I, pop, rows = flat_case(rng, nT, nI, d)
    if bf16:
        U, I = bf16_exact(U), bf16_exact(I)
    users = rng.permutation(nT)[:nU]
    _, _, st = both_warm_ups(dev, monkeypatch, U, I, pop, rows, users, by_user=by_user, bf16=bf16)
    assert float(st["pairs_rescored"][0]) / nU > 2.0           # (the sweep behind the warm-up appends to most rows)


_BIG = {}


def big_case(nT, nI):
    """flat_case for blocks of many users, built once with numpy alone: U and I at d = 128 (d = 64: their first 64 columns), histories of
    0 .. 12 items, one sorted array per user"""
    if (nT, nI) not in _BIG:
        rng = np.random.default_rng(nT + nI)
        U = (rng.standard_normal((nT, 128)) * 0.3).astype(F)
        I = (rng.standard_normal((nI, 128)) * 0.3).astype(F)
        pop = (0.5 + 0.5 * rng.permutation(nI) / nI).astype(F)
        draws = np.sort(rng.integers(0, nI, (nT, 12)), axis=1)
        keep = np.arange(12)[None, :] < rng.integers(0, 13, nT)[:, None]
        keep[:, 1:] &= draws[:, 1:] != draws[:, :-1]                    # (sorted, no item twice in a row)
        indptr = np.zeros(nT + 1, dtype=np.int64)
        indptr[1:] = np.cumsum(keep.sum(1))
        _BIG[(nT, nI)] = (U, I, pop, np.split(draws[keep].astype(np.int32), indptr[1:-1]))
    return _BIG[(nT, nI)]


# blocks in which the waves of warm_score5_kernel run a second unit (70 001 users: 2 188 units, 140 of them in the second register set,
# the ragged last one among them) and a third (140 003 users: 4 376 units, the ragged last one back in the first set, with the hand-over
# between the sets on both sides): every row's keys, image, norm and K-th value against warm4_kernel's, the keys against impl="v1"
@pytest.mark.parametrize("by_user", [True, False])
@pytest.mark.parametrize("d,bf16", [(64, False), (128, False), (64, True), (128, True)])
@pytest.mark.parametrize("nU", [70001, 140003])
def test_second_and_third_pass(dev, monkeypatch, nU, d, bf16, by_user):
    nI = 320
    U, I, pop, rows = big_case(140003 + 300, nI)
    U, I = np.ascontiguousarray(U[:, :d]), np.ascontiguousarray(I[:, :d])
    if bf16:
        U, I = bf16_exact(U), bf16_exact(I)
    users = np.random.default_rng(nU + d).permutation(U.shape[0])[:nU]
    _, _, st = both_warm_ups(dev, monkeypatch, U, I, pop, rows, users, by_user=by_user, bf16=bf16)
    assert (nU + 127) // 128 * 4 > (2 if nU > 131072 else 1) * 8 * torch.cuda.get_device_properties(dev).multi_processor_count


def test_without_a_history(dev, monkeypatch):
    rng = np.random.default_rng(11)
    U, I, pop, _ = flat_case(rng, 1100, 700, 64)
    both_warm_ups(dev, monkeypatch, U, I, pop, None, np.arange(1100))


def test_through_the_plan(dev, monkeypatch):
    """a block the library's plan gives to the huge geometry by itself (item splits behind a shared warm-up)"""
    rng = np.random.default_rng(12)
    nU, nI, d = 17067, 20000, 64            # (the block of tests/test_gpu_dense_call_passes.py's item-split cases)
    U, I, pop, rows = flat_case(rng, nU, nI, d)
    _, _, st = both_warm_ups(dev, monkeypatch, U, I, pop, rows, np.arange(nU), through_plan=True)
    assert st["n_splits"] > 1


# rows with 0 .. 51 unmasked items among the first 256 positions: short rows, -inf K-th values, zero fill
@pytest.mark.parametrize("by_user", [True, False])
def test_short_rows(dev, monkeypatch, by_user):
    rng = np.random.default_rng(21)
    nU, nI, d = 1100, 1500, 128
    U, I, pop, rows = flat_case(rng, nU, nI, d, max_hist=6)
    front = np.argsort(-pop, kind="stable")[:256].astype(np.int32)
    for n_keep in range(52):
        u = 3 + 20 * n_keep
        masked = front[rng.permutation(256)[n_keep:]]
        # (the user's drawn history keeps its items behind the warm-up only: exactly n_keep of the 256 stay unmasked)
        rows[u] = np.union1d(np.setdiff1d(rows[u], front), masked).astype(np.int32)
        assert 256 - len(np.intersect1d(rows[u], front)) == n_keep
    rows[7] = np.arange(nI, dtype=np.int32)                     # nothing at all: an empty row
    from pda_amd import ops
    merged, _, st = both_warm_ups(dev, monkeypatch, U, I, pop, rows, np.arange(nU), by_user=by_user)
    assert int((merged[7] != 0).sum()) == 0
    # the K-th values the warm-up left: -inf exactly for the rows with fewer than K unmasked items among the first 256
    o_kth = ops.huge_image_offsets(nU, nI, d, 1)[2]
    kth = st["workspace"][o_kth:o_kth + 4 * nU].view(torch.float32).cpu().numpy()
    for n_keep in range(52):
        assert np.isneginf(kth[3 + 20 * n_keep]) == (n_keep < K), n_keep
    assert np.isneginf(kth[7])


# the split ends just behind the warm-up (288, 320 items); 256 items: the call ends inside the warm-up and is the old one's
@pytest.mark.parametrize("nI", [288, 320, 256])
def test_split_boundaries(dev, monkeypatch, nI):
    rng = np.random.default_rng(30 + nI)
    nU, d = 1000, 64
    U, I, pop, rows = flat_case(rng, nU, nI, d)
    both_warm_ups(dev, monkeypatch, U, I, pop, rows, np.arange(nU), two_kernels=nI > 256, sweeps=nI > 256)


# several item splits behind the shared warm-up: the seed of the other splits
@pytest.mark.parametrize("by_user", [True, False])
def test_shared_warm_up(dev, monkeypatch, by_user):
    rng = np.random.default_rng(40)
    nU, nI, d = 5000, 20000, 128
    U, I, pop, rows = flat_case(rng, nU, nI, d)
    _, _, st = both_warm_ups(dev, monkeypatch, U, I, pop, rows, np.arange(nU), by_user=by_user, n_splits=4)
    assert st["n_splits"] == 4


def tie_case(seed, nU, nI, d):
    """100 of the 256 most popular items are copies of one row with one popularity, the largest of all"""
    rng = np.random.default_rng(seed)
    U, I, pop, rows = flat_case(rng, nU, nI, d, max_hist=6)
    front = np.argsort(-pop, kind="stable")[:256]
    copies = np.sort(front[rng.permutation(256)[:100]])
    I[copies] = I[copies[0]]
    pop[copies] = pop.max()
    assert np.all(np.isin(copies, np.argsort(-pop, kind="stable")[:256]))
    return U, I, pop, rows, copies


# more than kCap4 equal scores at the K-th value: the descent goes on over the item ids, the smaller ids win
@pytest.mark.parametrize("d", [64, 128])
def test_ties_at_the_kth_value(dev, monkeypatch, d):
    nU, nI = 1000, 1500
    U, I, pop, rows, copies = tie_case(50, nU, nI, d)
    merged, ref, _ = both_warm_ups(dev, monkeypatch, U, I, pop, rows, np.arange(nU))
    # the reference alone: on at least one row in ten the copied head is the row's K-th value (and the copies are cut there)
    r = ref.cpu().numpy().view(np.uint64)
    kth_item = (np.uint64(0xFFFFFFFF) - (r[:, K - 1] & np.uint64(0xFFFFFFFF))).astype(np.int64)
    at_kth = np.isin(kth_item, copies) & (r[:, K - 1] != 0)
    print("rows whose K-th value is the copied head: %d of %d" % (int(at_kth.sum()), nU))
    assert at_kth.mean() >= 0.1, at_kth.mean()
    # the order among the copies: ascending item ids, in the reference and therefore in the keys
    items = (np.uint64(0xFFFFFFFF) - (merged.cpu().numpy().view(np.uint64) & np.uint64(0xFFFFFFFF))).astype(np.int64)
    for u in np.nonzero(at_kth)[0][:50]:
        mine = items[u][np.isin(items[u], copies)]
        assert np.all(np.diff(mine) > 0), u


# a NaN user row (no score ranks) and a user row whose scores are all +inf or 0 (an infinite component): the keys of the one-kernel warm-up.
# A user row of -inf components is among them.  No SCORE is ever -inf: the head is (s > 0 ? s + 1 : exp(s)) x pop, ops rejects negative
# popularities (ops._check_pop: the head's bounds are derived for pop >= 0), and exp(-inf) x pop = 0 -- a dot product of -inf gives the
# score 0, the lowest a candidate can have, so the bisection's floor is pda_ordf(0), never pda_ordf(-inf).  Row 200 below has such scores:
# 0 where every product is -inf, NaN (no candidate) where the products' signs mix.
def test_non_finite_user_rows(dev, monkeypatch):
    rng = np.random.default_rng(60)
    nU, nI, d = 1100, 700, 64
    U, I, pop, rows = flat_case(rng, nU, nI, d)
    U[5] = np.nan
    U[70, 3] = -np.inf
    U[1099, 0] = np.inf
    U[200] = -np.inf
    I[:40] = np.abs(I[:40])                                     # (items whose dot product with row 200 is -inf, not NaN: scores of 0)
    finite = np.setdiff1d(np.arange(nU), [5, 70, 200, 1099])
    both_warm_ups(dev, monkeypatch, U, I, pop, rows, np.arange(nU), ref_rows=finite)

