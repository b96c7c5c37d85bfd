"""The warm-position masks once per history and visiting order (pda_score_topk_v4.hip: warm_mask_table4_kernel, warm4_kernel's gather;
pda_amd/ops.py: warm_mask_table):

  * the table's rows at users[row] against warm_mask4_kernel's words for the block, bit for bit, and both against the bits worked out
    here from the visiting order -- empty rows, repeated users, users in descending order, blocks below and above the 98 304 users from
    which the per-call kernel is a launch of its own, an item shard with item_offset > 0, warm-ups of 2 and 4 tiles;
  * keys of a call that gathers from the table == keys with PDA_WARM_MASK_TABLE=0 == the exact kernel (impl="v1"), early-terminating
    and dense sweeps;
  * a call handed an altered table returns what that table says: the library reads it and does not quietly walk the histories instead;
  * the cache: one table per history and order, a new one for another order, none for a history by block row or beyond the budget."""
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
    for k in ("PDA_SCORE_LISTS", "PDA_SCORE_KERNEL", "PDA_HUGE_SPLITS", "PDA_SCORE_IMPL", "PDA_SCORE_PRUNE", "PDA_WARM_PER_SPLIT", "PDA_WARM_MASK_TABLE"):
        monkeypatch.delenv(k, raising=False)


def hot_case(rng, nT, nI, d, item_offset=0, nloc=None):
    """Tables, a never-tying popularity and histories (GLOBAL ids) in which every user but each 17th has 2 .. 7 of the shard's 256 most
    popular items and up to 12 others; each 17th row is empty."""
    nloc = nI - item_offset if nloc is None else nloc
    U = (rng.standard_normal((nT, d)) * 0.3).astype(F)
    I = (rng.standard_normal((nI, d)) * 0.3).astype(F)
    pop = (0.5 + 0.5 * rng.permutation(nI) / nI).astype(F)
    hot = item_offset + np.argsort(-pop[item_offset:item_offset + nloc], kind="stable")[:256]
    n_hot, n_any = rng.integers(2, 8, nT), rng.integers(0, 13, nT)
    n_hot[::17] = 0
    n_any[::17] = 0
    items = np.concatenate([hot[rng.integers(0, len(hot), int(n_hot.sum()))], rng.integers(0, nI, int(n_any.sum()))])
    owner = np.concatenate([np.repeat(np.arange(nT, dtype=np.int64), n_hot), np.repeat(np.arange(nT, dtype=np.int64), n_any)])
    flat = np.unique(owner * nI + items)
    rows = np.split((flat % nI).astype(np.int32), np.searchsorted(flat // nI, np.arange(1, nT)))
    assert len(rows) == nT and len(rows[0]) == 0 and len(rows[1]) >= 1
    return U, I, pop, rows


def expected_words(rows, users, pop, item_offset, nloc, warm_tiles):
    """uint32 [len(users), 8]: bit (pos & 31) of word (pos >> 5) for every train item of the shard at visiting position pos < 64 warm_tiles"""
    order = np.argsort(-np.abs(pop[item_offset:item_offset + nloc]), kind="stable")
    pos_of = np.empty(nloc, np.int64)
    pos_of[order] = np.arange(nloc)
    out = np.zeros((len(users), 8), np.uint32)
    for r, u in enumerate(users):
        loc = rows[u].astype(np.int64) - item_offset
        pos = pos_of[loc[(loc >= 0) & (loc < nloc)]]
        for p in pos[pos < 64 * warm_tiles]:
            out[r, p >> 5] |= np.uint32(1) << np.uint32(p & 31)
    return out


def block_users(rng, nT, nU, kind):
    users = rng.permutation(nT)[:nU].astype(np.int32)
    if kind == "repeats":
        users[nU // 2:nU // 2 + 40] = users[:40]            # forty users twice in the block
        users[-1] = users[-2]
    else:
        users = np.sort(users)[::-1].copy()                 # descending ids
    return users


@pytest.mark.parametrize("nU,warm_tiles,item_offset,kind", [(1000, 4, 0, "repeats"), (1000, 2, 300, "descending"),
                                                           (100000, 4, 300, "repeats"), (100000, 2, 0, "descending")])
def test_table_rows_equal_the_per_call_kernel(dev, monkeypatch, nU, warm_tiles, item_offset, kind):
    from pda_amd import ops
    rng = np.random.default_rng(nU + warm_tiles)
    d, nI = 64, 2300
    nloc = nI - item_offset - (100 if item_offset else 0)
    nT = nU + 333
    U, I, pop, rows = hot_case(rng, nT, nI, d, item_offset, nloc)
    users = block_users(rng, nT, nU, kind)
    ip, ix = csr(rows)
    h = ops.HistoryCSR(torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev), by_user=True)
    Ish = torch.from_numpy(I[item_offset:item_offset + nloc].copy()).to(dev)
    psh = torch.from_numpy(pop[item_offset:item_offset + nloc].copy()).to(dev)
    ut = torch.from_numpy(users).to(dev)
    order = ops.visiting_order(Ish, psh)
    prep = ops.item_prep4(Ish, psh, order)
    tab = ops.warm_mask_table(h, prep, order, item_offset, nloc, d)
    assert tab is not None and tuple(tab.shape) == (nT, 8)
    per_call = ops.warm_mask_rows(prep, ut, h, item_offset, nloc, d, warm_tiles)
    torch.cuda.synchronize()
    nw = 2 * warm_tiles
    gathered = tab[ut.long()][:, :nw].cpu().numpy().view(np.uint32)
    kernel = per_call.cpu().numpy().view(np.uint32)
    want = expected_words(rows, users, pop, item_offset, nloc, warm_tiles)
    assert np.array_equal(kernel[:nU, :nw], want[:, :nw])
    assert np.array_equal(gathered, want[:, :nw])
    assert not kernel[nU:].any() and not kernel[:, nw:].any()                   # the padding rows; the words behind a shorter warm-up
    full = tab.cpu().numpy().view(np.uint32)
    assert np.array_equal(full, expected_words(rows, np.arange(nT), pop, item_offset, nloc, 4))      # every row, whole table: 4 tiles
    assert (want.any(axis=1) | (np.array([len(rows[u]) for u in users]) == 0)).mean() > 0.9          # (the rows carry bits)
    if nU >= 98304:
        # the words warm_mask4_kernel leaves in the workspace of a product call without the table: the new offsets query
        monkeypatch.setenv("PDA_WARM_MASK_TABLE", "0")
        st = {}
        Ut = torch.from_numpy(U).to(dev)
        ops.score_topk_keys(Ut, Ish, ut, K, ops.HEAD_POP, psh, h, item_offset, 0, impl="v2", prune="order", stats=st, warm_tiles=warm_tiles)
        torch.cuda.synchronize()
        assert st["warm_mask_table"] is None and int(st["error"][0]) == 0
        off, nbytes = ops.warm_mask_offsets(nU, nloc, d, st["n_splits"])
        assert nbytes >= per_call.numel() * 4
        in_ws = st["workspace"][off:off + per_call.numel() * 4].view(torch.int32).reshape(-1, 8).cpu().numpy().view(np.uint32)
        assert np.array_equal(in_ws, kernel)


def keys_three_ways(dev, monkeypatch, U, I, pop, h, ut, prune):
    """-> (merged keys with the table, with PDA_WARM_MASK_TABLE=0, of the exact kernel, the stats of the first)"""
    from pda_amd import ops
    Ut, It, pt = torch.from_numpy(U).to(dev), torch.from_numpy(I).to(dev), torch.from_numpy(pop).to(dev)
    st, st0 = {}, {}
    with_tab = ops.topk_merge(ops.score_topk_keys(Ut, It, ut, K, ops.HEAD_POP, pt, h, 0, 0, impl="v2", prune=prune, stats=st), want="keys")
    monkeypatch.setenv("PDA_WARM_MASK_TABLE", "0")
    without = ops.topk_merge(ops.score_topk_keys(Ut, It, ut, K, ops.HEAD_POP, pt, h, 0, 0, impl="v2", prune=prune, stats=st0), want="keys")
    monkeypatch.delenv("PDA_WARM_MASK_TABLE")
    ref = ops.topk_merge(ops.score_topk_keys(Ut, It, ut, K, ops.HEAD_POP, pt, h, 0, impl="v1"), want="keys")
    torch.cuda.synchronize()
    assert int(st["error"][0]) == 0 and int(st0["error"][0]) == 0
    assert ops.kernel_identity(st["kernel_id"][0])["generation"] == 4
    assert st0["warm_mask_table"] is None
    return with_tab, without, ref, st


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("prune", [True, "order"])
@pytest.mark.parametrize("nU", [1100, 100003])
def test_keys_with_the_table_without_it_and_exact(dev, monkeypatch, d, prune, nU):
    from pda_amd import ops
    rng = np.random.default_rng(d + nU)
    nI, nT = 1500, nU + 77
    U, I, pop, rows = hot_case(rng, nT, nI, d)
    users = block_users(rng, nT, nU, "repeats")
    ip, ix = csr(rows)
    h = ops.HistoryCSR(torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev), by_user=True)
    ut = torch.from_numpy(users).to(dev)
    with_tab, without, ref, st = keys_three_ways(dev, monkeypatch, U, I, pop, h, ut, prune)
    assert st["warm_mask_table"] is not None and st["warm_mask_table"] is h._warm_mask_cache[-1][-1]
    assert torch.equal(with_tab, ref), int((with_tab != ref).sum())
    assert torch.equal(without, ref), int((without != ref).sum())


# The library may decline a table it was handed (run_score4's conditions) and walk the histories as before, with the same keys: equal keys
# and a table in the stats do not show that the table was READ.  So the call is handed an altered table -- every bit set: all 256 warm
# positions count as train items of every user -- and must return what that table says: the exact kernel's keys for histories to which the
# 256 most popular items were added.  (The sweep behind the warm-up visits positions >= 256 only, where the CSR decides as before.)
@pytest.mark.parametrize("prune", [True, "order"])
@pytest.mark.parametrize("nU", [1100, 100003])
def test_an_altered_table_changes_the_keys(dev, monkeypatch, prune, nU):
    from pda_amd import ops
    rng = np.random.default_rng(nU + 5)
    d, nI, nT = 64, 1500, nU + 77
    U, I, pop, rows = hot_case(rng, nT, nI, d)
    users = block_users(rng, nT, nU, "repeats")
    ip, ix = csr(rows)
    h = ops.HistoryCSR(torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev), by_user=True)
    hot = np.argsort(-pop, kind="stable")[:256].astype(np.int32)
    ipa, ixa = csr([np.union1d(r, hot).astype(np.int32) for r in rows])
    h_all = ops.HistoryCSR(torch.from_numpy(ipa).to(dev), torch.from_numpy(ixa).to(dev), by_user=True)
    ut = torch.from_numpy(users).to(dev)
    Ut, It, pt = torch.from_numpy(U).to(dev), torch.from_numpy(I).to(dev), torch.from_numpy(pop).to(dev)
    real = ops.warm_mask_table
    monkeypatch.setattr(ops, "warm_mask_table", lambda *a: torch.full_like(real(*a), -1))
    st = {}
    got = ops.topk_merge(ops.score_topk_keys(Ut, It, ut, K, ops.HEAD_POP, pt, h, 0, 0, impl="v2", prune=prune, stats=st), want="keys")
    ref = ops.topk_merge(ops.score_topk_keys(Ut, It, ut, K, ops.HEAD_POP, pt, h, 0, impl="v1"), want="keys")
    ref_all = ops.topk_merge(ops.score_topk_keys(Ut, It, ut, K, ops.HEAD_POP, pt, h_all, 0, impl="v1"), want="keys")
    torch.cuda.synchronize()
    assert int(st["error"][0]) == 0 and ops.kernel_identity(st["kernel_id"][0])["generation"] == 4
    assert not torch.equal(ref, ref_all)
    assert not torch.equal(got, ref), "the call did not read the table it was handed"
    assert torch.equal(got, ref_all), int((got != ref_all).sum())


def test_cache_one_table_per_history_and_order(dev, monkeypatch):
    from pda_amd import ops
    rng = np.random.default_rng(7)
    d, nI, nU = 64, 1500, 1100
    nT = nU + 77
    U, I, pop, rows = hot_case(rng, nT, nI, d)
    users = block_users(rng, nT, nU, "repeats")
    ip, ix = csr(rows)
    ut = torch.from_numpy(users).to(dev)
    Ut, It, pt = torch.from_numpy(U).to(dev), torch.from_numpy(I).to(dev), torch.from_numpy(pop).to(dev)
    h = ops.HistoryCSR(torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev), by_user=True)

    def call(pop_t, hist, impl="v2"):
        st = {}
        keys = ops.score_topk_keys(Ut, It, ut, K, ops.HEAD_POP, pop_t, hist, 0, 0 if impl == "v2" else 1, impl=impl, prune="order", stats=st)
        return ops.topk_merge(keys, want="keys"), st

    k1, st1 = call(pt, h)
    k1b, st1b = call(pt, h)
    assert st1["warm_mask_table"] is not None and st1b["warm_mask_table"] is st1["warm_mask_table"]          # built once
    assert torch.equal(k1, call(pt, h, "v1")[0]) and torch.equal(k1b, k1)
    # another popularity, another order: a new table (the old one goes), that order's keys
    pop2 = pop[::-1].copy()
    pt2 = torch.from_numpy(pop2).to(dev)
    k2, st2 = call(pt2, h)
    assert st2["warm_mask_table"] is not None and st2["warm_mask_table"] is not st1["warm_mask_table"]
    assert len(h._warm_mask_cache) == 1
    assert not torch.equal(st2["warm_mask_table"], st1["warm_mask_table"])
    got2 = st2["warm_mask_table"].cpu().numpy().view(np.uint32)
    assert np.array_equal(got2, expected_words(rows, np.arange(nT), pop2, 0, nI, 4))
    assert torch.equal(k2, call(pt2, h, "v1")[0])
    # a history by block row builds none
    ipb, ixb = csr([rows[u] for u in users])
    hb = ops.HistoryCSR(torch.from_numpy(ipb).to(dev), torch.from_numpy(ixb).to(dev), by_user=False)
    kb, stb = call(pt, hb)
    assert stb["warm_mask_table"] is None and not hb.__dict__.get("_warm_mask_cache")
    assert torch.equal(kb, k1)
    # a table beyond the budget is not built: the call keeps its per-call walk
    h3 = ops.HistoryCSR(torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev), by_user=True)
    monkeypatch.setattr(ops, "WARM_MASK_TABLE_BUDGET", 32 * nT - 1)
    k3, st3 = call(pt, h3)
    assert st3["warm_mask_table"] is None and not h3.__dict__.get("_warm_mask_cache")
    assert torch.equal(k3, k1)
    monkeypatch.setattr(ops, "WARM_MASK_TABLE_BUDGET", 32 * nT)
    assert call(pt, h3)[1]["warm_mask_table"] is not None
    torch.cuda.synchronize()
