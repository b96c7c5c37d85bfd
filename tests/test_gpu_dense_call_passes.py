"""The dense top-K call of the huge geometry without the passes its result does not need (pda_score_topk_v4.hip, pda_v5_sweep.h,
pda_score_topk.hip):

  * warm4_kernel writes the sweep's user image and padded norms (no uprep5_kernel launch): compared with uprep5_kernel's bytes;
  * the warm-up's sorted rows go to out_keys only (no hand-over copy), the sweep copies a row into its list slots the first time it
    appends to it: packed keys bit for bit against the exact kernel (impl="v1") on SMALL catalogues, where most rows are appended to;
  * pda_topk_merge with one list per user is an unpack: (idx, val) and keys against the general merge kernel on the same keys.

Every call goes through the library's own plan (no geometry is forced); the plan and the identity word the sweep kernel writes are
asserted to be the huge geometry's on every call."""
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
    for k in ("PDA_SCORE_LISTS", "PDA_SCORE_KERNEL", "PDA_HUGE_SPLITS", "PDA_SCORE_IMPL", "PDA_SCORE_PRUNE", "PDA_WARM_PER_SPLIT"):
        monkeypatch.delenv(k, raising=False)


def case(rng, nU, nI, d, max_hist=20, flat=True):
    """Popularities that fall slowly (flat: the thresholds of the warm-up's 256 items are passed by many items behind them: most rows are
    appended to, several times) and never tie; histories of up to max_hist items."""
    U = (rng.standard_normal((nU, d)) * 0.3).astype(F)
    I = (rng.standard_normal((nI, d)) * 0.3).astype(F)
    pop = (0.5 + 0.5 * rng.permutation(nI) / nI).astype(F) if flat else (0.998 ** np.arange(nI, dtype=np.float64)).astype(F)
    assert len(np.unique(pop)) == nI
    lens = rng.integers(0, max_hist + 1, nU)
    flat = np.unique(np.repeat(np.arange(nU, dtype=np.int64), lens) * nI + rng.integers(0, nI, int(lens.sum())))      # (row, item) pairs, no repeats
    rows = np.split((flat % nI).astype(np.int32), np.searchsorted(flat // nI, np.arange(1, nU)))
    assert len(rows) == nU
    return U, I, pop, rows


def bf16_exact(x):
    return torch.from_numpy(x).bfloat16().float().numpy()


def hist_of(dev, rows, users, by_user):
    """by user id: one row per user of the table; by block row: one row per row of the block"""
    from pda_amd import ops
    ip, ix = csr(rows if by_user else [rows[u] for u in users])
    return ops.HistoryCSR(torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev), by_user=by_user)


def dense_call(dev, U, I, pop, rows, users, by_user=True, bf16=False, want_splits=None):
    """-> (keys [n_splits, Bu, K] of the library's dense call, merged keys of the exact kernel, stats, (U, users) on the device)"""
    from pda_amd import ops
    nU, d = len(users), U.shape[1]
    Uf, If, pt = torch.from_numpy(U).to(dev), torch.from_numpy(I).to(dev), torch.from_numpy(pop).to(dev)
    Ut, It = (Uf.bfloat16(), If.bfloat16()) if bf16 else (Uf, If)
    ut = torch.from_numpy(np.asarray(users, dtype=np.int32)).to(dev)
    h = hist_of(dev, rows, users, by_user) if rows is not None else None
    plan = ops.score_plan(nU, I.shape[0], d, K, ops.HEAD_POP, "order", bf16, h)
    assert plan["kernel"] == "v4" and plan["early_stop"] & 128, plan            # PDA_SWEEP_HUGE, chosen by the library
    if want_splits is not None:
        assert (plan["n_splits"] > 1) == want_splits, plan
    st = {}
    got = ops.score_topk_keys(Ut, It, ut, K, ops.HEAD_POP, pt, h, 0, 0, impl="v2", prune="order", stats=st)
    ref = ops.topk_merge(ops.score_topk_keys(Uf, If, ut, K, ops.HEAD_POP, pt, h, 0, impl="v1"), want="keys")
    torch.cuda.synchronize()
    assert got.shape[0] == plan["n_splits"] == st["n_splits"]
    assert int(st["error"][0]) == 0
    ident = ops.kernel_identity(st["kernel_id"][0])
    assert ident["generation"] == 4 and ident["geometry"] == "huge" and ident["d"] == d and ident["bf16"] == bf16, ident
    return got, ref, st, (Ut, ut)


def assert_user_image(st, Ut, ut, nI):
    """the image and the norms the warm-up left in the call's workspace == uprep5_kernel's on the same block: BIT FOR BIT, both (the
    warm-up sums the squares in uprep5_kernel's order), the rows of the padding included (zeros, norm 0)"""
    from pda_amd import ops
    nU, d = ut.numel(), Ut.shape[1]
    o_img, o_norm, _, n_pad = ops.huge_image_offsets(nU, nI, d, st["n_splits"])
    ufrag, unorm = ops.huge_user_image(Ut, ut)
    ws = st["workspace"]
    assert ufrag.numel() == n_pad * 2 * d and unorm.numel() == n_pad
    assert torch.equal(ws[o_img:o_img + n_pad * 2 * d], ufrag)
    assert torch.equal(ws[o_norm:o_norm + 4 * n_pad].view(torch.int32), unorm.view(torch.int32))
    if n_pad > nU:
        n16 = -(-nU // 16) * 16                          # (the image is laid out by blocks of 16 users, 32 d bytes each)
        assert int(ws[o_img + n16 * 2 * d:o_img + n_pad * 2 * d].ne(0).sum()) == 0
        assert float(ws[o_norm + 4 * nU:o_norm + 4 * n_pad].view(torch.float32).abs().max()) == 0.0


def appended_fraction(got, st, nU):
    """exact rescorings per user behind the warm-up.  The cases must exercise the appends -- and do, by construction (`case`, flat): the
    warm-up sees the 256 most popular items (pop > 0.9 of at most 1), a row's K-th value is about the 80th percentile of their heads; the
    items behind have pop 0.5 .. 0.9 and the same score distribution (std 0.7 .. 1.4), so about a tenth of them -- a hundred and more per
    user -- reach the threshold.  The tests ask for 2 per user: every row appended to on average, many rows several times."""
    return float(st["pairs_rescored"][0]) / nU


# small catalogues (a few hundred to a few thousand items): most rows are appended to behind the warm-up -- the lazy row copy, compactions
# behind it, several lanes of one pass on one untouched row; user counts that are no multiples of 128 or 1 024; d, table type, history kind
@pytest.mark.parametrize("d,bf16", [(64, False), (128, False), (256, True), (128, True), (256, False)])
@pytest.mark.parametrize("by_user", [True, False])
def test_small_catalogue_keys_and_user_image(dev, d, bf16, by_user):
    from pda_amd import ops
    rng = np.random.default_rng(100 + d + (7 if bf16 else 0) + (1 if by_user else 0))
    nU, nI = 200005 + 37 * d, (700 if d == 256 else 1500)
    nT = nU + 500
    U, I, pop, rows = case(rng, nT, nI, d)
    if bf16:
        U, I = bf16_exact(U), bf16_exact(I)
    users = rng.permutation(nT)[:nU]
    got, ref, st, (Ut, ut) = dense_call(dev, U, I, pop, rows, users, by_user=by_user, bf16=bf16, want_splits=False)
    per_user = appended_fraction(got, st, nU)
    print("d %d bf16 %s: %.1f exact rescorings per user behind the warm-up" % (d, bf16, per_user))
    assert per_user > 2.0, per_user                      # (most rows are appended to, many more than once)
    assert nU % 128 != 0 and nU % 1024 != 0
    got = ops.topk_merge(got, want="keys")
    assert torch.equal(got, ref), int((got != ref).sum())
    assert_user_image(st, Ut, ut, nI)


# item splits with the shared warm-up: split 0 holds the warm-up's rows, the others start from empty lists
@pytest.mark.parametrize("d,bf16", [(64, False), (128, False), (256, True)])
@pytest.mark.parametrize("by_user", [True, False])
def test_item_splits_with_the_shared_warm_up(dev, d, bf16, by_user):
    from pda_amd import ops
    rng = np.random.default_rng(200 + d)
    nU, nI = 17003 + d, 20000
    U, I, pop, rows = case(rng, nU, nI, d)
    if bf16:
        U, I = bf16_exact(U), bf16_exact(I)
    got, ref, st, (Ut, ut) = dense_call(dev, U, I, pop, rows, np.arange(nU), by_user=by_user, bf16=bf16, want_splits=True)
    assert appended_fraction(got, st, nU) > 2.0
    got = ops.topk_merge(got, want="keys")
    assert torch.equal(got, ref), int((got != ref).sum())
    assert_user_image(st, Ut, ut, nI)


# rows with fewer than K unmasked items: the -inf prologue path of the sweep (keys counted from out_keys), lists that stay short, the
# fill of the unpack (train items, lowest id first) and its -1 / -inf slots -- with the history by user id and by block row
@pytest.mark.parametrize("by_user", [True, False])
def test_rows_with_fewer_than_K_unmasked_items(dev, by_user):
    from pda_amd import ops
    rng = np.random.default_rng(300)
    d, nI = 128, 1200
    nU = 200000 + 11
    U, I, pop, rows = case(rng, nU, nI, d, max_hist=6)
    order = np.argsort(-pop, kind="stable")
    short = {}
    for u, n_keep in ((0, 30), (5, 0), (130, 49), (1023, 1), (1024, 12), (nU - 1, 7), (77777, 50), (4096, 51)):
        # n_keep items stay unmasked: some among the warm-up's 256 items, some behind them (those reach the row through the sweep's appends)
        keep = np.concatenate([order[:256][: n_keep // 2], order[256:][rng.permutation(nI - 256)[: n_keep - n_keep // 2]]]).astype(np.int32)
        rows[u] = np.setdiff1d(np.arange(nI, dtype=np.int32), keep).astype(np.int32)
        short[u] = n_keep
    got, ref, st, (Ut, ut) = dense_call(dev, U, I, pop, rows, np.arange(nU), by_user=by_user, want_splits=False)
    assert got.shape[0] == 1
    merged = ops.topk_merge(got, want="keys")
    assert torch.equal(merged, ref), int((merged != ref).sum())
    h = hist_of(dev, rows, np.arange(nU), by_user)
    idx, val = ops.topk_merge(got, ut, h)
    gen_idx, gen_val = ops.topk_merge(torch.cat([got, torch.zeros_like(got)]), ut, h)      # (two lists, one of them empty: the general merge kernel)
    assert torch.equal(idx, gen_idx) and torch.equal(val.view(torch.int32), gen_val.view(torch.int32))
    idx, val, keys = idx.cpu().numpy(), val.cpu().numpy(), merged.cpu().numpy()
    for u, n_keep in short.items():
        n_real = min(n_keep, K)
        assert int((keys[u] != 0).sum()) == n_real, (u, n_keep)
        assert np.all(np.isfinite(val[u, :n_real])) and np.all(np.isneginf(val[u, n_real:]))
        assert np.array_equal(idx[u, n_real:], rows[u][:K - n_real]), u              # the fill: train items, lowest id first
        assert not set(idx[u, :n_real]) & set(rows[u])
    # without a history the empty slots stay -1 / -inf
    idx0, val0 = ops.topk_merge(got)
    idx0, val0 = idx0.cpu().numpy(), val0.cpu().numpy()
    for u, n_keep in short.items():
        n_real = min(n_keep, K)
        assert np.all(idx0[u, n_real:] == -1) and np.all(np.isneginf(val0[u, n_real:])) and np.array_equal(idx0[u, :n_real], idx[u, :n_real])
    assert_user_image(st, Ut, ut, nI)


# the R = 1 unpack against the general merge kernel on the same keys: full rows, short rows, empty rows, with and without a history,
# want="keys" (a plain copy), K that is no multiple of the kernel's four keys per thread and a total that is not either
@pytest.mark.parametrize("Kk,nU", [(50, 4099), (7, 1001), (33, 515), (1, 77), (54, 3)])
@pytest.mark.parametrize("by_user", [True, False, None])
def test_unpack_of_one_list_equals_the_general_merge(dev, Kk, nU, by_user):
    from pda_amd import ops
    rng = np.random.default_rng(400 + Kk)
    nI = 5000
    val = np.sort(rng.uniform(0.01, 3.0, (nU, Kk)).astype(F), axis=1)[:, ::-1]
    item = np.stack([rng.permutation(nI)[:Kk] for _ in range(nU)]).astype(np.uint64)
    keys = (val.copy().view(np.uint32).astype(np.uint64) | np.uint64(0x80000000)) << np.uint64(32) | (np.uint64(0xFFFFFFFF) - item)
    n_real = rng.integers(0, Kk + 1, nU)
    n_real[rng.random(nU) < 0.6] = Kk
    keys[np.arange(Kk)[None, :] >= n_real[:, None]] = 0
    kt = torch.from_numpy(keys.view(np.int64)).to(dev).reshape(1, nU, Kk)
    users = rng.permutation(nU + 50)[:nU].astype(np.int32)
    ut = torch.from_numpy(users).to(dev)
    h = None
    if by_user is not None:
        rows = [np.unique(rng.integers(0, nI, rng.integers(0, 2 * Kk + 2))).astype(np.int32) for _ in range(nU + 50)]
        h = hist_of(dev, rows, users, by_user)
    two = torch.cat([kt, torch.zeros_like(kt)])
    idx, v = ops.topk_merge(kt, ut, h)
    gidx, gv = ops.topk_merge(two, ut, h)
    assert torch.equal(idx, gidx), int((idx != gidx).sum())
    assert torch.equal(v.view(torch.int32), gv.view(torch.int32))
    assert torch.equal(ops.topk_merge(kt, want="keys"), kt[0])
    assert torch.equal(ops.topk_merge(two, want="keys"), kt[0])
    ii, vv = idx.cpu().numpy(), v.cpu().numpy()
    full = n_real == Kk
    assert np.array_equal(ii[full], item[full].astype(np.int32)) and np.array_equal(vv[full], val[full])
    if h is None:
        assert np.all(ii[np.arange(Kk)[None, :] >= n_real[:, None]] == -1)
