"""GPU parity of deep lists on item shards: pda_deep_merge against numpy bit for bit, the fold of ops.deep_merge, emulated shards
(ops.deep_shard_keys over dist.shard_range + ops.deep_merge) against the CPU oracle and against the one-GPU deep call on the whole catalogue,
short rows across shards, and the model wrapper with an ItemShardedTopK."""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from test_dist_gloo import _pack, _unpack
from test_gpu_score_topk import csr, make_case

pytestmark = pytest.mark.gpu

N_ROWS = 37
KINDS = ("one_list", "interleaved", "some_empty", "all_empty", "ragged", "short", "random")


def make_lists(rng, R, K, kind):
    """One row: R lists of K u64 keys, each best first with zeros behind its keys, the non-zero keys distinct."""
    if kind == "one_list":                      # list 0 holds the K best keys of the row
        lens = np.array([K] + [int(rng.integers(0, K + 1)) for _ in range(R - 1)])
    elif kind == "interleaved":
        lens = np.full(R, K)
    elif kind == "some_empty":
        lens = np.where(rng.random(R) < 0.5, 0, rng.integers(1, K + 1, R))
        lens[int(rng.integers(0, R))] = K
    elif kind == "all_empty":
        lens = np.zeros(R, dtype=np.int64)
    elif kind == "ragged":
        lens = rng.integers(0, K + 1, R)
    elif kind == "short":                       # fewer than K keys in the whole row
        lens = rng.multinomial(int(rng.integers(0, K)), np.ones(R) / R)
    else:
        lens = rng.integers(K // 2, K + 1, R)
    lens = np.minimum(lens, K).astype(np.int64)
    total = int(lens.sum())
    items = rng.choice(1 << 20, total, replace=False).astype(np.int32)
    vals = (rng.integers(-40, 40, total) / np.float32(8)).astype(np.float32)          # many equal values: the id decides
    keys = np.sort(_pack(vals + np.float32(0), items).view(np.uint64))[::-1]
    out = np.zeros((R, K), dtype=np.uint64)
    if kind == "one_list":
        owner = np.concatenate([np.zeros(K, np.int64), rng.permutation(np.repeat(np.arange(1, R), lens[1:]))])
    elif kind == "interleaved":
        owner = np.arange(total) % R
    else:
        owner = rng.permutation(np.repeat(np.arange(R), lens))
    for r in range(R):
        mine = keys[owner == r]                 # (a subsequence of a descending sequence)
        out[r, :len(mine)] = mine
    return out


def make_rows(rng, R, K):
    kinds = [KINDS[i % len(KINDS)] for i in range(N_ROWS)]
    return np.stack([make_lists(rng, R, K, k) for k in kinds], axis=1), kinds          # [R, rows, K]


def numpy_merge(keys, hist_rows=None):
    """keys u64 [R, rows, K] -> (keys, ids, value bits): the union sorted descending, K of it; empty slots from the row's history, then -1."""
    R, n, K = keys.shape
    flat = np.ascontiguousarray(keys.transpose(1, 0, 2)).reshape(n, R * K)
    top = np.ascontiguousarray(np.sort(flat, axis=1)[:, ::-1][:, :K])
    val, idx = _unpack(top)
    val, idx = val.copy(), idx.copy()
    empty = top == 0
    val[empty], idx[empty] = -np.inf, -1
    if hist_rows is not None:
        for r in range(n):
            nreal = int((~empty[r]).sum())
            fill = np.unique(hist_rows[r])[:K - nreal]
            idx[r, nreal:nreal + len(fill)] = fill
    return top, idx, val.view(np.uint32)


def _hist(dev, rows, by_user):
    from pda_amd import ops
    ip, ix = csr(rows)
    return ops.HistoryCSR(torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev), by_user=by_user)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


# ---- 1: the kernel --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,K", [(1, 55), (2, 64), (2, 65), (3, 100), (5, 257), (8, 1000), (8, 1024), (64, 128)])
def test_merge_kernel_equals_numpy_bit_for_bit(dev, R, K):
    from pda_amd import ops
    rng = np.random.default_rng(100 * R + K)
    keys, kinds = make_rows(rng, R, K)
    assert set(kinds) == set(KINDS)
    kt = torch.from_numpy(keys.view(np.int64)).to(dev)
    # histories: by user id (unsorted user ids, one row with duplicate entries) and by block row
    n_ids = 50
    users = rng.permutation(n_ids)[:N_ROWS].astype(np.int32)
    by_id = [rng.integers(0, 3000, rng.integers(0, 2 * K)).astype(np.int32) for _ in range(n_ids)]
    short_row = kinds.index("short")
    by_id[users[short_row]] = np.concatenate([np.arange(5, 5 + K, dtype=np.int32), np.arange(5, 45, dtype=np.int32)])      # duplicates count once
    by_id[users[kinds.index("all_empty")]] = np.arange(7, 7 + K // 2, dtype=np.int32)                                        # ids, then -1
    by_row = [by_id[u] for u in users]
    ut = torch.from_numpy(users).to(dev)

    rkeys, ridx, rval = numpy_merge(keys, by_row)
    _, ridx0, _ = numpy_merge(keys, None)
    got = ops.deep_merge(kt, want="keys")
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint64), rkeys)
    for h in (_hist(dev, by_id, True), _hist(dev, by_row, False)):
        idx, val = ops.deep_merge(kt, ut, h)
        np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
        np.testing.assert_array_equal(_bits(val), rval)
    idx, val = ops.deep_merge(kt)                      # no history: -1 behind the keys
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx0)
    np.testing.assert_array_equal(_bits(val), rval)
    assert (ridx[short_row] >= 0).all() and (ridx0[short_row] == -1).any()
    # arrays that start off a 16-byte boundary take the same lists through single-word accesses
    off = torch.zeros(kt.numel() + 1, dtype=torch.int64, device=dev)
    off[1:] = kt.reshape(-1)
    got = ops.deep_merge(off[1:].view(R, N_ROWS, K), want="keys")
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint64), rkeys)


# ---- 2: more keys per row than one launch holds ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,K", [(9, 1024), (16, 1000)])
def test_folding_equals_numpy(dev, R, K):
    from pda_amd import ops
    assert R * K > ops.DEEP_MERGE_MAX_KEYS
    rng = np.random.default_rng(R + K)
    keys, kinds = make_rows(rng, R, K)
    rows = [rng.integers(0, 3000, 2 * K).astype(np.int32) for _ in range(N_ROWS)]
    rkeys, ridx, rval = numpy_merge(keys, rows)
    kt = torch.from_numpy(keys.view(np.int64)).to(dev)
    np.testing.assert_array_equal(ops.deep_merge(kt, want="keys").cpu().numpy().view(np.uint64), rkeys)
    idx, val = ops.deep_merge(kt, None, _hist(dev, rows, False))
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    np.testing.assert_array_equal(_bits(val), rval)


# ---- 3: emulated shards in one process ------------------------------------------------------------------------------------------------------
def sharded_lists(dev, Ut, It, pt, ut, K, head, h, R):
    from pda_amd import ops
    from pda_amd.dist import shard_range
    parts = []
    for r in range(R):
        lo, hi = shard_range(It.shape[0], r, R)
        parts.append(ops.deep_shard_keys(Ut, It[lo:hi].contiguous(), ut, K, head, pt[lo:hi].contiguous() if head else None, h, lo))
        assert parts[-1].shape == (ut.numel(), K)
    return ops.deep_merge(torch.stack(parts), ut, h)


@pytest.mark.parametrize("d,K,R,bf16", [(64, 100, 2, False), (128, 1000, 8, False), (32, 55, 3, False), (256, 1024, 8, False), (128, 257, 3, False),
                                        (64, 300, 3, True)])
def test_emulated_shards_equal_the_oracle_and_the_one_gpu_call(dev, d, K, R, bf16):
    from pda_amd import ops
    from pda_amd.dist import shard_range
    rng = np.random.default_rng(1000 * d + K + R)
    nU, nI = 300, 5000
    U, I, pop, hist = make_case(rng, nU, nI, d)
    if bf16:
        U, I = torch.from_numpy(U).bfloat16().float().numpy(), torch.from_numpy(I).bfloat16().float().numpy()
    users = rng.choice(nU, 173, replace=False).astype(np.int32)
    blk = [hist[u] for u in users]
    if R == 8:
        assert shard_range(nI, 0, R)[1] < K                      # 625-item shards under a list of 1 000
    Ut, It, pt, ut = (torch.from_numpy(x).to(dev) for x in (U, I, pop, users))
    if bf16:
        Ut, It = Ut.bfloat16(), It.bfloat16()
    by_user = (K % 2 == 0)
    h = _hist(dev, hist if by_user else blk, by_user)
    ridx, rval = c_oracle.score_topk(U, I, users, K, 0, None, *csr(blk), order=1)
    for head in (0, 1):
        idx, val = sharded_lists(dev, Ut, It, pt, ut, K, head, h, R)
        widx, wval = ops.recommend_topk_deep(Ut, It, ut, K, head, pt if head else None, h)
        assert torch.equal(idx, widx), (head, int((idx != widx).sum()))
        np.testing.assert_array_equal(_bits(val), _bits(wval))   # (per-pair values do not depend on the shard: the popularity head too)
        if head == 0:
            np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
            np.testing.assert_array_equal(val.cpu().numpy(), rval)


# ---- 4: short rows across shards ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [257, 600])
def test_short_rows_across_shards_end_in_their_history_by_id(dev, K):
    from pda_amd import ops
    rng = np.random.default_rng(9)
    nU, nI, d, R = 33, 600, 64, 3
    U, I, pop, _ = make_case(rng, nU, nI, d, max_hist=0)
    hist = [rng.permutation(nI)[:rng.integers(nI - 250, nI + 1)].astype(np.int32) for _ in range(nU)]     # 0 .. 250 unlisted items
    hist[0] = np.arange(nI, dtype=np.int32)                    # everything listed
    hist[1] = np.concatenate([hist[1], hist[1][:40]])          # duplicates count once
    users = np.arange(nU, dtype=np.int32)
    Ut, It, pt, ut = (torch.from_numpy(x).to(dev) for x in (U, I, pop, users))
    h = _hist(dev, hist, True)
    ridx, rval = c_oracle.score_topk(U, I, users, K, 0, None, *csr(hist), order=1)
    assert np.isneginf(rval).any(axis=1).sum() >= 10
    for head in (0, 1):
        idx, val = sharded_lists(dev, Ut, It, pt, ut, K, head, h, R)
        widx, wval = ops.recommend_topk_deep(Ut, It, ut, K, head, pt if head else None, h)
        assert torch.equal(idx, widx)
        np.testing.assert_array_equal(_bits(val), _bits(wval))
        if head == 0:
            np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
            np.testing.assert_array_equal(val.cpu().numpy(), rval)
    np.testing.assert_array_equal(idx[0].cpu().numpy(), np.arange(K))        # the fully listed user: its history by id
    assert torch.isneginf(val[0]).all()


# ---- 5: the model wrapper -------------------------------------------------------------------------------------------------------------------
def test_model_with_a_shard_returns_the_unsharded_lists(dev):
    from pda_amd import ops
    from pda_amd import train_new_api as t
    from pda_amd.dist import ItemShardedTopK
    from pda_amd.parse import parse_args
    rng = np.random.default_rng(5)
    cfg = {"n_users": 60, "n_items": 900}
    args = parse_args(["--topk_max", "100", "--train", "s_condition", "--embed_size", "64"])
    plain = t.DatasetApi_Model(args, cfg, 4, None, device=dev)
    U, I = plain.Recommender.score_tables()
    with torch.no_grad():
        U.copy_(torch.from_numpy((rng.standard_normal(tuple(U.shape)) * 0.1).astype(np.float32)).to(U.dtype))
        I.copy_(torch.from_numpy((rng.standard_normal(tuple(I.shape)) * 0.1).astype(np.float32)).to(I.dtype))
    shard = ItemShardedTopK(U, I, 0, None, rank=0, world=1)
    model = t.DatasetApi_Model(args, cfg, 4, None, device=dev, topk_shard=shard)
    assert model.topk_max == 100
    hist = [rng.integers(0, cfg["n_items"], rng.integers(0, 30)).astype(np.int32) for _ in range(cfg["n_users"])]
    h = _hist(dev, hist, True)
    users = torch.from_numpy(rng.permutation(cfg["n_users"])[:45].astype(np.int32)).to(dev)
    pop = torch.from_numpy((rng.uniform(0, 1, cfg["n_items"]) ** 0.22).astype(np.float32)).to(dev)
    for rec_type, p in (("main_branch", None), ("condition", pop)):
        idx, val = model.recommend_device(users, None, rec_type, p, h)
        ridx, rval = plain.recommend_device(users, None, rec_type, p, h)
        assert idx.shape == (45, 100) and torch.equal(idx, ridx)
        np.testing.assert_array_equal(_bits(val), _bits(rval))
    assert shard.n_collectives == 0
