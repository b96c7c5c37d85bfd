"""CPU suite for deep lists on item shards (pda_deep_merge, ops.deep_merge / deep_shard_keys, dist.ItemShardedTopK at K > 54): the entry
point's argument checks (all before any HIP call), the capability flag of the model wrapper, the orchestration under gloo with doubles that
answer through the CPU oracle (ids and values equal the unsharded oracle exactly), and the rule that cuts the exchange into user chunks."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import c_oracle
from test_dist_gloo import _free_port, _pack, _unpack, score_double

ERR_ARG, ERR_UNSUPPORTED = -1, -2


# ---- 1: the entry point --------------------------------------------------------------------------------------------------------------------
def test_merge_argument_checks_without_gpu():
    from pda_amd import _lib
    lib = _lib.load()
    assert lib.pda_deep_merge.argtypes == _lib.DEEP_SIGNATURES["pda_deep_merge"][1]
    assert _lib.DEEP_MERGE_MAX_KEYS == 8192
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pda_hip_deep.h")).read()
    assert "#define PDA_DEEP_MERGE_MAX_KEYS 8192" in text
    keep = C.create_string_buffer(4096)
    b, null = C.c_void_p(C.addressof(keep)), C.c_void_p(None)

    def call(keys=b, R=2, nu=4, K=100, out_keys=b, out_idx=b, out_val=b, users=b, indptr=null, indices=null, mode=0):
        return lib.pda_deep_merge(keys, R, nu, K, out_keys, out_idx, out_val, users, indptr, indices, mode, null)

    assert call(keys=null) == ERR_ARG
    assert call(R=0) == ERR_ARG and call(R=-1) == ERR_ARG
    assert call(K=0) == ERR_ARG and call(K=1025) == ERR_ARG
    assert call(nu=0) == ERR_ARG
    assert call(out_keys=null, out_idx=null) == ERR_ARG                       # (values alone are no output)
    assert call(indptr=b, indices=b, mode=1, users=null) == ERR_ARG           # a history by user id without the user ids
    assert call(indptr=b, indices=null) == ERR_ARG
    assert call(indptr=b, indices=b, mode=2) == ERR_ARG
    assert call(R=9, K=1024) == ERR_UNSUPPORTED                               # 9 216 keys per row
    assert call(R=8193, K=1) == ERR_UNSUPPORTED
    assert call(R=149, K=55) == ERR_UNSUPPORTED
    del keep


def test_ops_refuse_bad_arguments_before_the_library():
    from pda_amd import ops
    with pytest.raises((ValueError, TypeError)):
        ops.deep_merge(torch.zeros((2, 4, 100), dtype=torch.int64))           # host memory
    with pytest.raises((ValueError, TypeError)):
        ops.deep_shard_keys(torch.zeros((4, 64)), torch.zeros((300, 64)), torch.zeros(4, dtype=torch.int32), 100)
    assert ops.DEEP_MERGE_MAX_KEYS == 8192


# ---- doubles: one shard's list and the merge, through the oracle / numpy ------------------------------------------------------------------
def deep_score_double(U, I_shard, users, K, head, pop_shard, hist, item_offset, n_splits):
    """test_dist_gloo.score_double on min(K, shard) columns: listed items (value -inf) are empty slots, zeros behind the keys."""
    kc = min(K, I_shard.shape[0])
    keys = score_double(U, I_shard, users, kc, head, pop_shard, hist, item_offset, n_splits)
    val, _ = _unpack(keys.numpy())
    keys = torch.where(torch.from_numpy(np.isneginf(val)), torch.zeros_like(keys), keys)
    out = torch.zeros((1, users.numel(), K), dtype=torch.int64)
    out[:, :, :kc] = keys
    return out


def deep_merge_double(keys, users, hist, want="idx_val"):
    """pda_deep_merge's contract in numpy: the K largest keys of the union; empty slots from the user's history row, then -1."""
    R, Bu, K = keys.shape
    flat = np.ascontiguousarray(keys.numpy().view(np.uint64).transpose(1, 0, 2)).reshape(Bu, R * K)
    top = np.ascontiguousarray(np.sort(flat, axis=1)[:, ::-1][:, :K])
    if want == "keys":
        return torch.from_numpy(top.view(np.int64).copy())
    val, idx = _unpack(top)
    val, idx = val.copy(), idx.copy()
    empty = top == 0
    val[empty], idx[empty] = -np.inf, -1
    if hist is not None:
        ip, ix = hist
        for r, u in enumerate(users.numpy()):
            n = int((~empty[r]).sum())
            fill = np.unique(ix[ip[u]:ip[u + 1]])[:K - n]
            idx[r, n:n + len(fill)] = fill
    return torch.from_numpy(idx), torch.from_numpy(val)


def _case(seed=4):
    rng = np.random.default_rng(seed)
    nU, nI, d = 60, 777, 32
    U = (rng.standard_normal((nU, d)) * 0.1).astype(np.float32)
    I = (rng.standard_normal((nI, d)) * 0.1).astype(np.float32)
    pop = (rng.uniform(0, 1, nI) ** 0.22).astype(np.float32)
    rows = [np.sort(rng.integers(0, nI, rng.integers(0, 25))).astype(np.int32) for _ in range(nU)]
    ip = np.zeros(nU + 1, np.int64)
    ip[1:] = np.cumsum([len(r) for r in rows])
    return U, I, pop, rows, ip, np.concatenate(rows)


def _oracle(U, I, pop, rows, users, K, head):
    u = users.numpy()
    bip = np.zeros(len(u) + 1, np.int64)
    bip[1:] = np.cumsum([len(rows[x]) for x in u])
    bix = np.concatenate([rows[x] for x in u])
    return c_oracle.score_topk(U, I, u, K, head, pop if head else None, bip, bix, order=1)


# ---- 2: the capability flag ---------------------------------------------------------------------------------------------------------------
def test_a_shard_with_deep_lists_passes_the_model_wrapper():
    from pda_amd import train_new_api as t
    from pda_amd.dist import ItemShardedTopK
    from pda_amd.parse import parse_args
    U, I, pop, rows, ip, ix = _case()
    ev = ItemShardedTopK(torch.from_numpy(U), torch.from_numpy(I), 0, torch.from_numpy(pop), rank=0, world=1,
                         score_fn=deep_score_double, merge_fn=deep_merge_double)
    assert ItemShardedTopK.deep_lists is True
    assert t.check_topk_max(parse_args(["--topk_max", "100"]), topk_shard=ev) == 100
    assert t.check_topk_max(parse_args(["--topk_max", "1024"]), topk_shard=ev) == 1024
    with pytest.raises(NotImplementedError, match="item shards"):
        t.check_topk_max(parse_args(["--topk_max", "100"]), topk_shard=object())
    with pytest.raises(NotImplementedError, match="bias head"):
        t.check_topk_max(parse_args(["--topk_max", "100", "--train", "temp_pop"]), topk_shard=ev)
    # one rank, doubles: the deep path of the class is the oracle's list
    users = torch.arange(0, 60, dtype=torch.int32)
    for K in (100, 300):
        idx, val = ev.topk(users, K, 1, (ip, ix))
        ridx, rval = _oracle(U, I, pop, rows, users, K, 1)
        assert np.array_equal(idx.numpy(), ridx) and np.array_equal(val.numpy(), rval)
    assert ev.n_collectives == 0
    assert not ev._seed_applies(100, 1) and not ev._hot_applies(100, 1, None, users, True)


# ---- 3: two and three ranks under gloo ----------------------------------------------------------------------------------------------------
def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pda_amd.dist import ItemShardedTopK
    U, I, pop, rows, ip, ix = _case()                                   # the same data on every rank (replicated inputs)
    ev = ItemShardedTopK.from_full_tables(torch.from_numpy(U), torch.from_numpy(I), torch.from_numpy(pop), rank, world,
                                          score_fn=deep_score_double, merge_fn=deep_merge_double)
    blocks = [torch.arange(0, 30, dtype=torch.int32), torch.arange(30, 60, dtype=torch.int32)]
    ragged = torch.arange(7, 35, dtype=torch.int32)                     # 28 users: three ranks cannot split them evenly
    out, hist = [], (ip, ix)
    for K in (100, 300):
        for head in (0, 1):
            refs = [_oracle(U, I, pop, rows, b, K, head) for b in blocks]
            n0 = ev.n_collectives
            for sharded in (False, True):
                for users, (ridx, rval), (idx, val) in zip(blocks, refs, ev.topk_blocks(blocks, K, head, hist, sharded=sharded)):
                    lo, hi = ev.user_slice(users.numel()) if sharded else (0, users.numel())
                    out.append(bool(idx.shape == (hi - lo, K) and np.array_equal(idx.numpy(), ridx[lo:hi])
                                    and np.array_equal(val.numpy(), rval[lo:hi])))
            out.append(ev.n_collectives - n0 == 4)                      # one collective per block: these sizes fit one chunk
            n0 = ev.n_collectives
            idx, val = ev.topk(blocks[1], K, head, hist)
            out.append(bool(np.array_equal(idx.numpy(), refs[1][0]) and np.array_equal(val.numpy(), refs[1][1])))
            lo, hi = ev.user_slice(30)
            idx, val = ev.topk_sharded(blocks[0], K, head, hist)
            out.append(bool(np.array_equal(idx.numpy(), refs[0][0][lo:hi]) and np.array_equal(val.numpy(), refs[0][1][lo:hi])))
            ridx, rval = _oracle(U, I, pop, rows, ragged, K, head)
            idx, val = ev.topk_sharded(ragged, K, head, hist)
            if 28 % world == 0:
                lo, hi = ev.user_slice(28)
            else:
                per = -(-28 // world)
                lo, hi = min(rank * per, 28), min(rank * per + per, 28)
            out.append(bool(np.array_equal(idx.numpy(), ridx[lo:hi]) and np.array_equal(val.numpy(), rval[lo:hi])))
            out.append(ev.n_collectives - n0 == 3)
    q.put((rank, out, ev.item_offset, ev.I_shard.shape[0]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_deep_lists_on_item_shards_gloo(world):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    assert [r[0] for r in res] == list(range(world))
    assert all(all(r[1]) for r in res), res
    assert sum(r[3] for r in res) == 777
    if world == 3:
        assert all(r[3] < 300 for r in res)                               # short shards: 288, 288 and 201 items under K = 300


# ---- 4: the chunk rule --------------------------------------------------------------------------------------------------------------------
def test_exchange_chunks_depend_on_users_k_and_world_only(monkeypatch):
    from pda_amd import dist as pd
    from pda_amd import ops
    assert list(inspect.signature(pd.deep_exchange_chunk).parameters) == ["n_users", "K", "world"]
    budget = ops.DEEP_WORKSPACE_BUDGET
    for world in (1, 2, 3, 8, 16):
        for K in (55, 100, 1000, 1024):
            for nu in (1, 7, 173, 65536, 262144, 1 << 22):
                c = pd.deep_exchange_chunk(nu, K, world)
                assert c % world == 0 and c >= world                      # whole users per rank, at least one
                assert c <= -(-nu // world) * world
                assert world * c * K * 8 <= budget                        # the gathered [R, chunk, K] keys
                if c < nu:                                                # ... and no smaller than it has to be
                    assert world * (c + world) * K * 8 > budget
    assert pd.deep_exchange_chunk(262144, 1000, 8) < 262144 // 8          # config 3 on eight ranks: 2.1 GB per shard goes in chunks

    # the collectives of a block are the same whatever this rank's shard holds: 1 row or 10^6
    monkeypatch.setattr(ops, "DEEP_WORKSPACE_BUDGET", 2 * 2 * 100 * 8 * 5)    # five users per rank and chunk at K = 100 on two ranks
    seen = []

    def gather(keys, world, group=None):
        seen[-1].append(("gather", tuple(keys.shape)))
        return torch.stack([keys] * world)

    def exchange(keys, world, group=None):
        seen[-1].append(("exchange", tuple(keys.shape)))
        return keys.view(world, keys.shape[0] // world, keys.shape[1]).clone()

    monkeypatch.setattr(pd, "_all_gather_keys", gather)
    monkeypatch.setattr(pd, "_exchange_user_slices", exchange)
    merged = []

    def merge(keys, users, hist, want="idx_val"):
        merged.append((tuple(keys.shape), users.numel()))
        return torch.zeros((users.numel(), keys.shape[2]), dtype=torch.int32), torch.zeros((users.numel(), keys.shape[2]))

    users, keys = torch.arange(46, dtype=torch.int32), torch.zeros((46, 100), dtype=torch.int64)
    for n_local in (1, 10 ** 6):
        ev = pd.ItemShardedTopK(torch.zeros((50, 8)), torch.zeros((n_local, 8)), 0, None, rank=1, world=2, score_fn=deep_score_double, merge_fn=merge)
        seen.append([])
        idx, val = ev._finish_deep(keys, users, None, False)
        assert idx.shape == (46, 100) and ev.n_collectives == 5            # 10 + 10 + 10 + 10 + 6 users
        idx, val = ev._finish_deep(keys, users, None, True)
        assert idx.shape == (23, 100) and ev.n_collectives == 10           # 5 + 5 + 5 + 5 + 3 rows of each rank's 23
    assert seen[0] == seen[1] and len(seen[0]) == 10
    assert seen[0][:5] == [("gather", (10, 100))] * 4 + [("gather", (6, 100))]
    assert seen[0][5:] == [("exchange", (10, 100))] * 4 + [("exchange", (6, 100))]
    assert all(m[0][0] == 2 for m in merged)
