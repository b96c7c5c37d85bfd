"""The criterion behind the huge geometry's test-free tail (pda_amd/csrc/pda_v5_sweep.h), restated in numpy and checked against
oracle/pda_oracle.py on the CPU: behind the decided tile of a 1 024-user workgroup no item appears in any oracle list of its rows."""
import numpy as np
import pytest

from decided_tail_cases import decided_tile, lowered, oracle_lists, padded_norm, plant, steep_case, suffix_bounds

K = 50


def decided_tiles_of_block(U, I, pop, users, rows, simple):
    """per 1 024-user workgroup: (the decided tile on the FINAL K-th values -- the earliest a sweep can ever decide --, the oracle's lists as
    visiting positions)"""
    order, sufA, sufB = suffix_bounds(I, pop)
    pos_of = np.empty(len(order), np.int64)
    pos_of[order] = np.arange(len(order))
    idx, val = oracle_lists(U, I, pop, users, rows, K)
    tau = lowered(val[:, K - 1].astype(np.float32))
    nu = padded_norm(U, users)
    out = []
    for w0 in range(0, len(users), 1024):
        sl = slice(w0, min(w0 + 1024, len(users)))
        if simple:      # one criterion per workgroup: largest norm, lowest threshold (what the kernel does)
            t = decided_tile(sufA, sufB, nu[sl].max(), tau[sl].min())
        else:           # per row, the last row decides
            t = max(decided_tile(sufA, sufB, a, b) for a, b in zip(nu[sl], tau[sl]))
        out.append((t, pos_of[idx[sl]]))
    return out, len(sufA)


@pytest.mark.parametrize("simple", [True, False])
@pytest.mark.parametrize("d,ratio,seed", [(64, 0.998, 1), (128, 0.9995, 2), (128, 0.99995, 3)])
def test_nothing_behind_the_decided_tile_ranks_random(d, ratio, seed, simple):
    rng = np.random.default_rng(seed)
    U, I, pop, rows = steep_case(rng, 1500, 6000, d, ratio=ratio)
    users = np.arange(1500, dtype=np.int32)
    blocks, n_tiles = decided_tiles_of_block(U, I, pop, users, rows, simple)
    for t, pos in blocks:
        assert pos.max() < 64 * t, (t, int(pos.max()))
    if ratio <= 0.9995:                                   # a popularity this steep decides inside the catalogue
        assert all(t < n_tiles for t, _ in blocks)


def test_per_row_criterion_is_at_most_the_workgroups():
    rng = np.random.default_rng(4)
    U, I, pop, rows = steep_case(rng, 1024, 6000, 128, ratio=0.9995)
    users = np.arange(1024, dtype=np.int32)
    (ts, _), = decided_tiles_of_block(U, I, pop, users, rows, True)[0]
    (tr, _), = decided_tiles_of_block(U, I, pop, users, rows, False)[0]
    assert tr <= ts


@pytest.mark.parametrize("simple", [True, False])
@pytest.mark.parametrize("where", ["first_half", "second_half", "two_items"])
def test_planted_item_keeps_the_bound_up(where, simple):
    """A planted item in the last fifth of the visiting order whose norm lifts its head into the lists of the users aligned with it: the
    decided tile of every workgroup lies BEHIND its tile, and the oracle's lists of the aligned users contain it."""
    rng = np.random.default_rng(11)
    nU, nI, d = 1500, 8000, 128
    U, I, pop, rows = steep_case(rng, nU, nI, d, ratio=0.999, hist=False)
    item = 64 * 106 + (5 if where != "second_half" else 40)          # position 6 789 / 6 824 of 8 000
    aligned = np.arange(0, nU, 7, dtype=np.int32)
    plant(U, I, pop, item, aligned)
    if where == "two_items":
        plant(U, I, pop, item - 64, aligned[:0])                       # (no further users: the direction is another one)
    users = np.arange(nU, dtype=np.int32)
    idx, _ = oracle_lists(U, I, pop, users, None, K)
    assert all(item in idx[u] for u in aligned), "the planted item must rank for the users aligned with it"
    blocks, n_tiles = decided_tiles_of_block(U, I, pop, users, None, simple)
    for t, pos in blocks:
        assert t == item // 64 + 1, (t, item // 64)                    # right behind it: the rest of the catalogue cannot rank
        assert pos.max() < 64 * t


def test_equal_popularities_never_decide():
    rng = np.random.default_rng(5)
    U, I, pop, rows = steep_case(rng, 1024, 4000, 64)
    pop[:] = 0.5
    users = np.arange(1024, dtype=np.int32)
    blocks, n_tiles = decided_tiles_of_block(U, I, pop, users, rows, True)
    assert blocks[0][0] == n_tiles


def test_short_list_never_decides():
    order, sufA, sufB = suffix_bounds(np.ones((128, 64), np.float32), np.linspace(1, 0.1, 128).astype(np.float32))
    assert decided_tile(sufA, sufB, 1.0, -np.inf) == len(sufA)
