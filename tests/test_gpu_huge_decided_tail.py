"""The huge geometry's test-free tail (pda_amd/csrc/pda_v5_sweep.h: the decided half-tile; Loop6Free::run): packed keys bit for bit against
the exact kernel (impl="v1"), and -- through stats["huge_free_halftiles"] -- each case did what its name says.  The geometry is forced the
way tests/test_gpu_score_topk.py's "k4huge" path forces it; the identity word the sweep kernel writes is asserted on every call."""
import numpy as np
import pytest
import torch

from decided_tail_cases import csr, oracle_lists, plant, steep_case

pytestmark = pytest.mark.gpu
K = 50


@pytest.fixture(autouse=True)
def huge(monkeypatch):
    monkeypatch.setenv("PDA_SCORE_IMPL", "v2")
    monkeypatch.setenv("PDA_CHECK_SWEEP_ERRORS", "1")
    monkeypatch.setenv("PDA_SCORE_PRUNE", "order")
    monkeypatch.setenv("PDA_SCORE_LISTS", "huge")
    monkeypatch.setenv("PDA_SCORE_KERNEL", "v4")


def user_tile(d):
    return 512 if d == 256 else 1024


def sweep_halftiles(n_users, n_items, d, n_splits=1, warm=4):
    """32-item half-tiles of the sweep, summed over the workgroups: everything behind the warm-up's tiles (one shared warm-up of `warm`
    tiles of the whole order when the catalogue is split; warm = 0: a sweep from empty lists)"""
    return 2 * (-(-n_users // user_tile(d))) * (-(-n_items // 64) - warm)


def to_dev(dev, U, I, pop, rows, bf16=False):
    from pda_amd import ops
    Ut, It, pt = torch.from_numpy(U).to(dev), torch.from_numpy(I).to(dev), torch.from_numpy(pop).to(dev)
    h = None
    if rows is not None:
        ip, ix = csr(rows)
        h = ops.HistoryCSR(torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev), by_user=True)
    if bf16:
        return (Ut.bfloat16(), It.bfloat16(), pt, h), (Ut, It, pt, h)
    return (Ut, It, pt, h), (Ut, It, pt, h)


def assert_huge(st, d):
    from pda_amd import ops
    assert int(st["error"][0]) == 0
    ident = ops.kernel_identity(st["kernel_id"][0])
    assert ident["generation"] == 4 and ident["geometry"] == "huge" and ident["d"] == d, ident


def run_both(dev, U, I, pop, rows, users, n_splits=1, bf16=False):
    """-> (merged keys of the huge geometry, merged keys of the exact kernel, half-tiles run test-free)"""
    from pda_amd import ops
    (Ut, It, pt, h), (Uf, If, pf, hf) = to_dev(dev, U, I, pop, rows, bf16)
    ut = torch.from_numpy(np.asarray(users, dtype=np.int32)).to(dev)
    st = {}
    got = ops.score_topk_keys(Ut, It, ut, K, ops.HEAD_POP, pt, h, 0, n_splits, impl="v2", prune="order", stats=st)
    assert got.shape[0] == n_splits
    got = ops.topk_merge(got, want="keys")
    ref = ops.topk_merge(ops.score_topk_keys(Uf, If, ut, K, ops.HEAD_POP, pf, hf, 0, impl="v1"), want="keys")
    torch.cuda.synchronize()
    assert_huge(st, U.shape[1])
    free = int(st["huge_free_halftiles"][0])
    print("huge_free_halftiles %d of %d" % (free, sweep_halftiles(len(users), I.shape[0], U.shape[1])))
    return got, ref, free


def bf16_exact(x):
    return torch.from_numpy(x).bfloat16().float().numpy()


# (a), (i): popularity falling steeply -- the tail is entered right behind the warm-up; every instance of the loop, with and without a mask
@pytest.mark.parametrize("hist", [True, False])
@pytest.mark.parametrize("d,bf16", [(64, False), (128, False), (256, True)])
def test_steep_popularity_runs_test_free_behind_the_warm_up(dev, d, bf16, hist):
    rng = np.random.default_rng(10 + d)
    nU, nI = 2500, 8000
    U, I, pop, rows = steep_case(rng, nU, nI, d, ratio=0.998, hist=hist)
    if bf16:
        U, I = bf16_exact(U), bf16_exact(I)
    got, ref, free = run_both(dev, U, I, pop, rows, np.arange(nU), bf16=bf16)
    assert torch.equal(got, ref), int((got != ref).sum())
    total = sweep_halftiles(nU, nI, d)
    assert 0.85 * total <= free <= total, (free, total)


# (b) all popularities equal: the bound never falls below a threshold
@pytest.mark.parametrize("d", [64, 128])
def test_equal_popularities_stay_tested(dev, d):
    rng = np.random.default_rng(20 + d)
    U, I, pop, rows = steep_case(rng, 2000, 5000, d)
    pop[:] = 0.5
    got, ref, free = run_both(dev, U, I, pop, rows, np.arange(2000))
    assert torch.equal(got, ref), int((got != ref).sum())
    assert free == 0


# (c) a planted item in the last fifth of the visiting order whose head enters the lists of the users aligned with it
@pytest.mark.parametrize("where", ["first_half", "second_half", "two_items"])
def test_planted_item_is_found_and_nothing_goes_test_free_in_front_of_it(dev, where):
    rng = np.random.default_rng(30)
    nU, nI, d = 2500, 8000, 128
    U, I, pop, rows = steep_case(rng, nU, nI, d, ratio=0.999, hist=False)
    item = 64 * 106 + (5 if where != "second_half" else 40)
    aligned = np.arange(0, nU, 7, dtype=np.int32)
    plant(U, I, pop, item, aligned)
    if where == "two_items":
        plant(U, I, pop, item - 64, aligned[:0])
    idx, _ = oracle_lists(U, I, pop, aligned, None, K)                   # (oracle/pda_oracle.py alone: the case is what it claims to be)
    assert all(item in row for row in idx)
    got, ref, free = run_both(dev, U, I, pop, None, np.arange(nU))
    assert torch.equal(got, ref), int((got != ref).sum())
    from pda_amd import ops
    ids, _ = ops.unpack_keys(got)
    assert all(item in ids[u] for u in aligned)
    # the planted item keeps the suffix bound above every threshold up to its own tile: test-free from the tile behind it, in every workgroup
    behind = 2 * (-(-nU // 1024)) * (-(-nI // 64) - (item // 64 + 1))
    assert 0 < free <= behind, (free, behind)


# (d) one user row scaled x 50: only its workgroup stays tested longer
def test_one_large_user_keeps_only_its_workgroup_tested(dev):
    rng = np.random.default_rng(40)
    nU, nI, d = 3000, 12000, 128
    U, I, pop, rows = steep_case(rng, nU, nI, d, ratio=0.9995)
    users = np.arange(nU)
    got, ref, plain = run_both(dev, U, I, pop, rows, users)
    assert torch.equal(got, ref)
    _, _, plain_rest = run_both(dev, U, I, pop, rows, users[1024:])
    U[17] *= 50.0
    got, ref, scaled = run_both(dev, U, I, pop, rows, users)
    assert torch.equal(got, ref), int((got != ref).sum())
    got, ref, scaled_rest = run_both(dev, U, I, pop, rows, users[1024:])
    assert torch.equal(got, ref)
    per_wg = sweep_halftiles(1024, nI, d)
    assert scaled_rest == plain_rest                                     # workgroups 1 and 2 do not see row 17
    assert 0 < scaled - scaled_rest < plain - plain_rest <= per_wg, (scaled, scaled_rest, plain, plain_rest)


# (e) a ragged block and a block smaller than one workgroup
@pytest.mark.parametrize("nU", [1500, 300, 1025])
def test_ragged_and_small_blocks(dev, nU):
    rng = np.random.default_rng(50 + nU)
    U, I, pop, rows = steep_case(rng, 1600, 6000, 128, ratio=0.998)
    users = rng.permutation(1600)[:nU]
    got, ref, free = run_both(dev, U, I, pop, rows, users)
    assert torch.equal(got, ref), int((got != ref).sum())
    total = sweep_halftiles(nU, 6000, 128)
    assert 0.8 * total <= free <= total, (free, total)


# (f) item splits: the shared warm-up, splits that start from empty lists and a seed
@pytest.mark.parametrize("n_splits", [2, 3, 8])
@pytest.mark.parametrize("d", [64, 128])
def test_item_splits(dev, n_splits, d):
    rng = np.random.default_rng(60 + n_splits + d)
    nU, nI = 2000, 20000
    U, I, pop, rows = steep_case(rng, nU, nI, d, ratio=0.9995)
    got, ref, free = run_both(dev, U, I, pop, rows, np.arange(nU), n_splits=n_splits)
    assert torch.equal(got, ref), int((got != ref).sum())
    total = sweep_halftiles(nU, nI, d)
    # (bound 2.3 x pop against a K-th value near pop[50]: decided some 1 700 items down the order, 9 % of this catalogue)
    assert 0.7 * total <= free <= total, (free, total)


# (g) ops.sweep_from_seed (phase 4): empty lists, a row's threshold is its seed until its list fills
@pytest.mark.parametrize("n_splits", [1, 3])
@pytest.mark.parametrize("seeded", ["finite", "minus_inf", "mixed"])
def test_sweep_from_seed(dev, seeded, n_splits):
    from pda_amd import ops
    rng = np.random.default_rng(70)
    nU, nI, d = 2000, 10000, 128
    U, I, pop, rows = steep_case(rng, nU, nI, d, ratio=0.999)
    (Ut, It, pt, h), _ = to_dev(dev, U, I, pop, rows)
    ut = torch.arange(nU, dtype=torch.int32, device=dev)
    refk = ops.topk_merge(ops.score_topk_keys(Ut, It, ut, K, ops.HEAD_POP, pt, h, 0, impl="v1"), want="keys")
    _, val = ops.topk_merge(ops.score_topk_keys(Ut, It, ut, K, ops.HEAD_POP, pt, h, 0, impl="v1"), ut, h)
    seed = val[:, K - 1].clone().float()                                 # the exact K-th value: a lower bound that keeps the whole list
    if seeded == "minus_inf":
        seed[:] = float("-inf")
    elif seeded == "mixed":
        seed[::3] = float("-inf")
    st = {}
    got = ops.sweep_from_seed(Ut, It, ut, K, ops.HEAD_POP, pt, h, 0, seed, n_splits=n_splits, prune="order", stats=st)
    got = ops.topk_merge(got, want="keys")
    torch.cuda.synchronize()
    assert_huge(st, d)
    assert torch.equal(got, refk), int((got != refk).sum())
    free, total = int(st["huge_free_halftiles"][0]), sweep_halftiles(nU, nI, d, warm=0)
    print("huge_free_halftiles %d of %d" % (free, total))
    assert 0 < free <= total
    if seeded == "finite":                                               # every threshold is final from the first entry on
        assert free >= 0.8 * total, (free, total)


# (h) a row with fewer than K rankable items: its threshold stays -inf, its workgroup never goes test-free
def test_a_row_that_never_fills_keeps_its_workgroup_tested(dev):
    rng = np.random.default_rng(80)
    nU, nI, d = 1500, 6000, 128
    U, I, pop, rows = steep_case(rng, nU, nI, d, ratio=0.998)
    keep = rng.permutation(nI)[:30]
    rows[5] = np.setdiff1d(np.arange(nI, dtype=np.int32), keep).astype(np.int32)      # user 5 may rank 30 items
    got, ref, free = run_both(dev, U, I, pop, rows, np.arange(1024))
    assert torch.equal(got, ref), int((got != ref).sum())
    assert int((got[5] != 0).sum()) == 30
    assert free == 0
    got, ref, free = run_both(dev, U, I, pop, rows, np.arange(nU))       # the second workgroup is an ordinary one
    assert torch.equal(got, ref), int((got != ref).sum())
    per_wg = sweep_halftiles(1024, nI, d)
    assert 0.85 * per_wg <= free <= per_wg, (free, per_wg)
