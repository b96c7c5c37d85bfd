"""The exits of the huge geometry's asm loop (pda_v5_sweep.h): a flag sends all four waves of a workgroup out of the loop, the two
half-tiles behind it are scored again in ONE pass over the user blocks (the fused extract: user fragments loaded once for both, in
batches whose loads are in flight together), the candidates are rescored exactly, the loop is entered again.

Packed keys bit for bit against the exact kernel (impl="v1", merged) with stats["error"] == 0; every case asserts that exits happened
(more than one loop entry per wave; where the sweep is one or two half-tiles long an exit is never followed by an entry, and the rescored
pairs are the witness: at least one per list entry of the exact kernel that comes from behind the warm-up) and that rows were appended to.  The shapes are small, so the library's plan would not pick the huge
geometry: it is forced the way tests/test_gpu_score_topk.py -k k4huge forces it, and the identity word the sweep kernel writes is
asserted on every call."""
import numpy as np
import pytest
import torch

from test_gpu_dense_call_passes import bf16_exact, case, hist_of

pytestmark = pytest.mark.gpu
K = 50
F = np.float32


@pytest.fixture(autouse=True)
def forced_huge(monkeypatch):
    monkeypatch.setenv("PDA_CHECK_SWEEP_ERRORS", "1")
    for k in ("PDA_HUGE_SPLITS", "PDA_SCORE_IMPL", "PDA_SCORE_PRUNE", "PDA_WARM_PER_SPLIT", "PDA_WARM_MASK_TABLE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PDA_SCORE_LISTS", "huge")
    monkeypatch.setenv("PDA_SCORE_KERNEL", "v4")


def run_case(dev, U, I, pop, rows, users, by_user, bf16):
    """-> (merged keys of the huge geometry, merged keys of the exact kernel, stats, loop entries per wave)"""
    from pda_amd import ops
    nU, d = len(users), U.shape[1]
    Uf, If, pt = torch.from_numpy(U).to(dev), torch.from_numpy(I).to(dev), torch.from_numpy(pop).to(dev)
    Ut, It = (Uf.bfloat16(), If.bfloat16()) if bf16 else (Uf, If)
    ut = torch.from_numpy(np.asarray(users, dtype=np.int32)).to(dev)
    h = hist_of(dev, rows, users, by_user)
    st = {}
    got = ops.score_topk_keys(Ut, It, ut, K, ops.HEAD_POP, pt, h, 0, 0, impl="v2", prune="order", stats=st)
    ref = ops.topk_merge(ops.score_topk_keys(Uf, If, ut, K, ops.HEAD_POP, pt, h, 0, impl="v1"), want="keys")
    torch.cuda.synchronize()
    assert int(st["error"][0]) == 0
    ident = ops.kernel_identity(st["kernel_id"][0])
    assert ident["generation"] == 4 and ident["geometry"] == "huge" and ident["d"] == d and ident["bf16"] == bf16, ident
    waves = 4 * -(-nU // (512 if d == 256 else 1024)) * got.shape[0]
    return ops.topk_merge(got, want="keys"), ref, st, float(st["huge_entries"][0]) / waves


def short_rows(rng, rows, pop, nU):
    """some rows keep only 0 .. 51 unmasked items (half of them among the warm-up's 256, half behind it)"""
    nI = len(pop)
    order = np.argsort(-pop, kind="stable")
    for u, n_keep in ((0, 30), (3, 0), (130, 49), (255, 1), (256, 12), (nU - 1, 7), (777, 50), (999, 51)):
        keep = np.concatenate([order[:256][: n_keep // 2], order[256:][rng.permutation(nI - 256)[: n_keep - n_keep // 2]]]).astype(np.int32)
        rows[u] = np.setdiff1d(np.arange(nI, dtype=np.int32), keep).astype(np.int32)


# slowly falling, never tying popularities on small catalogues: every row is appended to, flags come at many half-tiles; a partial wave
# (1 000 users), a partial workgroup (1 100) and a third workgroup (2 050); both table types, both kinds of history
@pytest.mark.parametrize("d,bf16,nU,nI", [(64, False, 1000, 700), (64, True, 2050, 1500), (128, False, 1100, 1500), (128, True, 1000, 700),
                                          (256, False, 2050, 700), (256, True, 1100, 1500), (128, False, 2050, 700), (64, False, 1100, 1500)])
@pytest.mark.parametrize("by_user", [True, False])
def test_flags_at_many_half_tiles(dev, d, bf16, nU, nI, by_user):
    rng = np.random.default_rng(d + nU + nI + (1 if bf16 else 0))
    nT = nU + 50
    U, I, pop, rows = case(rng, nT, nI, d, flat=True)
    if bf16:
        U, I = bf16_exact(U), bf16_exact(I)
    short_rows(rng, rows, pop, nU)
    users = np.arange(nU) if by_user else rng.permutation(nT)[:nU]
    got, ref, st, entries = run_case(dev, U, I, pop, rows, users, by_user, bf16)
    per_user = float(st["pairs_rescored"][0]) / nU
    print("d %d bf16 %s %d users x %d items: %.2f loop entries per wave, %.1f exact rescorings per user" % (d, bf16, nU, nI, entries, per_user))
    assert entries > 1.0 and per_user > 2.0, (entries, per_user)
    assert torch.equal(got, ref), int((got != ref).sum())


# the guards of the fused extract: one to four half-tiles behind the warm-up's 256 items -- a flag is met at h = 1 (no half-tile h - 2),
# at h = 2 and at the split's last half-tile (the half-tile behind it does not exist).
# With one or two half-tiles (288, 320 items) the loop has reached the split's end when it leaves on a flag: nothing is entered again, and the
# counter of loop ENTRIES stays at one per wave however many exits there were (measured: 1.00, with 1.36 exact rescorings per user at 288
# items) -- there the exits are witnessed by the rescored pairs, which reach the ring through an exit's extract and no other way.
@pytest.mark.parametrize("nI", [288, 320, 352, 384])
@pytest.mark.parametrize("d", [64, 128])
def test_flags_at_the_first_and_last_half_tiles(dev, nI, d):
    rng = np.random.default_rng(nI + d)
    nU = 1100
    U, I, pop, rows = case(rng, nU, nI, d, flat=True)
    got, ref, st, entries = run_case(dev, U, I, pop, rows, np.arange(nU), True, False)
    # the floor of the rescored pairs comes from the exact kernel's lists: an item behind the warm-up's 256 positions reaches a list only
    # through an exit's extract, the ring and its exact rescoring, so every such entry of the final lists is at least one rescored pair
    from pda_amd import ops
    behind = np.argsort(-pop, kind="stable")[256:]
    idx, _ = ops.unpack_keys(ref)
    n_behind = int(np.isin(idx, behind).sum())
    rescored = int(st["pairs_rescored"][0])
    print("%d items, d %d: %.2f loop entries per wave, %.2f exact rescorings per user, %.2f list entries per user from behind the warm-up"
          % (nI, d, entries, rescored / nU, n_behind / nU))
    assert st["n_splits"] == 1 and n_behind > 0 and rescored >= n_behind, (st["n_splits"], entries, rescored, n_behind)
    if nI > 320:
        assert entries > 1.0, entries
    assert torch.equal(got, ref), int((got != ref).sum())


# several item splits behind the shared warm-up: the end handed to the tested body clamps inside a split
@pytest.mark.parametrize("d,bf16", [(128, False), (256, True)])
def test_flags_in_item_splits(dev, d, bf16):
    rng = np.random.default_rng(20000 + d)
    nU, nI = 2050, 20000
    U, I, pop, rows = case(rng, nU, nI, d, flat=True)
    if bf16:
        U, I = bf16_exact(U), bf16_exact(I)
    got, ref, st, entries = run_case(dev, U, I, pop, rows, np.arange(nU), True, bf16)
    print("d %d: %d splits, %.2f loop entries per wave" % (d, st["n_splits"], entries))
    assert st["n_splits"] > 1 and entries > 1.0 and float(st["pairs_rescored"][0]) / nU > 2.0
    assert torch.equal(got, ref), int((got != ref).sum())
