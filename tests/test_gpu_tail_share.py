"""The huge geometry's SHARED test-free tail (pda_amd/csrc/pda_tail_share.h, pda_v5_sweep.h): a workgroup publishes the decided part of its
split in a record, and workgroups that have emitted their rows claim chunks of it.  Which CU runs a decided half-tile changes no result:
packed keys bit for bit against the exact kernel (impl="v1") and against the same call without sharing (PDA_SWEEP_TAIL_SHARE=0), the
counters equal to the run without sharing, every record exhausted.  The smallest chunk is forced down to 2 half-tiles; the geometry is
forced the way tests/test_gpu_huge_decided_tail.py forces it, and the identity word is asserted on every call.  Stolen chunks are printed
per case: no result may depend on whether a steal happened."""
import numpy as np
import pytest
import torch

from decided_tail_cases import csr, steep_case

pytestmark = pytest.mark.gpu
K = 50


@pytest.fixture(autouse=True)
def huge(monkeypatch):
    monkeypatch.setenv("PDA_SCORE_IMPL", "v2")
    monkeypatch.setenv("PDA_CHECK_SWEEP_ERRORS", "1")
    monkeypatch.setenv("PDA_SCORE_PRUNE", "order")
    monkeypatch.setenv("PDA_SCORE_LISTS", "huge")
    monkeypatch.setenv("PDA_SCORE_KERNEL", "v4")
    monkeypatch.setenv("PDA_SWEEP_TAIL_MIN_CHUNK", "2")


def user_tile(d):
    return 512 if d == 256 else 1024


_cases = {}


def case(dev, nU, nI, d, bf16, popk):
    """-> the tensors of one shape and its exact keys (impl="v1" on the fp32 tables), computed once and shared"""
    from pda_amd import ops
    key = (nU, nI, d, bf16, popk)
    if key not in _cases:
        rng = np.random.default_rng(1000 + nU + nI + d + (7 if bf16 else 0))
        U, I, pop, rows = steep_case(rng, nU, nI, d, ratio=0.995)
        if popk == "flat":
            pop[:] = 0.5
        Uf, If, pt = torch.from_numpy(U).to(dev), torch.from_numpy(I).to(dev), torch.from_numpy(pop).to(dev)
        if bf16:                                                          # (bf16-exact values: the fp32 tables of the reference hold the same numbers)
            Uf, If = Uf.bfloat16().float(), If.bfloat16().float()
        ip, ix = csr(rows)
        h = ops.HistoryCSR(torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev), by_user=True)
        ut = torch.arange(nU, dtype=torch.int32, device=dev)
        ref = ops.topk_merge(ops.score_topk_keys(Uf, If, ut, K, ops.HEAD_POP, pt, h, 0, impl="v1"), want="keys")
        _cases[key] = (Uf.bfloat16() if bf16 else Uf, If.bfloat16() if bf16 else If, pt, h, ut, ref)
    return _cases[key]


def run(c, n_splits, d):
    """one call of the huge geometry -> (merged keys, counters)"""
    from pda_amd import ops
    Ut, It, pt, h, ut, _ = c
    st = {}
    got = ops.score_topk_keys(Ut, It, ut, K, ops.HEAD_POP, pt, h, 0, n_splits, impl="v2", prune="order", stats=st)
    assert got.shape[0] == n_splits
    got = ops.topk_merge(got, want="keys")
    torch.cuda.synchronize()
    assert int(st["error"][0]) == 0
    ident = ops.kernel_identity(st["kernel_id"][0])
    assert ident["generation"] == 4 and ident["geometry"] == "huge" and ident["d"] == d, ident
    n = {k: int(st[k][0]) for k in ("tiles_scored", "huge_free_halftiles", "huge_entries", "tail_stolen_chunks", "tail_stolen_halftiles")}
    n["tiles_dense"] = int(st["tiles_dense"])
    n["records"] = st["tail_records"].cpu().numpy().astype(np.uint64)
    return got, n


def assert_records_exhausted(rec, share=True):
    nxt, end = (rec & np.uint64(0xFFFFFFFF)).astype(np.int64), (rec >> np.uint64(32)).astype(np.int64)
    assert np.array_equal(nxt, end), (nxt, end)                           # (an unpublished record: 0 == 0)
    if not share:
        assert not rec.any()


def check(monkeypatch, c, n_splits, d):
    ref = c[5]
    monkeypatch.setenv("PDA_SWEEP_TAIL_SHARE", "0")
    plain, n0 = run(c, n_splits, d)
    monkeypatch.delenv("PDA_SWEEP_TAIL_SHARE")
    got, n1 = run(c, n_splits, d)
    print("free half-tiles %d, entries %d (unshared %d); chunks run for other workgroups %d (%d half-tiles)" %
          (n1["huge_free_halftiles"], n1["huge_entries"], n0["huge_entries"], n1["tail_stolen_chunks"], n1["tail_stolen_halftiles"]))
    assert torch.equal(plain, ref), int((plain != ref).sum())
    assert torch.equal(got, ref), int((got != ref).sum())
    assert torch.equal(got, plain)
    assert n1["tiles_scored"] == n0["tiles_scored"] and n1["tiles_scored"] >= n1["tiles_dense"], (n1, n0)
    assert n1["huge_free_halftiles"] == n0["huge_free_halftiles"], (n1, n0)
    assert n0["tail_stolen_chunks"] == 0 and n0["tail_stolen_halftiles"] == 0
    assert n1["tail_stolen_halftiles"] <= n1["huge_free_halftiles"]
    assert_records_exhausted(n0["records"], share=False)
    assert_records_exhausted(n1["records"])
    return n1


@pytest.mark.parametrize("popk", ["flat", "steep"])
@pytest.mark.parametrize("n_splits", [1, 3])
@pytest.mark.parametrize("d,bf16", [(64, False), (64, True), (128, False), (128, True), (256, True)])
@pytest.mark.parametrize("nI", [1500, 5000])
@pytest.mark.parametrize("nU", [2050, 3100])
def test_keys_and_counters_with_and_without_sharing(dev, monkeypatch, nU, nI, d, bf16, n_splits, popk):
    n = check(monkeypatch, case(dev, nU, nI, d, bf16, popk), n_splits, d)
    wgs = -(-nU // user_tile(d)) * n_splits
    assert len(n["records"]) == wgs
    if popk == "flat":
        assert n["huge_free_halftiles"] == 0 and not n["records"].any()   # nothing is ever decided: nothing published
    else:
        total = 2 * (-(-nU // user_tile(d))) * (-(-nI // 64) - 4)
        assert n["huge_free_halftiles"] >= total // 2, (n["huge_free_halftiles"], total)      # most of a split is test-free


# the test mode: a workgroup that has published looks at the OTHER records first.  Same keys, same counters -- and here chunks do move.
@pytest.mark.parametrize("d,bf16,n_splits", [(128, False, 1), (64, True, 3), (256, True, 1)])
def test_others_first_moves_chunks_and_changes_nothing(dev, monkeypatch, d, bf16, n_splits):
    monkeypatch.setenv("PDA_SWEEP_TAIL_OTHERS_FIRST", "1")
    n = check(monkeypatch, case(dev, 3100, 5000, d, bf16, "steep"), n_splits, d)
    assert n["tail_stolen_chunks"] > 0 and n["tail_stolen_halftiles"] >= 2 * n["tail_stolen_chunks"], n


# one workgroup that never goes test-free: a row of it has fewer than K unmasked items, its threshold stays -inf.  It publishes nothing;
# the others share among themselves, finish and leave.
@pytest.mark.parametrize("others_first", [False, True])
def test_a_workgroup_that_never_publishes(dev, monkeypatch, others_first):
    from pda_amd import ops
    if others_first:
        monkeypatch.setenv("PDA_SWEEP_TAIL_OTHERS_FIRST", "1")
    nU, nI, d = 3100, 5000, 128
    rng = np.random.default_rng(90)
    U, I, pop, rows = steep_case(rng, nU, nI, d, ratio=0.995)
    keep = rng.permutation(nI)[:30]
    rows[1024 + 5] = np.setdiff1d(np.arange(nI, dtype=np.int32), keep).astype(np.int32)       # a row of workgroup 1 may rank 30 items
    Ut, It, pt = torch.from_numpy(U).to(dev), torch.from_numpy(I).to(dev), torch.from_numpy(pop).to(dev)
    ip, ix = csr(rows)
    h = ops.HistoryCSR(torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev), by_user=True)
    ut = torch.arange(nU, dtype=torch.int32, device=dev)
    ref = ops.topk_merge(ops.score_topk_keys(Ut, It, ut, K, ops.HEAD_POP, pt, h, 0, impl="v1"), want="keys")
    n = check(monkeypatch, (Ut, It, pt, h, ut, ref), 1, d)
    assert int((ref[1024 + 5] != 0).sum()) == 30
    rec = n["records"]
    assert rec[1] == 0 and rec[0] != 0 and rec[2] != 0 and rec[3] != 0, rec
    per_wg = 2 * (-(-nI // 64) - 4)
    assert 0 < n["huge_free_halftiles"] <= 3 * per_wg


# two calls in a row on ONE workspace, a larger block first: the second call finds the first one's records (exhausted ones in front, and one
# behind its own) and every other byte of the first call.  Its keys, counters and records must be those of a call on a fresh workspace.
@pytest.mark.parametrize("others_first", [False, True])
def test_two_calls_on_one_workspace(dev, others_first):
    from pda_amd import ops
    lib = ops._lib.load()
    d, nI = 128, 5000
    big, small = case(dev, 3100, nI, d, False, "steep"), case(dev, 2050, nI, d, False, "steep")
    Ut, It, pt, h = big[0], big[1], big[2], big[3]
    Us, Is, ps, hs = small[:4]
    es = 128 | ops.SWEEP_TAIL_MIN2 | (ops.SWEEP_TAIL_OTHERS_FIRST if others_first else 0)      # PDA_SWEEP_HUGE
    ws = torch.full((lib.pda_score_topk4_workspace_bytes(3100, nI, d, 1),), 0xFF, dtype=torch.uint8, device=dev)
    off = ops.tail_record_offset(3100)
    assert off == ops.tail_record_offset(2050)

    def call(Uc, Ic, pc, hc, nU):
        order = ops.visiting_order(Ic, pc)
        prep = ops.item_prep4(Ic, pc, order)
        ut = torch.arange(nU, dtype=torch.int32, device=dev)
        out = torch.empty((1, nU, K), dtype=torch.int64, device=dev)
        ops.check(lib.pda_score_topk4_f32(ops.ptr(Uc), ops.ptr(Ic), ops.ptr(prep), ops.ptr(pc), ops.ptr(ut), nU, 0, nI, d, ops.ptr(hc.indptr),
                                          ops.ptr(hc.indices), hc.mode, K, ops.HEAD_POP, es, 1, ops.ptr(out), ops.ptr(ws), ops.stream_ptr()), "pda_score_topk4")
        torch.cuda.synchronize()
        assert int(ws[0:4].view(torch.int32)[0]) == 0
        ident = ops.kernel_identity(ws[16:20].view(torch.int32)[0])
        assert ident["generation"] == 4 and ident["geometry"] == "huge", ident
        n = {"tiles_scored": int(ws[8:16].view(torch.int64)[0]), "free": int(ws[28:32].view(torch.int32)[0]), "stolen": int(ws[36:40].view(torch.int32)[0])}
        return ops.topk_merge(out, want="keys"), n, ws[off:off + 8 * 8].view(torch.int64).cpu().numpy().astype(np.uint64)

    k1, n1, r1 = call(Ut, It, pt, h, 3100)
    assert torch.equal(k1, big[5])
    assert r1[:4].all()
    assert_records_exhausted(r1[:4])
    k2, n2, r2 = call(Us, Is, ps, hs, 2050)
    print("first call: %s; second call: %s" % (n1, n2))
    assert torch.equal(k2, small[5]), int((k2 != small[5]).sum())
    assert r2[:3].all() and not r2[3:].any(), r2                          # the stale fourth record is gone, not merely ignored
    assert_records_exhausted(r2[:3])
    fresh = torch.zeros_like(ws)
    ws = fresh
    k3, n3, _ = call(Us, Is, ps, hs, 2050)
    assert torch.equal(k3, k2)
    assert n2["tiles_scored"] == n3["tiles_scored"] and n2["free"] == n3["free"], (n2, n3)
