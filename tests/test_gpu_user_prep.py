"""GPU: the user side of the pre-filter, field by field, against tests/user_prep_ref.py -- the per-block user image (bf16 for the huge geometry, fp16
for the funnel), its padded norms, the funnel's padded residual norms and the Bloom filters of the train items.  Every pre-filtered score + top-K
path is exact only if these are right; the rest of the suite sees them only through the lists behind them, where a bound that is wrong for an
adversarial pair, or merely loose, changes nothing.

Each field is built through the per-block entries (ops.huge_user_image, ops.funnel_user_image, ops.hist_bloom_rows, ops.funnel_bloom_rows: the
per-call kernels on one block as calls of their own), copied to the host once, decoded by the restated layout and held to conditions computed from
the inputs alone: float64 inequalities with prep_ref's a-priori caps where the field is a bound, bit equality everywhere else.  The cases are the
smallest shapes at which a mechanism changes: d in {64, 128, 256}, fp32 and bf16 tables, both images, blocks of {1, 17, 255, 257, 1 025} rows
({1, 17, 127, 129, 513} at d = 256: a 16-user fragment, a wave's rows, a workgroup's), shuffled user ids with repeats out of a 2 000-row table that
holds every row kind (user_prep_ref.make_table); histories of 0 .. 1 025 entries (every remainder of the 8-lanes x 4-loads loop), ids up to
2^31 - 1, both history modes, blocks of {1, 31, 32, 33, 70} rows behind a sentinel fill, a real ordered prep7 of a 300-item shard at offset 100.
The image the one-call dense sweep's warm-up leaves in its workspace (warm_score5_kernel + warm_select5_kernel, warm4_kernel) is decoded and held to
the same restatement directly.  tests/test_user_prep_host.py shows on the CPU that an fp32 emulation meets every condition on every case here and
that fourteen single-defect mutants each fail the condition they name.

Every test prints its smallest..largest ratio per field.  Observed on an MI355X (recorded, not thresholds), over all cases; the pad itself is
1.0010767, cap(d) = 1.0010788 / 1.0010807 / 1.0010845 and floor(d) = 1.0010745 / 1.0010726 / 1.0010688 at d = 64 / 128 / 256:
    stored norm / exact norm                      1.0010765 .. 1.0010768   (uprep5_kernel, both images, every d and table type; the same range in the
                                                                           workspace of the dense call behind warm_score5 + warm_select5 and behind warm4_kernel)
    stored residual norm / exact residual norm    1.0010765 .. 1.0010769   (the funnel's uerr; bf16 tables: 1.0010766 .. 1.0010767, only the clamped, tiny and
                                                                           sub-subnormal rows have a residual at all)
    every bit equality (bf16 and fp16 images, padding rows, zero norms, both Bloom filters: 0 .. 894 of 1 024 bits per row for generation 4,
    0 .. 439 for the funnel's 300-item shard; the sentinel behind every block): exact.
No condition failed on the device; no kernel was changed.
"""
import numpy as np
import pytest
import torch

import prep_ref as pr
import test_gpu_dense_call_passes as dcp
import user_prep_ref as ur

pytestmark = pytest.mark.gpu
checked = dcp.checked                       # (the same environment as the dense call's own tests: sweep errors checked, no forcing variable set)
F = np.float32
SENTINEL = 0x5A5A5A5A
_TABLES = {}


def device_table(dev, d, bf16):
    """the case table on the device, once per (d, type)"""
    if (d, bf16) not in _TABLES:
        U32, Ubits = ur.make_table(d, bf16)
        _TABLES[d, bf16] = torch.from_numpy(Ubits.view(np.int16).copy()).to(dev).view(torch.bfloat16) if bf16 else torch.from_numpy(U32.copy()).to(dev)
    return _TABLES[d, bf16]


@pytest.mark.parametrize("c", ur.gpu_cases(), ids=ur.case_id)
def test_every_field_of_the_user_image(dev, c):
    from pda_amd import ops
    U32, Ubits = ur.make_table(c.d, c.bf16)
    users = ur.make_users(c)
    Ut, ut = device_table(dev, c.d, c.bf16), torch.from_numpy(users).to(dev)
    if c.f16:
        ufrag, unorm, uerr = ops.funnel_user_image(Ut, ut)
    else:
        (ufrag, unorm), uerr = ops.huge_user_image(Ut, ut), None
    torch.cuda.synchronize()
    assert ufrag.numel() == ur.image_bytes(c.n, c.d) and unorm.numel() == ur.n_pad(c.n, c.d) == ops.huge_image_offsets(c.n, 20000, c.d, 1)[3]
    R = ur.check_user_image(ufrag.cpu().numpy(), unorm.cpu().numpy(), None if uerr is None else uerr.cpu().numpy(), U32, Ubits, users, c.d, c.f16)
    print("%s: %s" % (ur.case_id(c), R.line()))
    assert not R.failed, R.failed


# the image the warm-up of a one-call dense sweep leaves in the workspace, held to the restatement itself (not to uprep5_kernel's bytes): block rows
# drawn with repeats from the case table, so every row kind passes through the warm-up's own rounding and summation
@pytest.mark.parametrize("d,bf16,one_kernel", [(64, False, False), (128, True, False), (256, False, False), (128, False, True)])
def test_the_warm_up_image_of_the_dense_call(dev, monkeypatch, d, bf16, one_kernel):
    from pda_amd import ops
    if one_kernel:
        monkeypatch.setenv("PDA_WARM_ONE_KERNEL", "1")
    rng = np.random.default_rng(500 + d)
    nU, nI = (8200 if d == 256 else 17003) + d, 20000
    _, I, pop, rows = dcp.case(rng, ur.TABLE_ROWS, nI, d)
    U32, Ubits = ur.make_table(d, bf16)
    users = np.concatenate([np.array(sorted(ur.SPECIAL), np.int32), rng.integers(0, ur.TABLE_ROWS, nU - len(ur.SPECIAL)).astype(np.int32)])
    users = rng.permutation(users).astype(np.int32)
    Ut, ut = device_table(dev, d, bf16), torch.from_numpy(users).to(dev)
    It, pt = torch.from_numpy(I).to(dev), torch.from_numpy(pop).to(dev)
    if bf16:
        It = It.bfloat16()
    h = dcp.hist_of(dev, rows, users, True)
    plan = ops.score_plan(nU, nI, d, dcp.K, ops.HEAD_POP, "order", bf16, h)
    assert plan["kernel"] == "v4" and plan["early_stop"] & 128, plan            # PDA_SWEEP_HUGE, chosen by the library
    st = {}
    ops.score_topk_keys(Ut, It, ut, dcp.K, ops.HEAD_POP, pt, h, 0, 0, impl="v2", prune="order", stats=st)
    torch.cuda.synchronize()
    assert int(st["error"][0]) == 0
    ident = ops.kernel_identity(st["kernel_id"][0])
    assert ident["generation"] == 4 and ident["geometry"] == "huge" and ident["d"] == d and ident["bf16"] == bf16, ident
    assert int(st["warm_kernels"][0]) == (5 if d <= 128 and not one_kernel else 0)
    o_img, o_norm, _, npad = ops.huge_image_offsets(nU, nI, d, st["n_splits"])
    assert npad == ur.n_pad(nU, d)
    ws = st["workspace"]
    raw = ws[o_img:o_img + ur.image_bytes(nU, d)].cpu().numpy()
    unorm = ws[o_norm:o_norm + 4 * npad].view(torch.float32).cpu().numpy()
    R = ur.check_user_image(raw, unorm, None, U32, Ubits, users, d, False)
    print("warm-up d %d %s %s: %s" % (d, "bf16" if bf16 else "f32", "warm4_kernel" if int(st["warm_kernels"][0]) == 0 else "score + select", R.line()))
    assert not R.failed, R.failed


# ---- the Bloom filters -----------------------------------------------------------------------------------------------------------------------------
def device_history(dev, funnel, by_user):
    from pda_amd import ops
    indptr, indices = ur.make_history(funnel)
    return ops.HistoryCSR(torch.from_numpy(indptr.copy()).to(dev), torch.from_numpy(indices.copy()).to(dev), by_user=by_user)


def item_table(dev, n):
    return torch.from_numpy((np.random.default_rng(20262).standard_normal((n, 64)) * 0.1).astype(F)).to(dev)


@pytest.mark.parametrize("c", ur.bloom_cases(), ids=ur.bloom_case_id)
def test_bloom_rows(dev, c):
    from pda_amd import ops
    indptr, indices = ur.make_history(c.funnel)
    users = ur.make_bloom_users(c)
    ut, h = torch.from_numpy(users).to(dev), device_history(dev, c.funnel, c.by_user)
    guard = 5
    out = torch.full((c.n + guard, 32), SENTINEL, dtype=torch.int32, device=dev)
    shard = None
    if c.funnel:
        order, pos_of = ur.shard_order()
        prep7 = ops.item_prep7(item_table(dev, ur.SHARD_ITEMS), torch.from_numpy(order).to(dev))
        ops.funnel_bloom_rows(prep7, ut, h, ur.SHARD_OFFSET, ur.SHARD_ITEMS, 64, out=out)
        torch.cuda.synchronize()
        f = pr.decode_prep4(prep7.cpu().numpy(), ur.SHARD_ITEMS, 64)
        assert np.array_equal(f["pos_of"], pos_of) and f["hdr"][2] == 1 and f["hdr"][3] == 1          # a real ordered prep7
        shard = (pos_of, ur.SHARD_OFFSET)
    else:
        ops.hist_bloom_rows(ops.item_prep4(item_table(dev, 64), None, None), ut, h, out=out)
        torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[c.n:] == SENTINEL).all(), "rows behind the block were written"
    R = ur.check_bloom(got[:c.n], users, indptr, indices, c.by_user, shard)
    assert not R.failed, R.failed
    fill = np.unpackbits(got[:c.n].view(np.uint8), axis=1).sum(1)
    print("%s: %d .. %d of 1 024 bits set per row, every word exact" % (ur.bloom_case_id(c), fill.min(), fill.max()))


@pytest.mark.parametrize("by_user", [True, False])
def test_generation_4_skips_the_filters_of_an_ordered_prep(dev, by_user):
    """skip_if_ordered with a prep built with an order: the call writes nothing (sweeps of the popularity head in visiting order never read the filters);
    either of the two alone: the filters are written, the same words"""
    from pda_amd import ops
    c = ur.BloomCase(False, by_user, 33)
    indptr, indices = ur.make_history(False)
    users = ur.make_bloom_users(c)
    ut, h = torch.from_numpy(users).to(dev), device_history(dev, False, by_user)
    It = item_table(dev, 64)
    ordered = ops.item_prep4(It, None, torch.randperm(64, device=dev).to(torch.int32))
    natural = ops.item_prep4(item_table(dev, 64), None, None)
    outs = []
    for prep, skip in ((ordered, True), (ordered, False), (natural, True)):
        out = torch.full((c.n + 5, 32), SENTINEL, dtype=torch.int32, device=dev)
        ops.hist_bloom_rows(prep, ut, h, skip_if_ordered=skip, out=out)
        outs.append(out)
    torch.cuda.synchronize()
    skipped, a, b = (o.cpu().numpy().view(np.uint32) for o in outs)
    assert (skipped == SENTINEL).all()
    for got in (a, b):
        assert (got[c.n:] == SENTINEL).all()
        R = ur.check_bloom(got[:c.n], users, indptr, indices, by_user)
        assert not R.failed, R.failed
