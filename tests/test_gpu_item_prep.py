"""GPU: the item prep blob, field by field, against tests/prep_ref.py -- float64 where a field is a bound, bit for bit where it is a rounding or a
maximum of stored values.  Every pre-filtered score + top-K path (generation 3, generation 4, the huge geometry, the funnel) trusts this blob; the
rest of the suite sees it only through the lists behind it, where a bound that is wrong for an adversarial pair, or merely loose, changes nothing.

The preps are built through ops.item_prep4 / item_prep7 / item_prep_ordered / item_prep, copied to the host once and decoded by the restated
layout.  The cases (prep_ref.gpu_cases) are the smallest shapes at which a mechanism changes: d in {64, 128, 256} (threads per row, the swizzle
rule), both table types, n in {1, 63, 64, 65, 4 097} (a tile of padding, a full tile, a half-tile of padding only, a ragged end), 65 600 items at
d = 64 (suffix_max4_kernel's two tiles per thread, suffix_max_kernel's three) with the largest |pop| ||i|| at the seam, every popularity kind
(none, uniform^0.22, exact zeros, below 1e-6, NaN, all 1.0), every order kind (none, random, ops.visiting_order), rows that are zero, scaled by
1e-18 and by 1e4, and an entry of 7e4 for the fp16 clamp.  Overflow or underflow of a row's sum of squares in fp32 is out of scope (the precondition
is stated in include/pda_hip.h); the thresholds are prep_ref's a-priori ones.  tests/test_prep_host.py shows on the CPU that an fp32 emulation meets
every condition on every case here and that sixteen single-defect mutants each fail a named one.

Every test prints its smallest..largest ratio per field.  Observed on an MI355X (recorded, not thresholds), over all cases; the pad itself is
1.0010767, cap(d) = 1.0010788 / 1.0010807 / 1.0010845 at d = 64 / 128 / 256, and (1/pop)' may go down to 1 - 2^-20 = 0.9999990:
    stored norm / exact norm                  1.0010765 .. 1.0010769   (row tail, pinfo, generation-3 norm; the same at every d and for both preps)
    residual norm / exact residual norm       1.0010765 .. 1.0010769   (prep4 bf16 image and prep7 fp16 image)
    meta5 nmax / exact max pop ||i||          1.0010774 .. 1.0010778   (the allowance is cap x 1.000002)
    sufB / exact max |pop| ||i||              1.0010775 .. 1.0010778   (generation 4 and generation 3; 65 600 items with the maximum at every seam too)
    (1/pop)' x pop, pop >= 1e-6               0.9999994 .. 0.9999996
    every bit-equality (rows, images, pmax, rmax, sufA, sufR, pos_of, tail, pinfo, headers) and every hist_reorder row: exact.
No condition failed on the device; no kernel was changed.
"""
import numpy as np
import pytest
import torch

import prep_ref as pr

pytestmark = pytest.mark.gpu
F = np.float32


def device_inputs(dev, inp):
    """-> (table, pop or None) on the device: fresh tensors, so that the preps' caches (keyed on the table object) never serve an older blob"""
    if inp["Ibits"] is not None:
        It = torch.from_numpy(inp["Ibits"].view(np.int16).copy()).to(dev).view(torch.bfloat16)
    else:
        It = torch.from_numpy(inp["I32"].copy()).to(dev)
    pt = None if inp["pop"] is None else torch.from_numpy(inp["pop"].copy()).to(dev)
    return It, pt


def build(dev, c, inp, order_t=None):
    """-> (blob as a host uint8 array, the order used as a host array or None, the order tensor)"""
    from pda_amd import ops
    It, pt = device_inputs(dev, inp)
    if order_t is None and inp["order"] is not None:
        order_t = ops.visiting_order(It, pt) if isinstance(inp["order"], str) else torch.from_numpy(inp["order"]).to(dev)
    if c.kind == "prep4":
        buf = ops.item_prep4(It, pt, order_t)
    elif c.kind == "prep7":
        buf = ops.item_prep7(It, order_t)
    elif c.kind == "gen3o":
        buf, _ = ops.item_prep_ordered(It, pt, order_t)
    else:
        buf = ops.item_prep(It)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), None if order_t is None else order_t.cpu().numpy().astype(np.int32), order_t


@pytest.mark.parametrize("c", pr.gpu_cases(), ids=pr.case_id)
def test_every_field_of_the_prep(dev, c):
    inp = pr.make_inputs(c)
    blob, order, _ = build(dev, c, inp)
    R = pr.check(c, pr.decode(c, blob, inp["pop"] is not None), inp, order)
    print("%s: %s" % (pr.case_id(c), R.line()))
    assert not R.failed, R.failed


STABLE = [c for c in pr.gpu_cases() if (c.n == 4097 and c.d in (64, 256) and c.orderk in ("random", None) and c.popk in ("pow", "nan", None)) or c.n == 1]


@pytest.mark.parametrize("c", STABLE, ids=pr.case_id)
def test_two_preps_of_the_same_inputs_are_byte_identical(dev, c):
    """Two buffers, the same inputs: every byte the layout names is the same (the maxima are atomics on bit patterns, the flags idempotent).  The
    alignment gaps between the fields belong to nobody and are not compared."""
    inp = pr.make_inputs(c)
    blob_a, _, order_t = build(dev, c, inp)
    blob_b, _, _ = build(dev, c, inp, order_t)
    a = pr.named_bytes(pr.decode(c, blob_a, inp["pop"] is not None))
    b = pr.named_bytes(pr.decode(c, blob_b, inp["pop"] is not None))
    for k in a:
        assert np.array_equal(a[k], b[k]), (k, int((a[k] != b[k]).sum()))


@pytest.mark.parametrize("bad_kind", ["repeated", "out_of_range"])
def test_prep4_rejects_a_non_permutation(dev, bad_kind):
    """the generation-4 twin of test_gpu_score_topk.py::test_ordered_prep_rejects_a_non_permutation"""
    from pda_amd import ops
    n, d = 640, 64
    It = torch.randn(n, d, device=dev)
    good = torch.randperm(n, device=dev).to(torch.int32)
    lib = ops._lib.load()
    ops.check(lib.pda_item_prep4_check(ops.ptr(ops.item_prep4(It, None, good)), n, d, ops.stream_ptr()), "pda_item_prep4_check")
    bad = good.clone()
    bad[17] = bad[400] if bad_kind == "repeated" else n
    prep = ops.item_prep4(It, None, bad)
    with pytest.raises(ops._lib.PdaHipError):
        ops.check(lib.pda_item_prep4_check(ops.ptr(prep), n, d, ops.stream_ptr()), "pda_item_prep4_check")
    prep3, _ = ops.item_prep_ordered(It, None, bad)
    with pytest.raises(ops._lib.PdaHipError):
        ops.check_order(prep3, n, d)


def test_hist_reorder_rows(dev):
    """pda_hist_reorder on its own: rows of 0, 1, 63, 64, 65 (the first bitonic size and beyond), 1 024, 2 048 (the last row sorted in the LDS), 2 049
    and 3 000 (the rank sort) entries in one CSR, duplicates inside the rows, ids below, inside and above the shard [1 000, 6 000), a random order.
    Every row is the sorted image of its ids; the sentinel behind the last row is untouched (an empty row writes nothing)."""
    from pda_amd import ops
    rng = np.random.default_rng(20260)
    n, d, off = 5000, 64, 1000
    lens = [65, 0, 1, 2049, 63, 0, 64, 1024, 3000, 2048, 0]
    assert set(lens) == {0, 1, 63, 64, 65, 1024, 2048, 2049, 3000}
    rows = []
    for L in lens:
        r = rng.integers(0, off + n + 2000, L).astype(np.int32)
        if L >= 63:
            r[:6] = [0, off - 1, off, off + n - 1, off + n, off + n + 1999]          # both edges of the shard
            r[6:9] = [off + 7, off + 7, off + n + 5]                                   # duplicates inside and outside the shard
            r[9] = r[8]
        rows.append(np.sort(r))
        if L >= 1024:
            assert len(np.unique(r)) < L and (r < off).any() and (r >= off + n).any() and ((r >= off) & (r < off + n)).any()
    indptr = np.zeros(len(lens) + 1, np.int64)
    indptr[1:] = np.cumsum(lens)
    indices = np.concatenate(rows).astype(np.int32)
    order = rng.permutation(n).astype(np.int32)
    pos_of = np.zeros(n, np.int32)
    pos_of[order] = np.arange(n, dtype=np.int32)
    It = torch.from_numpy((rng.standard_normal((n, d)) * 0.1).astype(F)).to(dev)
    order_t = torch.from_numpy(order).to(dev)
    prep, _ = ops.item_prep_ordered(It, None, order_t)
    ops.check_order(prep, n, d)
    guard = 64
    out = torch.full((len(indices) + guard,), -7, dtype=torch.int32, device=dev)
    ip_t, ix_t = torch.from_numpy(indptr).to(dev), torch.from_numpy(indices).to(dev)
    ops.check(ops._lib.load().pda_hist_reorder(ops.ptr(prep), n, d, off, ops.ptr(ip_t), ops.ptr(ix_t), len(lens), ops.ptr(out), ops.stream_ptr()),
              "pda_hist_reorder")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for r, (b, e) in enumerate(zip(indptr[:-1], indptr[1:])):
        ids = indices[b:e]
        inside = (ids >= off) & (ids < off + n)
        want = np.sort(np.where(inside, off + pos_of[np.clip(ids - off, 0, n - 1)], ids))
        assert np.array_equal(got[b:e], want), (r, lens[r], int((got[b:e] != want).sum()))
    assert (got[len(indices):] == -7).all()
    print("hist_reorder rows %s: every row exact" % lens)
