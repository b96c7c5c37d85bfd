"""GPU suite of the four metrics entry points (ops.metrics_sums, metrics_sums_ordered, metrics_sums_deep, metrics_sums_deep_ordered) against
the float64 restatement of tests/metrics_ref.py, on that file's case table: row by row (a sum over one row is that row), the same row at
the wave and workgroup borders of a block of rows without targets, whole matrices at row counts around the borders and one that takes the
ordered reduction past 256 waves, and the short kernels against the deep ones bit for bit.

Precision, recall and hit ratio are one IEEE division of small integers: equal bits are demanded.  NDCG goes through the device's log2 and
a sequential sum of up to 1 024 discounts: rtol 1e-12, the tolerance every metrics test of the suite uses."""
import numpy as np
import pytest
import torch

import metrics_ref as mr

pytestmark = pytest.mark.gpu
RTOL = 1e-12
ENTRIES = ("short", "short_ordered", "deep", "deep_ordered")


def _entry(name):
    from pda_amd import ops
    return {"short": ops.metrics_sums, "short_ordered": ops.metrics_sums_ordered, "deep": ops.metrics_sums_deep,
            "deep_ordered": ops.metrics_sums_deep_ordered}[name]


def entries(k_cols):
    """The short pair runs for k_cols <= 64, the deep pair for every k_cols."""
    return ENTRIES if k_cols <= mr.SHORT_MAX else ENTRIES[2:]


def _dev_case(dev, lists, targets, ks):
    indptr, flat = mr.csr_of(targets)
    return (torch.tensor(lists, dtype=torch.int32, device=dev), torch.from_numpy(indptr).to(dev), torch.from_numpy(flat).to(dev),
            torch.tensor(ks, dtype=torch.int32, device=dev))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _check_rows(got, ref, what):
    """got, ref [..., 4, n_ks]: finite, precision / recall / hit ratio with equal bits, NDCG at RTOL."""
    assert np.isfinite(got).all(), what
    for m in (0, 1, 3):
        np.testing.assert_array_equal(_bits(got[..., m, :]), _bits(ref[..., m, :]), err_msg="%s: %s" % (what, mr.NAMES[m]))
    np.testing.assert_allclose(got[..., 2, :], ref[..., 2, :], rtol=RTOL, atol=0, err_msg="%s: ndcg" % what)


def test_the_table_holds_its_cases():
    mr.check_table()


WHICH = pytest.mark.parametrize("which", [0, 1], ids=["six_cutoffs", "one_cutoff"])


@WHICH
@pytest.mark.parametrize("k_cols", mr.K_COLS)
def test_every_row_alone_and_at_the_borders_of_an_empty_block(dev, k_cols, which):
    """Each hand-built row and a sample of random rows: alone at either list of cut-offs, then (at the single cut-off) at rows 0, 63, 64
    and 255 of a block whose other rows have no targets, so that those must add exactly zero.  The short and the deep kernels: equal bits
    in all four metrics."""
    names, lists, targets = mr.matrix(k_cols)
    picks = mr.single_rows(k_cols)
    n_launch = 0
    for ks in [mr.ks_lists(k_cols)[which]]:
        ref = mr.matrix_ref(k_cols, which)
        ksd = torch.tensor(ks, dtype=torch.int32, device=dev)
        out = {e: [] for e in entries(k_cols)}
        placed = {e: [] for e in entries(k_cols)}
        for i in picks:
            row = torch.tensor([lists[i]], dtype=torch.int32, device=dev)
            tgt = torch.tensor(targets[i], dtype=torch.int32, device=dev)
            ip = torch.tensor([0, len(targets[i])], dtype=torch.int64, device=dev)
            block = row.repeat(mr.BLOCK_ROWS, 1)           # (the other rows hold the same list: without targets they add nothing)
            for e in entries(k_cols):
                out[e].append(_entry(e)(row, ip, tgt, ksd))
                n_launch += 1
                if which == 1:                             # (the single cut-off: the walk over a long row costs once per cut-off)
                    for at in mr.PLACES:
                        bp = torch.zeros(mr.BLOCK_ROWS + 1, dtype=torch.int64, device=dev)
                        bp[at + 1:] = len(targets[i])
                        placed[e].append(_entry(e)(block, bp, tgt, ksd))
                        n_launch += 1
        for e in entries(k_cols):
            got = torch.stack(out[e]).cpu().numpy()
            _check_rows(got, ref[picks], "%s k_cols %d Ks %s rows %s" % (e, k_cols, ks, [names[i] for i in picks]))
            if which == 1:
                gp = torch.stack(placed[e]).cpu().numpy().reshape(len(picks), len(mr.PLACES), 4, len(ks))
                for j, at in enumerate(mr.PLACES):
                    _check_rows(gp[:, j], ref[picks], "%s k_cols %d Ks %s at row %d of an empty block" % (e, k_cols, ks, at))
                    np.testing.assert_array_equal(_bits(gp[:, j]), _bits(got), err_msg="%s: row %d of an empty block against the row alone" % (e, at))
            out[e] = got
        if k_cols <= mr.SHORT_MAX:                         # cross-kernel agreement, row by row
            for a in ENTRIES[1:]:
                np.testing.assert_array_equal(_bits(out[a]), _bits(out["short"]), err_msg="%s against short, k_cols %d Ks %s" % (a, k_cols, ks))
        else:
            np.testing.assert_array_equal(_bits(out["deep_ordered"]), _bits(out["deep"]), err_msg="k_cols %d Ks %s" % (k_cols, ks))
    assert n_launch <= 450                                 # (some 4 000 single-row launches over the ten k_cols and both lists)


def _whole(dev, lists, targets, ks, ref_rows, k_cols, what):
    topk, ip, fl, ksd = _dev_case(dev, lists, targets, ks)
    ref = mr.fsum_rows(ref_rows)
    assert (ref[1] > 0).all() or len(lists) == 1           # (a relative tolerance on a sum that is not zero)
    for e in entries(k_cols):
        fn = _entry(e)
        got = fn(topk, ip, fl, ksd)
        g = got.cpu().numpy()
        assert np.isfinite(g).all(), (e, what)
        np.testing.assert_allclose(g, ref, rtol=RTOL, atol=0, err_msg="%s %s" % (e, what))
        np.testing.assert_array_equal(g[3], ref[3], err_msg="%s %s: a sum of zeros and ones" % (e, what))
        twice = fn(topk, ip, fl, ksd, got.clone())         # `sums` is added to
        if e.endswith("ordered"):
            assert torch.equal(fn(topk, ip, fl, ksd).view(torch.int64), got.view(torch.int64)), (e, what)   # the same bits run after run
            assert torch.equal(twice, got + got), (e, what)
        else:                                              # (atomics: the second call's sums land on the first's in any order)
            np.testing.assert_allclose(twice.cpu().numpy(), 2.0 * ref, rtol=RTOL, atol=0, err_msg="%s %s twice" % (e, what))


@WHICH
@pytest.mark.parametrize("n_rows", mr.ROW_COUNTS)
@pytest.mark.parametrize("k_cols", mr.K_COLS)
def test_whole_matrices_against_the_exactly_rounded_sums(dev, k_cols, n_rows, which):
    _, lists, targets = mr.matrix(k_cols)
    ks = mr.ks_lists(k_cols)[which]
    _whole(dev, lists[:n_rows], targets[:n_rows], ks, mr.matrix_ref(k_cols, which)[:n_rows], k_cols, "k_cols %d rows %d Ks %s" % (k_cols, n_rows, ks))


def test_the_ordered_sum_past_256_waves_with_a_ragged_last_one(dev):
    _, lists, targets = mr.large_matrix()
    n_waves = 4 * ((mr.LARGE_ROWS + 255) // 256)
    assert n_waves > 4 * 256 and n_waves % 256 != 0
    _whole(dev, lists, targets, mr.ks_lists(mr.LARGE_K_COLS)[0], mr.large_ref(), mr.LARGE_K_COLS, "the large case")


@pytest.mark.parametrize("k_cols", [64, 65])
def test_the_trainers_routing_reaches_both_kernel_families(dev, k_cols):
    """ops.metrics_route at the two sides of the limit: 64 columns are taken by the short kernels (bit 63 of the hit mask), 65 by the deep
    ones (the short ones refuse them)."""
    from pda_amd import _lib, ops
    _, lists, targets = mr.matrix(k_cols)
    ks = mr.ks_lists(k_cols)[0]
    topk, ip, fl, ksd = _dev_case(dev, lists, targets, ks)
    ref = mr.fsum_rows(mr.matrix_ref(k_cols, 0))
    for ordered in (False, True):
        fn = ops.metrics_route(k_cols, ordered)
        assert fn is _entry(("short", "deep")[k_cols > 64] + ("_ordered" if ordered else ""))
        np.testing.assert_allclose(fn(topk, ip, fl, ksd).cpu().numpy(), ref, rtol=RTOL, atol=0)
    if k_cols > 64:
        with pytest.raises(_lib.PdaHipError):
            ops.metrics_sums(topk, ip, fl, ksd)
        with pytest.raises(_lib.PdaHipError):
            ops.metrics_sums_ordered(topk, ip, fl, ksd)


def test_no_case_is_left_out():
    """The parametrised tests above run every k_cols of the table; this pins which entry points each of them calls."""
    assert [k for k in mr.K_COLS if entries(k) == ENTRIES] == list(mr.K_COLS_SHORT)
    assert [k for k in mr.K_COLS if entries(k) == ENTRIES[2:]] == list(mr.K_COLS_DEEP)
    assert entries(64) == ENTRIES and entries(65) == ("deep", "deep_ordered")
