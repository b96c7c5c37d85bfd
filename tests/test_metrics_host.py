"""Host suite of the ranking metrics: the float64 restatement (tests/metrics_ref.py) against the reference's recorded vectors, the four host
statements of the metric against each other on the case table the GPU tests run (tests/test_gpu_metrics.py), and the host glue around the
kernels: the divisor of evaluate_on_device, the routing between the short and the deep kernels, the check of the cut-offs."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest

import metrics_ref as mr
from oracle import c_oracle
from oracle import pda_oracle as po
from pda_amd import used_metric

G = os.path.join(os.path.dirname(__file__), "golden")
KEYS = ("precision", "recall", "ndcg", "hit_ratio")        # mr.NAMES as the keys of get_performance
RTOL = 1e-12                                               # numpy's pairwise sums and the C loop against math.fsum of <= 1 024 discounts


def _golden():
    return json.load(open(os.path.join(G, "metrics.json")))


def test_the_table_holds_its_cases():
    mr.check_table()


def test_restatement_equals_every_reference_vector():
    cases = _golden()
    assert len(cases) >= 40 and {len(c["r"]) for c in cases} > {50}          # every list length, not only 50
    for c in cases:
        out = mr.row_metrics(c["r"], c["target"], c["Ks"])
        for m, k in enumerate(KEYS):
            if k == "ndcg":
                np.testing.assert_allclose(out[m], c["out"][k], rtol=RTOL, atol=0, err_msg=k)
            else:                                          # one division of small integers: the same bits
                assert out[m] == c["out"][k], (k, c)


def _host_rows(fn, lists, targets, ks):
    out = np.empty((len(lists), 4, len(ks)))
    for i, (r, t) in enumerate(zip(lists, targets)):
        one = fn(t, r, ks)
        for m, k in enumerate(KEYS):
            out[i, m] = one[k]
    return out


def _agree(got, ref, what):
    assert np.isfinite(got).all(), what
    for m in (0, 1, 3):
        np.testing.assert_array_equal(got[:, m], ref[:, m], err_msg="%s %s" % (what, mr.NAMES[m]))
    np.testing.assert_allclose(got[:, 2], ref[:, 2], rtol=RTOL, atol=0, err_msg="%s ndcg" % what)


@pytest.mark.parametrize("k_cols", mr.K_COLS)
def test_the_four_host_statements_agree_on_the_case_table(k_cols):
    """Row by row for the two get_performance, and through the C oracle's sums at every row count."""
    _, lists, targets = mr.matrix(k_cols)
    for which, ks in enumerate(mr.ks_lists(k_cols)):
        ref = mr.matrix_ref(k_cols, which)
        _agree(_host_rows(po.get_performance, lists, targets, ks), ref, "oracle.pda_oracle k_cols %d Ks %s" % (k_cols, ks))
        _agree(_host_rows(used_metric.get_performance, lists, targets, ks), ref, "pda_amd.used_metric k_cols %d Ks %s" % (k_cols, ks))
        for i in mr.single_rows(k_cols):                   # the C oracle row by row: a sum of one row is that row
            got = c_oracle.metrics(np.array([lists[i]], np.int32), *mr.csr_of([targets[i]]), ks)
            _agree(got[None], ref[i:i + 1], "oracle.c_oracle k_cols %d Ks %s row %d" % (k_cols, ks, i))
        for n in mr.ROW_COUNTS:
            got = c_oracle.metrics(np.array(lists[:n], np.int32), *mr.csr_of(targets[:n]), ks)
            assert np.isfinite(got).all()
            np.testing.assert_allclose(got, mr.fsum_rows(ref[:n]), rtol=RTOL, atol=0, err_msg="c_oracle k_cols %d n %d" % (k_cols, n))


def test_the_host_statements_agree_on_the_large_case():
    """65 541 rows: the C oracle on all of them, the two get_performance on the rows behind the first 257 (those are in the test above) in
    steps of 64."""
    _, lists, targets = mr.large_matrix()
    ks = mr.ks_lists(mr.LARGE_K_COLS)[0]
    ref = mr.large_ref()
    assert ref.shape == (mr.LARGE_ROWS, 4, len(ks))
    got = c_oracle.metrics(np.array(lists, np.int32), *mr.csr_of(targets), ks)
    np.testing.assert_allclose(got, mr.fsum_rows(ref), rtol=RTOL, atol=0)
    pick = list(range(max(mr.ROW_COUNTS), mr.LARGE_ROWS, 64))
    for fn in (po.get_performance, used_metric.get_performance):
        _agree(_host_rows(fn, [lists[i] for i in pick], [targets[i] for i in pick], ks), ref[pick], fn.__module__)


@pytest.mark.parametrize("fn", [po.get_performance, used_metric.get_performance, None], ids=["oracle_py", "product_host", "oracle_c"])
def test_the_two_decisions_by_hand(fn):
    """K beyond the list: cut to the list's length, in the ideal DCG too.  No targets: zeros.  Figures worked out by hand."""
    def one(r, t, ks):
        if fn is None:
            return c_oracle.metrics(np.array([r], np.int32), *mr.csr_of([t]), ks)
        out = fn(t, r, ks)
        return np.array([out[k] for k in KEYS])
    w = [1.0, 1.0 / np.log2(3.0), 0.5]
    # three columns, hits in columns 0 and 2, five targets, K = 7 > 3: precision 2/3 (not 2/7), ideal DCG over 3 (not 5) discounts
    got = one([4, 9, 6], [6, 4, 100, 101, 102], [7, 3])
    assert got[0, 0] == got[0, 1] == 2 / 3 and got[1, 0] == 2 / 5 and got[3, 0] == 1.0
    np.testing.assert_allclose(got[2], [(w[0] + w[2]) / (w[0] + w[1] + w[2])] * 2, rtol=RTOL)
    for ref_row in (mr.row_metrics([4, 9, 6], [6, 4, 100, 101, 102], [7, 3]),):
        np.testing.assert_allclose(got, ref_row, rtol=RTOL)
    # no targets: zeros, no NaN, also next to a row that has some
    got = one([4, 9, 6], [], [1, 2, 7])
    assert got.shape == (4, 3) and (got == 0.0).all()
    if fn is None:
        both = c_oracle.metrics(np.array([[4, 9, 6], [4, 9, 6]], np.int32), *mr.csr_of([[], [9]]), [1, 2, 7])
        np.testing.assert_array_equal(both, np.array(mr.row_metrics([4, 9, 6], [9], [1, 2, 7])))


# ---------------------------------------------------------------------------------------------------------------- the glue around the kernels
class _Sums:
    def __init__(self, a):
        self.a = a

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def test_evaluate_on_device_divides_by_tot_user_or_by_the_rows(monkeypatch):
    from pda_amd import ops
    sums = np.arange(1.0, 9.0).reshape(4, 2)
    seen = []

    def fake(topk, tgt_indptr, tgt_indices, ks):
        seen.append(ks.tolist())
        return _Sums(sums)

    monkeypatch.setattr(ops, "metrics_sums", fake)
    topk = types.SimpleNamespace(shape=(8, 50), device="cpu")
    for tot, div in ((None, 8.0), (20, 20.0), (3, 3.0)):
        out = used_metric.evaluate_on_device(topk, None, None, [20, 50], tot_user=tot)
        for m, k in enumerate(KEYS):
            np.testing.assert_array_equal(out[k], sums[m] / div)
    assert seen == [[20, 50]] * 3


def test_routing_sends_64_columns_to_the_short_kernel_and_65_to_the_deep_one():
    from pda_amd import _lib, ops
    assert _lib.MAX_K == mr.SHORT_MAX == 64
    for k_cols in range(1, 65):
        assert ops.metrics_route(k_cols) is ops.metrics_sums and ops.metrics_route(k_cols, ordered=True) is ops.metrics_sums_ordered
    for k_cols in (65, 66, 100, 1024):
        assert ops.metrics_route(k_cols) is ops.metrics_sums_deep and ops.metrics_route(k_cols, ordered=True) is ops.metrics_sums_deep_ordered
    # the short kernels' own limit is the routing constant: one more column is refused before anything is launched
    lib = _lib.load()
    keep = (C.c_char * 4096)()
    b, null = C.c_void_p(C.addressof(keep)), C.c_void_p(None)
    assert lib.pda_metrics(b, 10, _lib.MAX_K + 1, b, b, b, 2, b, null) == -1
    assert lib.pda_metrics_ordered(b, 10, _lib.MAX_K + 1, b, b, b, 2, b, b, null) == -1
    assert lib.pda_metrics_deep(b, 10, ops.DEEP_MAX_K + 1, b, b, b, 2, b, null, null) == -1


def test_the_trainer_routes_through_metrics_route():
    import inspect
    from pda_amd import train_new_api as t
    src = inspect.getsource(t.evaluation.eval)
    assert "ops.metrics_route(idx.shape[1]" in src and "metrics_sums" not in src


@pytest.mark.parametrize("bad", [[0], [20, 0], [-1, 5], [], [2.5], [20, 50.5]])
def test_cut_offs_below_one_are_refused_on_the_host(bad, monkeypatch):
    from pda_amd import ops
    from pda_amd import train_new_api as t
    monkeypatch.setattr(ops, "metrics_sums", lambda *a, **k: pytest.fail("the kernel must not be reached"))
    with pytest.raises(ValueError, match="Ks must be"):
        used_metric.check_ks(bad)
    with pytest.raises(ValueError, match="Ks must be"):
        used_metric.evaluate_on_device(types.SimpleNamespace(shape=(8, 50), device="cpu"), None, None, bad)
    with pytest.raises(ValueError, match="Ks must be"):
        t.evaluation(object(), bad, "cpu", block=8)
    with pytest.raises(ValueError, match="Ks must be"):
        used_metric.get_performance([1], [1, 2], bad)


def test_cut_offs_that_are_fine_pass_unchanged():
    from pda_amd import train_new_api as t
    assert used_metric.check_ks([20, 50]) == [20, 50] and used_metric.check_ks((50, 1, 50)) == [50, 1, 50]
    assert used_metric.check_ks(np.array([5, 70])) == [5, 70] and all(type(k) is int for k in used_metric.check_ks(np.array([5, 70])))
    assert t.evaluation(object(), [50, 1, 50], "cpu", block=8).Ks == [50, 1, 50]
