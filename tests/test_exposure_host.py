"""CPU suite for the bias report (`--bias_report 1`, pda_amd/exposure.py, include/pda_hip_exposure.h): the popularity groups, the statistics on
hand-computed counts, APLT against xquad.aplt, the flags, and the argument checks of pda_list_exposure without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from exposure_ref import exposure_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = [5, 0, 3, 3, 1, 0, 8]


# ---- item_groups ----------------------------------------------------------------------------------------------------------------------------
def test_the_hand_cases_of_both_modes():
    from pda_amd.exposure import item_groups
    g = item_groups(HAND, 4, "items")
    assert g.dtype == np.int64 and g.tolist() == [0, 2, 1, 1, 2, 3, 0]
    assert item_groups(HAND, 4, "interactions").tolist() == [1, 3, 2, 3, 3, 3, 0]
    assert item_groups(HAND, 4).tolist() == [1, 3, 2, 3, 3, 3, 0]                    # the default mode


def test_ties_go_to_the_smaller_id_and_the_order_is_that_of_head_items():
    from pda_amd.exposure import item_groups, popularity_order
    from pda_amd.xquad import head_items
    assert item_groups([2, 2, 2, 2], 2, "items").tolist() == [0, 0, 1, 1]
    assert item_groups([2, 2, 2, 2], 4, "interactions").tolist() == [0, 1, 2, 3]
    assert item_groups([1, 7, 7, 1], 2, "items").tolist() == [1, 0, 0, 1]
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 6, 200)
    order = popularity_order(counts)
    assert (np.diff(counts[order]) <= 0).all()
    assert all(a < b for a, b in zip(order[:-1], order[1:]) if counts[a] == counts[b])
    head = head_items(counts, 0.5)
    assert head[order[:int(head.sum())]].all()                                       # the head is a prefix of the same order
    for by in ("items", "interactions"):
        assert (np.diff(item_groups(counts, 7, by)[order]) >= 0).all()               # groups do not decrease along it


def test_one_group_more_groups_than_items_and_empty_groups():
    from pda_amd.exposure import item_groups
    for by in ("items", "interactions"):
        assert item_groups(HAND, 1, by).tolist() == [0] * 7
    assert item_groups([3, 9, 1], 64, "items").tolist() == [21, 0, 42]               # (p 64) // 3
    g = item_groups([3, 9, 1], 8, "interactions")                                    # cum_before 0, 9, 12 of 13
    assert g.tolist() == [5, 0, 7] and set(range(8)) - set(g.tolist())               # groups 1 .. 4 and 6 are empty
    assert item_groups([0, 0, 4], 3, "interactions").tolist() == [2, 2, 0]           # items without a train entry: the last group
    sizes = np.bincount(item_groups(np.arange(1000)[::-1], 10, "items"), minlength=10)
    assert sizes.tolist() == [100] * 10


def test_equal_interaction_groups_on_a_zipf_catalogue():
    from pda_amd.exposure import item_groups
    counts = (1e6 / np.arange(1, 5001)).astype(np.int64)
    g = item_groups(counts, 10, "interactions")
    per = np.bincount(g, weights=counts, minlength=10) / counts.sum()
    sizes = np.bincount(g, minlength=10)
    assert (np.diff(sizes) >= 0).all() and sizes[0] == 1 and sizes.sum() == 5000
    assert abs(per[3:] - 0.1).max() < 0.02 and abs(per.sum() - 1.0) < 1e-12          # flat behind the few most popular items


def test_item_groups_refusals():
    from pda_amd.exposure import item_groups
    for G in (0, 65, -1, 2.5):
        with pytest.raises(ValueError, match="number of groups"):
            item_groups(HAND, G)
    with pytest.raises(ValueError, match="grouped by"):
        item_groups(HAND, 4, "users")
    with pytest.raises(ValueError, match="without interactions"):
        item_groups([0, 0, 0], 2, "interactions")
    assert item_groups([0, 0, 0], 3, "items").tolist() == [0, 1, 2]
    with pytest.raises(ValueError, match=">= 0"):
        item_groups([1, -1], 2)
    with pytest.raises(ValueError, match="empty catalogue"):
        item_groups([], 2)


# ---- the statistics --------------------------------------------------------------------------------------------------------------------------
def test_gini_on_hand_counts():
    from pda_amd.exposure import gini
    assert gini([0, 0, 0, 4]) == 0.75 and gini([1, 2, 3, 4]) == 0.25 and gini([1, 1, 1, 1]) == 0.0
    assert gini([0, 0, 0]) == 0.0 and gini([4, 0, 0, 0]) == 0.75 and gini([7]) == 0.0


def test_report_on_hand_counts():
    from pda_amd.exposure import ExposureReport, cumulate
    counts, groups, head = [10, 5, 3, 2], [0, 0, 1, 1], [1, 1, 0, 0]
    shown = cumulate([[3, 0, 0, 0], [0, 2, 0, 1]])
    hit = cumulate([[1, 0, 0, 0], [0, 1, 0, 1]])
    assert shown.tolist() == [[3, 0, 0, 0], [3, 2, 0, 1]]
    rep = ExposureReport(shown, hit, 3, [1, 2], counts, groups, head, tgt_counts=[2, 1, 0, 1])
    assert rep.group_items.tolist() == [2, 2] and rep.train_share.tolist() == [0.75, 0.25]
    np.testing.assert_array_equal(rep.rr, [[1.0, 0.0], [5.0 / 6.0, 1.0 / 6.0]])
    np.testing.assert_array_equal(rep.arp, [10.0, 7.0])
    np.testing.assert_array_equal(rep.coverage, [0.25, 0.75])
    np.testing.assert_array_equal(rep.gini, [0.75, 10.0 / 24.0])
    np.testing.assert_array_equal(rep.aplt, [0.0, (1.0 / 2.0) / 3.0])
    np.testing.assert_array_equal(rep.hit_share, [[1.0, 0.0], [2.0 / 3.0, 1.0 / 3.0]])
    np.testing.assert_array_equal(rep.group_recall, [[1.0 / 3.0, 0.0], [2.0 / 3.0, 1.0]])
    lines = rep.lines()
    assert len(lines) == 2 and lines[0].startswith("||--- bias@1 arp=10.00 cov=0.25000 gini=0.75000 aplt=0.00000 rr=[1.0000,0.0000] hit_share=")
    assert "group_recall=[0.6667,1.0000]" in lines[1] and rep.group_line() == "||--- bias groups items=[2,2] train_share=[0.7500,0.2500]"


def test_report_of_nothing_shown_groups_without_targets_and_lists_without_targets():
    from pda_amd.exposure import ExposureReport
    z = np.zeros((1, 4), np.int64)
    rep = ExposureReport(z, z, 0, [5], [1, 1, 1, 1], [0, 0, 1, 2], [1, 0, 0, 0], tgt_counts=[0, 0, 0, 0], n_groups=4)
    assert rep.n_groups == 4 and rep.group_items.tolist() == [2, 1, 1, 0]
    for v in (rep.rr, rep.hit_share, rep.group_recall, rep.arp, rep.coverage, rep.gini, rep.aplt):
        assert not v.any()
    rep = ExposureReport([[2, 0, 1, 0]], [[1, 0, 1, 0]], 2, [5], [1, 1, 1, 1], [0, 0, 1, 2], [1, 0, 0, 0], tgt_counts=[4, 0, 0, 9], n_groups=3)
    assert rep.group_recall.tolist() == [[0.25, 0.0, 0.0]]                           # group 1: hits without targets stay 0, group 2: no hits
    rep = ExposureReport([[2, 0, 1, 0]], None, 2, [5], [1, 1, 1, 1], [0, 0, 1, 2], [1, 0, 0, 0])
    assert not rep.has_hits and not hasattr(rep, "hit_share") and "hit_share" not in rep.lines()[0]
    with pytest.raises(ValueError):
        ExposureReport([[1, 2]], None, 1, [5], [1, 1, 1], [0, 0, 0], [0, 0, 0])
    with pytest.raises(ValueError):
        ExposureReport([[1, 2, 3]], [[1, 1, 1]], 1, [5], [1, 1, 1], [0, 0, 0], [0, 0, 0])   # hits without target counts


def test_aplt_is_the_expression_of_xquad_aplt():
    from pda_amd.exposure import ExposureReport, cumulate
    from pda_amd.xquad import aplt, head_items
    rng = np.random.default_rng(11)
    n_items, Ks = 300, [5, 20, 50]
    counts = rng.integers(0, 50, n_items)
    head = head_items(counts, 0.6)
    idx = np.argsort(rng.random((137, n_items)), axis=1)[:, :50].astype(np.int32)
    idx[rng.random(idx.shape) < 0.2] = -1
    idx[5] = -1
    shown, _ = exposure_ref(idx, Ks, n_items)
    rep = ExposureReport(cumulate(shown), None, idx.shape[0], Ks, counts, np.zeros(n_items, np.int64), head)
    want = aplt(torch.from_numpy(idx), torch.from_numpy(head), Ks)
    assert want.min() > 0
    np.testing.assert_array_equal(rep.aplt, want)


# ---- flags -------------------------------------------------------------------------------------------------------------------------------------
def test_parser_defaults_and_flag_checks():
    from pda_amd import exposure
    from pda_amd.parse import parse_args
    a = parse_args([])
    assert (a.bias_report, a.bias_groups, a.bias_group_by) == (0, 10, "interactions")
    assert exposure.check_flags(a) is False and exposure.BiasReport.from_args(a, None, [20]) is None
    a = parse_args(["--bias_report", "1", "--bias_groups", "4", "--bias_group_by", "items"])
    assert (a.bias_report, a.bias_groups, a.bias_group_by) == (1, 4, "items") and exposure.check_flags(a) is True
    with pytest.raises(NotImplementedError, match="one GPU"):
        exposure.check_flags(a, topk_shard=object())
    assert exposure.check_flags(parse_args([]), topk_shard=object()) is False          # flag 0: nothing is refused
    for bad in (["--bias_report", "2"], ["--bias_report", "1", "--bias_groups", "0"], ["--bias_report", "1", "--bias_groups", "65"],
                ["--bias_report", "1", "--bias_group_by", "users"], ["--bias_report", "1", "--xq_head_share", "1.0"]):
        with pytest.raises(ValueError):
            exposure.check_flags(parse_args(bad))
    assert exposure.report_ks([50, 20, 100, 20], 54) == [20, 50]
    with pytest.raises(ValueError, match="no cut-off"):
        exposure.report_ks([100], 50)


def test_bias_report_of_a_dataset():
    from pda_amd.exposure import BiasReport
    from pda_amd.xquad import head_items
    b = BiasReport(HAND, [20, 50], 4, "interactions", 0.8)
    assert b.groups.tolist() == [1, 3, 2, 3, 3, 3, 0] and b.is_head.tolist() == head_items(HAND, 0.8).tolist() and b.n_items == 7
    assert b.header() == ["||--- bias groups items=[1,1,1,4] train_share=[0.4000,0.2500,0.1500,0.2000]"] and b.header() == []   # once per run


def test_the_evaluation_refuses_item_shards_before_it_ranks():
    from pda_amd import train_new_api as t

    class Sharded:
        _shard = object()

        def recommend_device(self, *a, **k):
            raise AssertionError("the refusal comes first")

    class Wrapped:
        model = Sharded()
        recommend_device = Sharded.recommend_device

    ev = t.evaluation(data_=object(), Ks_=[20], device="cpu", block=4)
    for m in (Sharded(), Wrapped()):
        with pytest.raises(NotImplementedError, match="item-sharded"):
            ev.eval(m, None, "main_branch", exposure=object())


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_is_the_header():
    from pda_amd import _lib
    from test_abi import declared_in
    names = declared_in("pda_hip_exposure.h")
    assert names == ["pda_list_exposure", "pda_list_exposure_plain"] == sorted(_lib.EXPOSURE_SIGNATURES)
    assert not set(names) & (set(_lib.SIGNATURES) | set(declared_in("pda_hip.h")) | set(declared_in("pda_hip_experimental.h")))
    text = open(os.path.join(ROOT, "include", "pda_hip_exposure.h")).read()
    assert int(re.search(r"#define PDA_EXPOSURE_MAX_KS (\d+)", text).group(1)) == _lib.EXPOSURE_MAX_KS == 8
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n)


@pytest.mark.parametrize("name", ["pda_list_exposure", "pda_list_exposure_plain"])
def test_argument_checks_without_gpu(name):
    from pda_amd import _lib
    fn = getattr(_lib.load(), name)
    null, p = C.c_void_p(None), C.c_void_p(4096)          # (never read: every check comes before the launch)
    ok = dict(topk=p, n_rows=4, k_cols=50, n_items=9, tptr=p, tidx=p, Ks=p, n_ks=2, shown=p, hit=p)

    def call(**kw):
        a = dict(ok, **kw)
        return fn(a["topk"], a["n_rows"], a["k_cols"], a["n_items"], a["tptr"], a["tidx"], a["Ks"], a["n_ks"], a["shown"], a["hit"], null)

    # some but not all of the three target arguments
    for bad in (dict(tptr=null), dict(tidx=null), dict(hit=null), dict(tptr=null, tidx=null), dict(tptr=null, hit=null), dict(tidx=null, hit=null)):
        assert call(**bad) == -1, bad
    # the rest, with targets and without
    no_targets = dict(tptr=null, tidx=null, hit=null)
    for bad in (dict(topk=null), dict(Ks=null), dict(shown=null), dict(n_rows=0), dict(n_rows=-1), dict(n_items=0), dict(n_items=-5),
                dict(k_cols=0), dict(k_cols=1025), dict(k_cols=-1), dict(n_ks=0), dict(n_ks=9), dict(n_ks=-1)):
        assert call(**bad) == -1, bad
        assert call(**no_targets, **bad) == -1, bad


def test_ops_checks_the_cut_offs_and_the_tensors():
    from pda_amd import ops
    assert ops.exposure_ks([1]) == (1,) and ops.exposure_ks([5, 10, 20, 50, 100, 200, 500, 1024]) == (5, 10, 20, 50, 100, 200, 500, 1024)
    for bad in ([], [0, 5], [5, 5], [20, 10], [-1], list(range(1, 10)), [2.5], [1 << 31]):
        with pytest.raises(ValueError):
            ops.exposure_ks(bad)
    with pytest.raises(ValueError, match="HBM"):
        ops.list_exposure(torch.zeros((2, 3), dtype=torch.int32), [2], 5)
