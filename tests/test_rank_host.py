"""CPU suite for the ranks of held-out items (include/pda_hip_rank.h, `--rank_report`): the binding against its header, the entry points'
argument checks (all of them happen before any HIP call), the report's statistics on hand-made ranks, its per-group recall against the bias
report's on the lists the same ranks imply, the flags and the refusals of the command line."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from rank_ref import csr_of, lists_from, rank_ref
from test_abi import ROOT, declared_in

ERR_ARG, ERR_UNSUPPORTED = -1, -2
FNS = ["pda_rank_keys_f32", "pda_rank_keys_bf16", "pda_rank_count_f32", "pda_rank_count_bf16"]


def _buf(n_bytes=4096):
    """A host buffer: good enough for an argument that must only be non-null (every check happens before any HIP call)."""
    b = C.create_string_buffer(n_bytes)
    return b, C.c_void_p(C.addressof(b))


def test_binding_matches_the_header():
    from pda_amd import _lib
    assert declared_in("pda_hip_rank.h") == sorted(_lib.RANK_SIGNATURES) == sorted(FNS)
    text = open(os.path.join(ROOT, "include", "pda_hip_rank.h")).read()
    assert "#define PDA_RANK_TCHUNK %d" % _lib.RANK_TCHUNK in text
    # the twins take what the fp32 calls take
    assert _lib.RANK_SIGNATURES["pda_rank_keys_f32"] == _lib.RANK_SIGNATURES["pda_rank_keys_bf16"]
    assert _lib.RANK_SIGNATURES["pda_rank_count_f32"] == _lib.RANK_SIGNATURES["pda_rank_count_bf16"]


def test_every_symbol_is_exported():
    from pda_amd import _lib
    lib = _lib.load()
    for name in _lib.RANK_SIGNATURES:
        assert getattr(lib, name).argtypes == _lib.RANK_SIGNATURES[name][1], name
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if out.returncode == 0:
        exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
        assert set(_lib.RANK_SIGNATURES) <= exported


def test_no_overlap_with_the_other_surfaces():
    from pda_amd import _lib
    mine = set(_lib.RANK_SIGNATURES)
    assert not mine & set(_lib.SIGNATURES)
    for name in dir(_lib):
        if name.endswith("_SIGNATURES") and name != "RANK_SIGNATURES":
            assert not mine & set(getattr(_lib, name)), name
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "pda_hip_rank.h":
            assert not mine & set(declared_in(h)), h


def _keys(lib, b, fn, **kw):
    null = C.c_void_p(None)
    p = dict(U=b, I=b, pop=null, users=b, nu=300, off=0, nloc=5000, d=64, hp=null, hi=null, hm=0, tp=b, ti=b, head=0, keys=b)
    p.update(kw)
    return getattr(lib, fn)(p["U"], p["I"], p["pop"], p["users"], p["nu"], p["off"], p["nloc"], p["d"], p["hp"], p["hi"], p["hm"], p["tp"], p["ti"],
                            p["head"], p["keys"], null)


def _count(lib, b, fn, **kw):
    null = C.c_void_p(None)
    p = dict(U=b, I=b, pop=null, users=b, nu=300, off=0, nloc=5000, d=64, hp=null, hi=null, hm=0, tp=b, keys=b, max_row=10, head=0, splits=0,
             above=b, n_ranked=b)
    p.update(kw)
    return getattr(lib, fn)(p["U"], p["I"], p["pop"], p["users"], p["nu"], p["off"], p["nloc"], p["d"], p["hp"], p["hi"], p["hm"], p["tp"], p["keys"],
                            p["max_row"], p["head"], p["splits"], p["above"], p["n_ranked"], null)


@pytest.mark.parametrize("fn", FNS)
def test_argument_checks_without_gpu(fn):
    from pda_amd import _lib
    lib = _lib.load()
    keep, b = _buf()
    null = C.c_void_p(None)
    call = (lambda **kw: _keys(lib, b, fn, **kw)) if "keys" in fn else (lambda **kw: _count(lib, b, fn, **kw))
    assert call(U=null) == ERR_ARG and call(I=null) == ERR_ARG and call(users=null) == ERR_ARG and call(tp=null) == ERR_ARG
    assert call(d=48) == ERR_UNSUPPORTED and call(d=0) == ERR_UNSUPPORTED and call(d=512) == ERR_UNSUPPORTED
    assert call(nu=0) == ERR_ARG and call(nu=-3) == ERR_ARG
    assert call(nloc=0) == ERR_ARG and call(off=-1) == ERR_ARG
    assert call(head=2) == ERR_ARG
    assert call(head=1) == ERR_ARG                                # the popularity head without a popularity
    assert call(hp=b) == ERR_ARG                                  # a history without its indices
    assert call(hp=b, hi=b, hm=7) == ERR_ARG
    if "keys" in fn:
        assert call(ti=null) == ERR_ARG and call(keys=null) == ERR_ARG
    else:
        assert call(splits=-1) == ERR_ARG and call(above=null) == ERR_ARG and call(n_ranked=null) == ERR_ARG
        assert call(max_row=-1) == ERR_ARG and call(keys=null) == ERR_ARG
    del keep


def test_ops_refuses_bad_arguments_before_the_library():
    import torch
    from pda_amd import ops
    cpu = torch.zeros((4, 64))
    with pytest.raises((ValueError, TypeError)):
        ops.rank_targets(cpu, cpu, torch.zeros(4, dtype=torch.int32), torch.zeros(5, dtype=torch.int64), torch.zeros(0, dtype=torch.int32))
    assert ops.RANK_TCHUNK == 32


# ---- the report ---------------------------------------------------------------------------------------------------------------------------
def _stats(rank_rows, n_ranked, Ks=(1, 3), ids_rows=None, groups=None, n_groups=None):
    from pda_amd.rank_report import RankStats
    if ids_rows is None:                           # distinct ids per row
        ids_rows = [list(range(10 * r, 10 * r + len(x))) for r, x in enumerate(rank_rows)]
    tp, ids = csr_of(ids_rows)
    rank = np.concatenate([np.asarray(x, dtype=np.int64) for x in rank_rows]) if tp[-1] else np.zeros(0, np.int64)
    return RankStats(rank, n_ranked, tp, ids, list(Ks), groups, n_groups)


def test_auc_one_zero_and_a_half():
    s = _stats([[0, 1]], [10])                     # both targets in front of all 8 others
    assert s.auc == 1.0 and s.auc_users == 1 and s.auc_left_out == 0 and s.mrr == 1.0
    s = _stats([[8, 9]], [10])                     # both behind all others
    assert s.auc == 0.0 and s.mrr == pytest.approx(1.0 / 9.0)
    s = _stats([[2]], [5])                         # two in front, two behind
    assert s.auc == 0.5 and s.mpr == 0.5 and s.mean_rank == 2.0 and s.median_rank == 2.0
    s = _stats([[0, 9]], [10])                     # one wins all 8, one loses all 8
    assert s.auc == 0.5
    s = _stats([[0], [4]], [5, 5])                 # the mean over users
    assert s.auc == 0.5 and s.mrr == pytest.approx((1.0 + 0.2) / 2)


def test_a_user_without_negatives_is_left_out_and_counted():
    s = _stats([[0, 1], [0, 1, 2], []], [10, 3, 7])        # row 1: every ranking item is a target; row 2: no target
    assert s.auc == 1.0 and s.auc_users == 1 and s.auc_left_out == 2
    assert s.mrr == pytest.approx(2.0 / 3.0)               # rows 0 and 1 lead with a target, row 2 adds 0
    assert "left_out=2" in s.lines()[0] and s.lines()[0].startswith("||--- rank auc=1.000000 ")


def test_duplicates_count_once_and_minus_one_is_a_miss():
    dup = _stats([[3, 3, 5]], [10], ids_rows=[[7, 7, 9]])
    one = _stats([[3, 5]], [10], ids_rows=[[7, 9]])
    assert dup.auc == one.auc and dup.mpr == one.mpr and dup.mean_rank == one.mean_rank == 4.0 and dup.n_ranked_targets == 2
    # the metrics line's denominators: hits are distinct items, the row's length counts every entry
    assert dup.recall.tolist() == [0.0, 0.0] and _stats([[3, 3, 5]], [10], Ks=[4, 6], ids_rows=[[7, 7, 9]]).recall.tolist() == [1.0 / 3.0, 2.0 / 3.0]
    s = _stats([[-1, 0], [-1]], [10, 10], Ks=[1, 100000])
    assert s.n_ranked_targets == 1 and s.n_unranked_targets == 2
    assert s.recall.tolist() == [0.25, 0.25] and s.hit.tolist() == [0.5, 0.5]            # -1 never hits, at any K
    assert s.mrr == 0.5 and s.auc_users == 1 and s.auc_left_out == 1
    empty = _stats([[], []], [4, 4])
    assert empty.auc == 0.0 and empty.mrr == 0.0 and empty.mpr == 0.0 and empty.recall.tolist() == [0.0, 0.0] and empty.auc_left_out == 2


def test_rank_ks():
    from pda_amd.rank_report import rank_ks
    assert rank_ks("[50, 1000]") == [50, 1000] and rank_ks("[3000,5,5]") == [5, 3000] and rank_ks([7]) == [7]
    for bad in ("[]", "[0]", "[-5, 3]", "50", "[1.5]", "nonsense(", "[True]"):
        with pytest.raises(ValueError, match="rank_ks"):
            rank_ks(bad)


def test_group_recall_from_ranks_equals_the_bias_reports_on_the_implied_lists():
    from pda_amd.exposure import ExposureReport, item_groups
    rng = np.random.default_rng(11)
    nu, ni, G = 90, 400, 5
    vals = (rng.integers(-16, 17, (nu, ni)) / 8.0)                                 # many exact ties: the id rule decides
    hist = [rng.integers(0, ni, rng.integers(0, 30)) for _ in range(nu)]
    tgt = [np.unique(rng.integers(0, ni, rng.integers(0, 25))) for _ in range(nu)]
    tgt[3] = np.concatenate([tgt[3], hist[4][:2], hist[3][:3]])                    # targets inside the history never hit
    counts = rng.integers(0, 50, ni)
    groups = item_groups(counts, G, "interactions")
    rank, n = rank_ref(vals, hist, tgt)
    Ks = [5, 20, 50]
    from pda_amd.rank_report import RankStats
    tp, ids = csr_of(tgt)
    s = RankStats(rank, n, tp, ids, Ks, groups, G)
    lists = lists_from(vals, hist, 50)
    shown, hit = np.zeros((3, ni), np.int64), np.zeros((3, ni), np.int64)
    for q, K in enumerate(Ks):
        for r in range(nu):
            np.add.at(shown[q], lists[r, :K], 1)
            np.add.at(hit[q], lists[r, :K][np.isin(lists[r, :K], tgt[r])], 1)
    rep = ExposureReport(shown, hit, nu, Ks, counts, groups, np.zeros(ni), np.bincount(ids, minlength=ni), G)
    np.testing.assert_array_equal(s.group_recall, rep.group_recall)
    assert s.group_recall.max() > 0 and s.group_targets.sum() == ids.shape[0]
    # and the overall recall / hit are the metrics line's: per-user hits / row length, over all users
    for q, K in enumerate(Ks):
        per = [np.isin(lists[r, :K], tgt[r]).sum() / len(tgt[r]) if len(tgt[r]) else 0.0 for r in range(nu)]
        assert s.recall[q] == pytest.approx(np.mean(per), rel=1e-12)
        assert s.hit[q] == pytest.approx(np.mean([p > 0 for p in per]), rel=1e-12)
    assert len(s.lines()) == 1 + 3 + 1 + 3


# ---- the flags ----------------------------------------------------------------------------------------------------------------------------
def test_flags_and_refusals():
    from pda_amd.parse import parse_args, reference_flag_names
    from pda_amd.rank_report import check_rank_report
    a = parse_args([])
    assert a.rank_report == 0 and a.rank_ks == "[50, 1000]" and check_rank_report(a) is False
    assert "rank_report" not in reference_flag_names() and "rank_ks" not in reference_flag_names()
    assert check_rank_report(parse_args(["--rank_report", "1"])) is True
    assert check_rank_report(parse_args(["--rank_report", "1", "--deterministic", "1", "--rank_ks", "[5000]"])) is True
    assert check_rank_report(parse_args(["--rank_report", "1", "--train", "s_condition", "--test", "normal"])) is True
    assert check_rank_report(parse_args(["--train", "temp_pop"]), topk_shard=object()) is False          # off: nothing is looked at
    with pytest.raises(NotImplementedError, match="item shards"):
        check_rank_report(parse_args(["--rank_report", "1"]), topk_shard=object())
    for flags in (["--train", "temp_pop"], ["--test", "temp_pop"]):
        with pytest.raises(NotImplementedError, match="temp_pop"):
            check_rank_report(parse_args(["--rank_report", "1"] + flags))
    with pytest.raises(NotImplementedError, match="macr"):
        check_rank_report(parse_args(["--rank_report", "1", "--train", "macr", "--test", "macr"]))
    with pytest.raises(ValueError, match="rank_report"):
        check_rank_report(parse_args(["--rank_report", "2"]))
    with pytest.raises(ValueError, match="rank_ks"):
        check_rank_report(parse_args(["--rank_report", "1", "--rank_ks", "[0]"]))
    with pytest.raises(ValueError, match="bias_groups"):
        check_rank_report(parse_args(["--rank_report", "1", "--bias_groups", "65"]))


def test_main_refuses_before_anything_is_built(tmp_path):
    from pda_amd import synthetic
    from pda_amd import train_new_api as t
    toy = str(tmp_path / "data") + "/"
    synthetic.write_dataset(toy + "toy", n_users=60, n_items=40, mean_hist=6)
    base = ["--data_path", toy, "--dataset", "toy", "--save_dir", str(tmp_path / "save") + "/", "--rank_report", "1"]
    with pytest.raises(NotImplementedError, match="temp_pop"):
        t.main(base + ["--train", "temp_pop", "--test", "temp_pop"])
    with pytest.raises(NotImplementedError, match="macr"):
        t.main(base + ["--train", "macr", "--test", "macr"])
    # bpr_pc, xquad and export_topk do not take the flag
    from pda_amd import bpr_pc, export_topk, xquad
    for tool, extra in ((bpr_pc, []), (xquad, []), (export_topk, ["--export_out", str(tmp_path / "x.npz")])):
        with pytest.raises(NotImplementedError, match="does not take the flag"):
            tool.main(base + ["--train", "normal"] + extra)
    assert not os.path.exists(str(tmp_path / "save"))
    # the model wrapper and the evaluation refuse item shards
    from pda_amd.parse import parse_args
    from pda_amd.rank_report import RankReport
    with pytest.raises(NotImplementedError, match="item shards"):
        RankReport.from_args(parse_args(["--rank_report", "1"]), None, topk_shard=object())


def test_the_flag_at_zero_prints_no_rank_line():
    code = ("import io, contextlib, numpy as np\n"
            "from pda_amd.parse import parse_args\n"
            "from pda_amd.rank_report import RankReport\n"
            "from pda_amd import train_new_api as t\n"
            "a = parse_args([])\n"
            "assert RankReport.from_args(a, None) is None\n"
            "ev = t.evaluation(object(), [20, 50], 'cpu', block=8)\n"
            "assert ev.rank is None\n"
            "ret = {k: np.array([0.1, 0.2]) for k in ('recall', 'precision', 'hit_ratio', 'ndcg')}\n"
            "t._print_result(ret)\n"
            "from pda_amd.exposure import EvalResult\n"
            "r2 = EvalResult(ret); r2.rank_lines = ['||--- rank auc=0.5']\n"
            "print('----'); t._print_result(r2)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    off, on = r.stdout.split("----\n")
    assert off.count("\n") == 1 and "rank" not in off and off.startswith("||------")
    assert on.splitlines()[1:] == ["||--- rank auc=0.5"]
