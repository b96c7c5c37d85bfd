"""GPU: the item exposure of the lists (`--bias_report 1`, include/pda_hip_exposure.h) -- pda_list_exposure and pda_list_exposure_plain against
the numpy restatement of tests/exposure_ref.py, every count exactly, and the report end to end."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from exposure_ref import csr_of, exposure_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN = -(1 << 31)
KS8 = [5, 10, 20, 50, 100, 200, 500, 1024]


def run(dev, topk, Ks, n_items, tgt_rows=None, shown=None, hit=None, plain=False):
    """-> (shown, hit | None) as numpy, through ops.list_exposure."""
    from pda_amd import ops
    t = torch.from_numpy(np.ascontiguousarray(topk, dtype=np.int32)).to(dev)
    tp = ti = None
    if tgt_rows is not None:
        tp, ti = (torch.from_numpy(x).to(dev) for x in csr_of(tgt_rows))
    s, h = ops.list_exposure(t, Ks, n_items, tp, ti, shown, hit, plain=plain)
    assert s.dtype == torch.int32 and tuple(s.shape) == (len(Ks), n_items) and (h is None) == (tgt_rows is None)
    return s.cpu().numpy(), None if h is None else h.cpu().numpy()


def check(dev, topk, Ks, n_items, tgt_rows):
    """Both kernels, with and without targets, against the restatement; -> the reference counts."""
    want_s, want_h = exposure_ref(topk, Ks, n_items, tgt_rows)
    for plain in (False, True):
        s, h = run(dev, topk, Ks, n_items, tgt_rows, plain=plain)
        np.testing.assert_array_equal(s, want_s)
        np.testing.assert_array_equal(h, want_h)
        assert (h <= s).all()
        s0, _ = run(dev, topk, Ks, n_items, None, plain=plain)
        np.testing.assert_array_equal(s0, want_s)                    # targets absent: the same shown
    return want_s, want_h


def random_targets(rng, n_rows, n_items, longest=6):
    """Unsorted rows with duplicates, some of them empty."""
    return [rng.integers(0, n_items, rng.integers(0, longest + 1)) for _ in range(n_rows)]


@pytest.mark.parametrize("k_cols", [1, 50, 54, 64, 65, 1024])
def test_shapes(dev, k_cols):
    rng = np.random.default_rng(k_cols)
    ks_sets = [[1], [20, 50], KS8, [max(1, k_cols // 2), k_cols + 7]]
    case = 0
    for n_rows in (1, 3, 64, 65, 257):
        for Ks in ks_sets:
            n_items = (1, 7, 4097)[case % 3]
            case += 1
            topk = rng.integers(-1, n_items + 1, (n_rows, k_cols))      # (-1 and n_items: ignored)
            want_s, _ = check(dev, topk, Ks, n_items, random_targets(rng, n_rows, n_items))
            in_buckets = topk[:, :min(Ks[-1], k_cols)]
            assert want_s.sum() == ((in_buckets >= 0) & (in_buckets < n_items)).sum()


def test_contention_every_row_holds_the_same_ids(dev):
    ids = np.random.default_rng(1).permutation(70000)[:50]
    topk = np.tile(ids, (4096, 1))
    for plain in (False, True):
        s, h = run(dev, topk, [20, 50], 70000, [[ids[30], ids[0]]] * 4096, plain=plain)
        want = np.zeros((2, 70000), np.int64)
        want[0, ids[:20]] = 4096
        want[1, ids[20:]] = 4096
        np.testing.assert_array_equal(s, want)
        want[:] = 0
        want[0, ids[0]] = want[1, ids[30]] = 4096
        np.testing.assert_array_equal(h, want)


def test_more_distinct_ids_than_any_table_holds(dev):
    rng = np.random.default_rng(2)
    n_items = 70000
    topk = rng.integers(0, n_items, (4096, 50))
    topk[0, 0], topk[4095, 49], topk[17, 20] = 0, n_items - 1, n_items - 1
    assert np.unique(topk[:128]).size > 4096                          # 128 rows, the smallest slab of a workgroup, hold more than the largest table
    want_s, _ = check(dev, topk, [20, 50], n_items, [r[rng.integers(0, 50, 3)] for r in topk])
    assert want_s[0, 0] >= 1 and want_s[1, n_items - 1] >= 2


@pytest.mark.parametrize("modulus", [1024, 4096, 16384])
def test_ids_congruent_modulo_a_power_of_two(dev, modulus):
    rng = np.random.default_rng(modulus)
    n_items = 70000
    pool = np.arange(modulus - 1, n_items, modulus)
    topk = pool[rng.integers(0, pool.size, (512, 50))]
    check(dev, topk, [20, 50], n_items, [pool[rng.integers(0, pool.size, 2)] for _ in range(512)])


def test_invalid_ids_are_skipped_and_their_neighbours_counted(dev):
    n_items = 10
    topk = np.array([[3, -1, 4, n_items, I32_MIN, 5],
                     [-1, -1, -1, -1, -1, -1],
                     [n_items + 1, 9, (1 << 31) - 1, 0, -7, 9]], np.int64)
    tgt = [[5, 3, n_items, -1], [-1], [9]]
    want_s, want_h = check(dev, topk, [2, 6], n_items, tgt)
    assert want_s.tolist() == [[0, 0, 0, 1, 0, 0, 0, 0, 0, 1], [1, 0, 0, 0, 1, 1, 0, 0, 0, 1]]
    assert want_h.tolist() == [[0, 0, 0, 1, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 1, 0, 0, 0, 1]]
    # nothing else changes: the items beside the counted ones keep what the buffer held
    from pda_amd import ops
    shown = torch.full((2, n_items), 7, dtype=torch.int32, device=dev)
    hit = torch.full((2, n_items), 7, dtype=torch.int32, device=dev)
    for plain in (False, True):
        shown.fill_(7), hit.fill_(7)
        s, h = run(dev, topk, [2, 6], n_items, tgt, shown, hit, plain=plain)
        np.testing.assert_array_equal(s, want_s + 7)
        np.testing.assert_array_equal(h, want_h + 7)
    assert ops.list_exposure(shown.new_full((4, 3), -1), [3], n_items)[0].count_nonzero() == 0


def test_targets_empty_unsorted_duplicated_and_absent(dev):
    topk = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [1, 1, 2, 9], [0, 0, 0, 0]])
    tgt = [[], [8, 5, 5], [1], [3]]
    want_s, want_h = check(dev, topk, [2, 4], 10, tgt)
    h = np.zeros((2, 10), np.int64)
    h[0, 5] = 1                  # a duplicated target: one hit
    h[1, 8] = 1                  # an unsorted row
    h[0, 1] = 2                  # both entries that hold item 1 are in the row's targets: every column counts on its own
    np.testing.assert_array_equal(want_h, h)
    assert want_s[:, 0].tolist() == [2, 2]


def test_accumulation_into_one_buffer(dev):
    rng = np.random.default_rng(4)
    n_items, Ks = 500, [3, 20, 50]
    a, b = rng.integers(-1, n_items, (300, 50)), rng.integers(-1, n_items, (77, 50))
    ta, tb = random_targets(rng, 300, n_items), random_targets(rng, 77, n_items)
    (sa, ha), (sb, hb) = exposure_ref(a, Ks, n_items, ta), exposure_ref(b, Ks, n_items, tb)
    for plain in (False, True):
        shown = torch.full((3, n_items), 7, dtype=torch.int32, device=dev)
        hit = torch.zeros((3, n_items), dtype=torch.int32, device=dev)
        run(dev, a, Ks, n_items, ta, shown, hit, plain=plain)
        s, h = run(dev, b, Ks, n_items, tb, shown, hit, plain=plain)
        np.testing.assert_array_equal(s, sa + sb + 7)
        np.testing.assert_array_equal(h, ha + hb)


def test_hits_sum_to_the_hits_of_the_metrics(dev):
    from pda_amd import ops
    from pda_amd.exposure import cumulate
    rng = np.random.default_rng(6)
    n, n_items, Ks = 700, 900, [5, 20, 50]
    topk = np.argsort(rng.random((n, n_items)), axis=1)[:, :50]
    tgt = [np.unique(rng.integers(0, n_items, rng.integers(0, 30))) for _ in range(n)]
    _, h = run(dev, topk, Ks, n_items, tgt)
    member = np.stack([np.isin(topk[r], tgt[r]) for r in range(n)])
    want = [int(member[:, :k].sum()) for k in Ks]
    assert cumulate(h).sum(axis=1).tolist() == want and want[0] > 0
    tp, ti = (torch.from_numpy(x).to(dev) for x in csr_of(tgt))
    sums = ops.metrics_sums(torch.from_numpy(topk.astype(np.int32)).to(dev), tp, ti, torch.as_tensor(Ks, dtype=torch.int32, device=dev))
    np.testing.assert_allclose(sums[0].cpu().numpy() * np.asarray(Ks), want, rtol=1e-12)        # precision sums x K = hits


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
COMMON = ["--dataset", "toy", "--epoch", "1", "--log_interval", "1", "--batch_size", "256", "--lr", "1e-2", "--regs", "1e-2", "--valid_set", "valid",
          "--save_flag", "0", "--saveID", "t", "--cuda", "0", "--eval_block", "256", "--bias_groups", "5"]


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from pda_amd import synthetic
    base = tmp_path_factory.mktemp("exposure")
    synthetic.write_dataset(str(base / "data" / "toy"), n_users=600, n_items=400)
    return str(base / "data") + "/", str(base / "save") + "/"


def _cli(module, toy, extra):
    argv = [sys.executable, "-m", module, "--data_path", toy[0], "--save_dir", toy[1], *COMMON, *extra]
    r = subprocess.run(argv, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def _bias_blocks(lines, Ks):
    """Every metrics line is followed by one bias line per cut-off (the first also by the line that names the groups) -> the blocks."""
    blocks = []
    at = [i for i, l in enumerate(lines) if l.startswith("||------") and " recall=[" in l]
    assert at
    for n, i in enumerate(at):
        j = i + 1
        if n == 0:
            assert lines[j].startswith("||--- bias groups items=[") and lines[j].count(",") == 2 * 4
            j += 1
        blocks.append(lines[j:j + len(Ks)])
        assert [l.split()[1] for l in blocks[-1]] == ["bias@%d" % k for k in Ks], lines[i:j + len(Ks)]
        assert all("hit_share=[" in l and "group_recall=[" in l for l in blocks[-1])
    assert sum(l.startswith("||--- bias") for l in lines) == 1 + len(Ks) * len(at)
    return blocks


def test_eval_with_an_accumulator_and_its_report(dev, toy):
    from pda_amd import train_new_api as t
    from pda_amd.exposure import BiasReport, EvalResult, ExposureAccumulator, ExposureReport, cumulate
    from pda_amd.xquad import head_items, train_counts
    t.configure(["--data_path", toy[0], *COMMON, "--train", "normal", "--Ks", "[20,50]", "--deterministic", "1"])
    data = t.data
    torch.manual_seed(5)
    model = t.DatasetApi_Model(t.args, {"n_users": data.n_users, "n_items": data.n_items}, 256, None, dev)
    ev = t.evaluation(data, [20, 50], dev)
    ev.set_evaluate_obj_pre("test")
    assert ev.tot_user > 256                                          # more than one block
    plain = ev.eval(model, None, "main_branch")
    acc = ExposureAccumulator(data.n_items, [20, 50], dev)
    with_acc = ev.eval(model, None, "main_branch", exposure=acc)
    assert type(plain) is dict and type(with_acc) is dict and list(with_acc) == ["precision", "recall", "ndcg", "hit_ratio"]
    for key in plain:
        np.testing.assert_array_equal(with_acc[key], plain[key])
    assert acc.rows == ev.tot_user

    lists = model.do_recommendation(None, ev.users_dev, None, "main_branch", None, ev._hist)
    users = ev.users_dev.cpu().numpy()
    tgt_rows = [ev.eval_user_list[int(u)] for u in users]
    want_s, want_h = exposure_ref(lists, [20, 50], data.n_items, tgt_rows)
    np.testing.assert_array_equal(acc.shown.cpu().numpy(), want_s)
    np.testing.assert_array_equal(acc.hit.cpu().numpy(), want_h)
    counts = train_counts(data)
    bias = BiasReport(counts, [20, 50], 5, "interactions", 0.8)
    tgt_counts = np.bincount(np.concatenate(tgt_rows), minlength=data.n_items)
    want = ExposureReport(cumulate(want_s), cumulate(want_h), len(users), [20, 50], counts, bias.groups, head_items(counts, 0.8), tgt_counts, 5)
    got = bias.report(acc, ev._tgt_host)
    for field in ("rr", "hit_share", "group_recall", "arp", "coverage", "gini", "aplt", "train_share", "group_items"):
        np.testing.assert_array_equal(getattr(got, field), getattr(want, field))
    assert want.rr[0].sum() == pytest.approx(1.0) and want.group_recall.max() > 0 and 0 < want.coverage[0] <= 1 and want.gini[0] > 0

    # the evaluation object's own report (what --bias_report 1 sets): the same metrics, the lines beside them
    ev.set_bias_report(bias)
    ret = ev.eval(model, None, "main_branch")
    assert isinstance(ret, EvalResult) and list(ret) == list(plain) and ret.bias_lines == want.lines() and ret.bias is bias
    assert bias.header() == [want.group_line()] and bias.header() == []                # a run names its groups once
    for key in plain:
        np.testing.assert_array_equal(ret[key], plain[key])
    assert ev.eval(model, None, "main_branch").bias_lines == want.lines()
    ev.set_bias_report(None)
    assert type(ev.eval(model, None, "main_branch")) is dict


def test_cli_normal_head_and_xquad(dev, toy):
    flags = ["--train", "normal", "--test", "normal", "--Ks", "[20,50]", "--deterministic", "1"]
    on = _cli("pda_amd.train_new_api", toy, flags + ["--bias_report", "1"])
    _bias_blocks(on, [20, 50])
    # the flag at 0: the same lines without the bias lines (the timing lines aside)
    off = _cli("pda_amd.train_new_api", toy, flags)

    def steady(lines):
        return [l for l in lines if "time" not in l and not l.startswith("Epoch") and "bias_report" not in l]
    assert not any("bias@" in l or "bias groups" in l for l in off)
    assert steady(off) == [l for l in steady(on) if not l.startswith("||--- bias")]

    out = _cli("pda_amd.xquad", toy, flags + ["--bias_report", "1", "--xq_candidates", "100"])
    blocks = _bias_blocks(out, [20, 50])
    aplt = [re.search(r"aplt@\[20, 50\]=\[([\d.]+), ([\d.]+)\]", l).groups() for l in out if "aplt@[20, 50]=" in l]
    assert len(aplt) == len(blocks) == 4
    for block, own in zip(blocks, aplt):
        assert tuple(re.search(r" aplt=([\d.]+) ", l).group(1) for l in block) == own


@pytest.mark.parametrize("flags, Ks", [
    (["--train", "s_condition", "--test", "s_condition", "--Ks", "[20,50]"], [20, 50]),
    (["--train", "macr", "--test", "macr", "--step", "3", "--Ks", "[20,50]"], [20, 50]),
    (["--train", "temp_pop", "--test", "temp_pop", "--Ks", "[20,50]"], [20, 50]),
    (["--train", "normal", "--test", "normal", "--Ks", "[20,100,200]", "--topk_max", "100"], [20, 100]),
], ids=["s_condition", "macr", "temp_pop", "topk_max_100"])
def test_cli_prints_the_lines_for_every_head(dev, toy, flags, Ks):
    out = _cli("pda_amd.train_new_api", toy, flags + ["--bias_report", "1"])
    _bias_blocks(out, Ks)
    assert out[-1].strip() and any("training and testing end" in l for l in out)
