"""GPU suite of the rank calls (pda_rank_keys_*, pda_rank_count_*, ops.rank_targets, --rank_report) -- every comparison on integers or bit
patterns, no tolerance.  The references are not the code under test: pda_score_dense_f32 (the dense matrix fed to tests/rank_ref.py),
float64 numpy products, and the lists of recommend_topk_deep / recommend_topk.  Inputs come from test_gpu_score_topk.make_case (exact-zero
popularities, duplicate history entries, 173 of 300 users picked unsorted)."""
import functools
import re

import numpy as np
import pytest
import torch

from rank_ref import csr_of, rank_ref
from test_gpu_score_topk import csr, make_case

pytestmark = pytest.mark.gpu

NU, NPICK = 300, 173
DS = [32, 64, 128, 256]
NIS = [1999, 5000]


def target_rows(rng, users, hist, nI, tchunk, nan_item):
    """Rows of length 0, 1, 7, one chunk, two chunks + 5, a duplicated entry, a target inside the history, the item with a NaN popularity, ids at
    and behind the catalogue's end; the rest short and random (unsorted, now and then with a repeat)."""
    rows = [rng.integers(0, nI, rng.integers(0, 13)).astype(np.int32) for _ in users]
    rows[0] = np.zeros(0, np.int32)
    rows[1] = rng.integers(0, nI, 1).astype(np.int32)
    rows[2] = rng.permutation(nI)[:7].astype(np.int32)
    rows[3] = rng.permutation(nI)[:tchunk].astype(np.int32)
    rows[4] = rng.permutation(nI)[:2 * tchunk + 5].astype(np.int32)
    rows[5] = np.array([17, 400, 17, 3, 400], np.int32)
    with_hist = [r for r, u in enumerate(users) if len(hist[u]) >= 2 and r > 8]
    for r in with_hist[:5]:
        rows[r] = np.concatenate([rows[r], hist[users[r]][:2]]).astype(np.int32)
    rows[6] = np.array([nan_item, 5, nan_item + 1], np.int32)
    rows[7] = np.array([nI, 9, nI + 5, nI - 1, 0], np.int32)
    rows[8] = np.concatenate([rng.permutation(nI)[:tchunk + 1], [nan_item]]).astype(np.int32)
    rows[NPICK - 1] = rng.permutation(nI)[:tchunk + 9].astype(np.int32)          # the last row of the block, behind a full tile
    return rows


@functools.lru_cache(maxsize=None)
def case(d, nI):
    from pda_amd import ops
    rng = np.random.default_rng(77 * d + nI)
    U, I, pop, hist = make_case(rng, NU, nI, d)
    nan_item = 123
    pop[nan_item] = np.nan
    users = rng.choice(NU, NPICK, replace=False).astype(np.int32)
    tgt = target_rows(rng, users, hist, nI, ops.RANK_TCHUNK, nan_item)
    return U, I, pop, hist, users, tgt


@functools.lru_cache(maxsize=None)
def dense(d, nI, head):
    """The dense kernel's matrix of the case (the parent commit's ops.score_dense), computed once per (d, nI, head)."""
    from pda_amd import ops
    U, I, pop, hist, users, tgt = case(d, nI)
    dev = torch.device("cuda:0")
    sd = ops.score_dense(torch.from_numpy(U).to(dev), torch.from_numpy(I).to(dev), torch.from_numpy(users).to(dev), head,
                         torch.from_numpy(pop).to(dev) if head else None)
    return sd.cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference(d, nI, head):
    U, I, pop, hist, users, tgt = case(d, nI)
    return rank_ref(dense(d, nI, head), [hist[u] for u in users], tgt)


def on_dev(dev, U, I, pop, users, hist_rows, by_user, tgt, off=0, nloc=None, bf16=False):
    from pda_amd import ops
    nloc = I.shape[0] - off if nloc is None else nloc
    Ut, Ish = torch.from_numpy(U).to(dev), torch.from_numpy(I[off:off + nloc].copy()).to(dev)
    if bf16:
        Ut, Ish = Ut.bfloat16(), Ish.bfloat16()
    popsh = None if pop is None else torch.from_numpy(pop[off:off + nloc].copy()).to(dev)
    h = None
    if hist_rows is not None:
        ip, ix = csr(hist_rows)
        h = ops.HistoryCSR(torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev), by_user=by_user)
    tp, ti = (torch.from_numpy(x).to(dev) for x in csr_of(tgt))
    return Ut, Ish, torch.from_numpy(users).to(dev), tp, ti, popsh, h


def unpack(keys):
    k = keys.astype(np.int64).view(np.uint64)
    hi = (k >> np.uint64(32)).astype(np.uint32)
    bits = np.where(hi & np.uint32(0x80000000), hi ^ np.uint32(0x80000000), ~hi)
    return bits, (np.uint32(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF)).astype(np.uint32)).astype(np.int64)


# ---- 1. keys ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("head", [0, 1])
def test_keys_are_the_dense_kernels_bits(dev, d, head):
    from pda_amd import ops
    nI = 5000
    U, I, pop, hist, users, tgt = case(d, nI)
    sd = dense(d, nI, head)
    want, _ = reference(d, nI, head)
    tp, ids = csr_of(tgt)
    row = np.repeat(np.arange(NPICK), np.diff(tp))
    Ut, It, ut, tpt, tit, popt, h = on_dev(dev, U, I, pop if head else None, users, hist, True, tgt)
    keys = ops.rank_keys(Ut, It, ut, tpt, tit, head, popt, h).cpu().numpy()
    np.testing.assert_array_equal(keys != 0, want >= 0)
    nz = keys != 0
    bits, item = unpack(keys[nz])
    np.testing.assert_array_equal(item, ids[nz])
    at = sd[row[nz], ids[nz]] + np.float32(0)                                      # (-0.0 is +0.0 in a key)
    np.testing.assert_array_equal(bits, at.view(np.uint32))
    h6 = set(hist[users[6]].tolist())                                               # the NaN popularity ranks under the raw head only
    assert (want[tp[6]:tp[7]] >= 0).tolist() == [head == 0 and 123 not in h6, 5 not in h6, 124 not in h6]

    # an offset shard: entries outside it keep what the buffer held
    off, nloc = 1700, 2901
    Ut, Ish, ut, tpt, tit, popt, h = on_dev(dev, U, I, pop if head else None, users, hist, True, tgt, off, nloc)
    out = torch.full((ids.shape[0],), 0x5A5A5A5A5A, dtype=torch.int64, device=dev)
    got = ops.rank_keys(Ut, Ish, ut, tpt, tit, head, popt, h, item_offset=off, out=out).cpu().numpy()
    inside = (ids >= off) & (ids < off + nloc)
    assert inside.any() and (~inside).any()
    np.testing.assert_array_equal(got[~inside], 0x5A5A5A5A5A)
    np.testing.assert_array_equal(got[inside], keys[inside])                        # a key does not depend on the shard it is taken in


# ---- 2. ranks against the dense kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("nI", NIS)
@pytest.mark.parametrize("head", [0, 1])
def test_ranks_equal_the_reference_on_the_dense_matrix(dev, d, nI, head):
    from pda_amd import ops
    U, I, pop, hist, users, tgt = case(d, nI)
    want_rank, want_n = reference(d, nI, head)
    assert (want_rank >= 0).sum() > 1000 and (want_rank < 0).sum() >= 10
    blk = [hist[u] for u in users]
    for by_user in (True, False):
        Ut, It, ut, tpt, tit, popt, h = on_dev(dev, U, I, pop if head else None, users, hist if by_user else blk, by_user, tgt)
        rank, n = ops.rank_targets(Ut, It, ut, tpt, tit, head, popt, h)
        assert rank.dtype == torch.int32 and n.dtype == torch.int32
        np.testing.assert_array_equal(n.cpu().numpy(), want_n)
        np.testing.assert_array_equal(rank.cpu().numpy(), want_rank)


def test_no_history_and_no_target(dev):
    from pda_amd import ops
    d, nI = 64, 1999
    U, I, pop, hist, users, tgt = case(d, nI)
    want_rank, want_n = rank_ref(dense(d, nI, 0), None, tgt)
    Ut, It, ut, tpt, tit, _, _ = on_dev(dev, U, I, None, users, None, True, tgt)
    rank, n = ops.rank_targets(Ut, It, ut, tpt, tit)
    np.testing.assert_array_equal(rank.cpu().numpy(), want_rank)
    np.testing.assert_array_equal(n.cpu().numpy(), want_n)
    assert (want_n == nI).all()
    empty = [np.zeros(0, np.int32)] * NPICK                                         # no entry at all: the lengths alone
    Ut, It, ut, tpt, tit, _, h = on_dev(dev, U, I, None, users, hist, True, empty)
    rank, n = ops.rank_targets(Ut, It, ut, tpt, tit, hist=h)
    assert rank.numel() == 0
    np.testing.assert_array_equal(n.cpu().numpy(), reference(d, nI, 0)[1])


# ---- 3. ranks against float64, independent of any kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("nI", NIS)
def test_exact_tables_against_float64(dev, d, nI):
    from pda_amd import ops
    rng = np.random.default_rng(5 * d + nI)
    U = (rng.integers(-16, 17, (NU, d)) / 8.0).astype(np.float32)                   # every product and every sum is exact in fp32
    I = (rng.integers(-16, 17, (nI, d)) / 8.0).astype(np.float32)
    I[1::7] = I[0]                                                                  # many items with one score per user: the id rule
    _, _, _, hist, users, tgt = case(d, nI)
    blk = [hist[u] for u in users]
    vals = U[users].astype(np.float64) @ I.astype(np.float64).T
    want_rank, want_n = rank_ref(vals, blk, tgt)
    Ut, It, ut, tpt, tit, _, h = on_dev(dev, U, I, None, users, blk, False, tgt)
    rank, n = ops.rank_targets(Ut, It, ut, tpt, tit, hist=h)
    np.testing.assert_array_equal(n.cpu().numpy(), want_n)
    np.testing.assert_array_equal(rank.cpu().numpy(), want_rank)


# ---- 4. against the lists -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,nI,head", [(32, 1999, 0), (64, 5000, 1), (128, 1999, 1), (256, 5000, 0)])
def test_ranks_agree_with_the_lists(dev, d, nI, head):
    from pda_amd import ops
    U, I, pop, hist, users, tgt = case(d, nI)
    K = min(1024, nI - max(len(hist[u]) for u in users) - 1)                        # (- 1: the item with the NaN popularity)
    Ut, It, ut, tpt, tit, popt, h = on_dev(dev, U, I, pop if head else None, users, hist, True, tgt)
    rank, _ = ops.rank_targets(Ut, It, ut, tpt, tit, head, popt, h)
    rank = rank.cpu().numpy()
    idx, _ = ops.recommend_topk_deep(Ut, It, ut, K, head, popt, h)
    idx = idx.cpu().numpy()
    short, _ = ops.recommend_topk(Ut, It, ut, 50, head, popt, h)
    short = short.cpu().numpy()
    tp, ids = csr_of(tgt)
    seen = 0
    for r in range(NPICK):
        rr, ii = rank[tp[r]:tp[r + 1]], ids[tp[r]:tp[r + 1]]
        inl = (rr >= 0) & (rr < K)
        np.testing.assert_array_equal(idx[r, rr[inl]], ii[inl])
        assert not np.isin(idx[r], ii[~inl]).any()
        seen += int(inl.sum())
        assert len(np.unique(ii[(rr >= 0) & (rr < 50)])) == int(np.isin(short[r], ii).sum())
    assert seen > 200


# ---- 5. geometry and shards ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,head", [(64, 1), (128, 0)])
def test_geometry_runs_and_item_shards(dev, d, head):
    from pda_amd import ops
    nI = 5000
    U, I, pop, hist, users, tgt = case(d, nI)
    p = pop if head else None
    Ut, It, ut, tpt, tit, popt, h = on_dev(dev, U, I, p, users, hist, True, tgt)
    base_rank, base_n = (x.cpu().numpy() for x in ops.rank_targets(Ut, It, ut, tpt, tit, head, popt, h, n_splits=1))
    np.testing.assert_array_equal(base_rank, reference(d, nI, head)[0])
    for splits in (3, 0, 1, 157):
        rank, n = ops.rank_targets(Ut, It, ut, tpt, tit, head, popt, h, n_splits=splits)
        np.testing.assert_array_equal(rank.cpu().numpy(), base_rank)
        np.testing.assert_array_equal(n.cpu().numpy(), base_n)
    # three item shards: keys OR-ed, counts added
    bounds = [0, 1700, 1700 + 2901, nI]
    n_entries = tit.numel()
    keys = torch.zeros(n_entries, dtype=torch.int64, device=dev)
    shards = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        _, Ish, _, _, _, popsh, _ = on_dev(dev, U, I, p, users, hist, True, tgt, lo, hi - lo)
        shards.append((lo, Ish, popsh))
        keys |= ops.rank_keys(Ut, Ish, ut, tpt, tit, head, popsh, h, item_offset=lo)
    above = torch.zeros(n_entries, dtype=torch.int32, device=dev)
    n_ranked = torch.zeros(NPICK, dtype=torch.int32, device=dev)
    for lo, Ish, popsh in shards:
        ops.rank_count(Ut, Ish, ut, tpt, keys, head, popsh, h, item_offset=lo, above=above, n_ranked=n_ranked)
    rank = torch.where(keys != 0, above, torch.full_like(above, -1))
    np.testing.assert_array_equal(rank.cpu().numpy(), base_rank)
    np.testing.assert_array_equal(n_ranked.cpu().numpy(), base_n)
    # a longest row given as an upper bound changes nothing (the workgroups of the empty chunks return at once)
    k1 = ops.rank_keys(Ut, It, ut, tpt, tit, head, popt, h)
    a, _ = ops.rank_count(Ut, It, ut, tpt, k1, head, popt, h, max_row=1000)
    np.testing.assert_array_equal(torch.where(k1 != 0, a, torch.full_like(a, -1)).cpu().numpy(), base_rank)


# ---- 6. bf16 tables -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,head", [(32, 1), (64, 0), (128, 1), (256, 0)])
def test_bf16_tables_equal_the_widened_fp32_call(dev, d, head):
    from pda_amd import ops
    nI = 1999
    U, I, pop, hist, users, tgt = case(d, nI)
    p = pop if head else None
    Ub, Ib, ut, tpt, tit, popt, h = on_dev(dev, U, I, p, users, hist, True, tgt, bf16=True)
    kb = ops.rank_keys(Ub, Ib, ut, tpt, tit, head, popt, h)
    kf = ops.rank_keys(Ub.float(), Ib.float(), ut, tpt, tit, head, popt, h)
    assert torch.equal(kb, kf) and int((kb != 0).sum()) > 1000
    rb, nb = ops.rank_targets(Ub, Ib, ut, tpt, tit, head, popt, h)
    rf, nf = ops.rank_targets(Ub.float(), Ib.float(), ut, tpt, tit, head, popt, h)
    assert torch.equal(rb, rf) and torch.equal(nb, nf)


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------------
COMMON = ["--dataset", "toy", "--epoch", "1", "--log_interval", "1", "--batch_size", "256", "--lr", "1e-2", "--regs", "1e-2", "--valid_set", "valid",
          "--save_flag", "0", "--saveID", "t", "--cuda", "0", "--eval_block", "256", "--bias_groups", "5", "--Ks", "[20,50]"]


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from pda_amd import synthetic
    base = tmp_path_factory.mktemp("rank")
    synthetic.write_dataset(str(base / "data" / "toy"), n_users=600, n_items=400)
    return str(base / "data") + "/", str(base / "save") + "/"


def _run_main(monkeypatch, capsys, toy, extra):
    """train_new_api.main in this process, every eval() pass recorded: (evaluation object, model, rec_type, popularity, result)."""
    from pda_amd import train_new_api as t
    passes = []
    orig = t.evaluation.eval

    def recording(self, model, sess, rec_type, exposure=None):
        ret = orig(self, model, sess, rec_type, exposure)
        passes.append((self, model, rec_type, None if self.testing_popularity is None else self._pop_dev.clone(), ret))
        return ret
    monkeypatch.setattr(t.evaluation, "eval", recording)
    t.main(["--data_path", toy[0], "--save_dir", toy[1], *COMMON, *extra])
    return passes, capsys.readouterr().out.splitlines()


def test_cli_prints_the_rank_lines_and_its_auc_is_the_references(dev, toy, monkeypatch, capsys):
    from pda_amd import ops
    from pda_amd.rank_report import RankReport
    from pda_amd.xquad import train_counts
    passes, lines = _run_main(monkeypatch, capsys, toy, ["--train", "normal", "--test", "normal", "--rank_report", "1", "--bias_report", "1",
                                                       "--rank_ks", "[20, 300]", "--deterministic", "1"])
    metric = [i for i, l in enumerate(lines) if l.startswith("||------") and " recall=[" in l]
    assert len(passes) >= len(metric) >= 8                                          # (the pass that ends the gamma search is not printed)
    recorded = [list(p[4].rank_lines) for p in passes]
    n_rank = 1 + 2 + 1 + 2                                                           # auc line, two cut-offs, the groups, their recall
    for n, i in enumerate(metric):
        j = i + 1
        while lines[j].startswith("||--- bias"):                                    # the rank lines stand under the bias lines
            j += 1
        assert j >= i + 3
        block = lines[j:j + n_rank]
        assert block in recorded, block
        assert block[0].startswith("||--- rank auc=") and block[1].startswith("||--- rank@20 recall=") and block[2].startswith("||--- rank@300 ")
        assert block[3].startswith("||--- rank groups targets=[") and block[5].startswith("||--- rank@300 group_recall=[")
    assert sum(l.startswith("||--- rank") for l in lines) == n_rank * len(metric)

    # the last pass of each head on the final tables, restated: the dense kernel's matrix, the numpy ranks, the report
    for rec_type in ("main_branch", "main_with_pop"):
        ev, model, _, pop, ret = [p for p in passes if p[2] == rec_type][-1]
        U, I = model.Recommender.score_tables()
        users = ev.users_dev.cpu().numpy()
        sd = ops.score_dense(U, I, ev.users_dev, ops.HEAD_POP if pop is not None else ops.HEAD_RAW, pop).cpu().numpy()
        tgt = [ev.eval_user_list[int(u)] for u in users]
        hist = [ev.data.train_user_list[int(u)] for u in users]
        rank, n = rank_ref(sd, hist, tgt)
        want = RankReport(train_counts(ev.data), "[20, 300]", 5, "interactions").stats(rank, n, *csr_of(tgt)).lines()
        assert list(ret.rank_lines) == want
        auc = float(re.search(r"auc=([\d.]+) ", want[0]).group(1))
        assert 0.0 < auc < 1.0
        # recall@20 of the ranks is the metrics line's recall@20
        assert float(re.search(r"recall=([\d.]+)", want[1]).group(1)) == pytest.approx(ret["recall"][0], abs=6e-6)


def test_cli_gamma_search_of_a_pd_model(dev, toy, monkeypatch, capsys):
    passes, lines = _run_main(monkeypatch, capsys, toy, ["--train", "s_condition", "--test", "normal", "--rank_report", "1"])
    metric = [i for i, l in enumerate(lines) if l.startswith("||------") and " recall=[" in l]
    searched = [p for p in passes if p[2] == "main_with_pop"]
    assert len(passes) >= len(metric) >= 8 and len(searched) >= 5
    for i in metric:
        assert lines[i + 1].startswith("||--- rank auc=") and lines[i + 2].startswith("||--- rank@50 ") and lines[i + 3].startswith("||--- rank@1000 ")
    assert not any(l.startswith("||--- bias") for l in lines)
    assert len({p[4].rank_lines[0] for p in searched}) > 1                           # the popularity's exponent moves the ranks
