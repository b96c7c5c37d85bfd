"""GPU parity of the deep lists (pda_deep_topk_f32 / _bf16, pda_metrics_deep, --topk_max, pda_amd.export_topk) against the CPU oracle.

Bar: for the raw head, ids and values equal oracle order 1 exactly; for the popularity head (hardware exp) the project's near-tie criterion at
TOL, every returned value bit-equal to pda_score_dense_f32 at its pair, and every list the exact sort of the masked dense row.  Inputs come
from test_gpu_score_topk.make_case (exact-zero popularities, duplicate history entries, ragged user counts)."""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from test_gpu_score_topk import check_against_oracle, csr, make_case

pytestmark = pytest.mark.gpu


def run_deep(dev, U, I, users, K, head, pop, hist_rows, by_user, item_offset=0, n_local=None, bf16=False, want="idx_val", stats=None, budget=None):
    """hist_rows: per USER ID when by_user, per block row otherwise."""
    from pda_amd import ops
    n_local = I.shape[0] - item_offset if n_local is None else n_local
    Ut, Ish = torch.from_numpy(U).to(dev), torch.from_numpy(I[item_offset:item_offset + n_local].copy()).to(dev)
    if bf16:
        Ut, Ish = Ut.bfloat16(), Ish.bfloat16()
    popsh = None if pop is None else torch.from_numpy(pop[item_offset:item_offset + n_local].copy()).to(dev)
    h = None
    if hist_rows is not None:
        ip, ix = csr(hist_rows)
        h = ops.HistoryCSR(torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev), by_user=by_user)
    out = ops.recommend_topk_deep(Ut, Ish, torch.from_numpy(users).to(dev), K, head, popsh, h, item_offset, stats=stats, want=want,
                                  workspace_budget=budget)
    torch.cuda.synchronize()
    if want == "keys":
        return out.cpu().numpy()
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def some_users(rng, nU, n):
    return rng.choice(nU, n, replace=False).astype(np.int32)          # (unsorted: block rows and user ids differ)


@pytest.mark.parametrize("d", [32, 64, 128, 256])
@pytest.mark.parametrize("K", [55, 64, 100, 257, 1000, 1024])
@pytest.mark.parametrize("nI", [1999, 5000])
def test_raw_head_equals_the_oracle_exactly(dev, d, K, nI):
    rng = np.random.default_rng(1000 * d + K + nI)
    nU = 300
    U, I, pop, hist = make_case(rng, nU, nI, d)
    users = some_users(rng, nU, 173)
    blk = [hist[u] for u in users]
    ridx, rval = c_oracle.score_topk(U, I, users, K, 0, None, *csr(blk), order=1)
    for by_user in (False, True):
        idx, val = run_deep(dev, U, I, users, K, 0, None, hist if by_user else blk, by_user)
        np.testing.assert_array_equal(val, rval)
        np.testing.assert_array_equal(idx, ridx)


@pytest.mark.parametrize("d,K", [(64, 100), (128, 1000), (32, 55), (256, 257)])
def test_item_shard_with_an_offset(dev, d, K):
    rng = np.random.default_rng(31 + d)
    nU, nI, off, nloc = 300, 5000, 1700, 2901
    U, I, pop, hist = make_case(rng, nU, nI, d)
    users = some_users(rng, nU, 173)
    blk = [hist[u] for u in users]
    ip, ix = csr(blk)
    ridx, rval = c_oracle.score_topk(U, I, users, K, 0, None, ip, ix, item_offset=off, n_items_local=nloc, order=1)
    idx, val = run_deep(dev, U, I, users, K, 0, None, hist, True, item_offset=off, n_local=nloc)
    np.testing.assert_array_equal(val, rval)
    np.testing.assert_array_equal(idx, ridx)
    assert idx.min() >= off and idx.max() < off + nloc


@pytest.mark.parametrize("d,K,nI", [(32, 64, 1999), (64, 100, 5000), (128, 1000, 1999), (128, 257, 5000), (256, 1024, 5000), (64, 55, 1999)])
def test_pop_head_three_ways(dev, d, K, nI):
    from pda_amd import ops
    rng = np.random.default_rng(7 * d + K)
    nU = 300
    U, I, pop, hist = make_case(rng, nU, nI, d)
    users = some_users(rng, nU, 173)
    blk = [hist[u] for u in users]
    idx, val = run_deep(dev, U, I, users, K, 1, pop, hist, True)
    # 1: the project's near-tie criterion against the oracle (libm exp there, the hardware's here)
    check_against_oracle(idx, val, U, I, users, K, 1, pop, blk, exact=False)
    # 2: every pair is the dense kernel's value at that pair, bit for bit
    sd = ops.score_dense(torch.from_numpy(U).to(dev), torch.from_numpy(I).to(dev), torch.from_numpy(users).to(dev), ops.HEAD_POP,
                         torch.from_numpy(pop).to(dev)).cpu().numpy()
    at = np.take_along_axis(sd, idx.astype(np.int64), axis=1)
    assert np.isfinite(val).all()
    np.testing.assert_array_equal((val + np.float32(0)).view(np.uint32), (at + np.float32(0)).view(np.uint32))   # (-0.0 is +0.0 in a key)
    # 3: every list is the sort of the masked dense row by (value descending, id ascending)
    masked = sd.copy()
    for r, h in enumerate(blk):
        masked[r, h] = -np.inf
    ids = np.arange(nI)
    for r in range(len(users)):
        order = np.lexsort((ids, -masked[r]))[:K]
        np.testing.assert_array_equal(idx[r], order)
        np.testing.assert_array_equal(val[r], masked[r, order])


def test_short_rows_end_in_their_listed_items_by_id(dev):
    rng = np.random.default_rng(9)
    nU, nI, d = 33, 600, 64
    U, I, pop, _ = make_case(rng, nU, nI, d, max_hist=0)
    hist = [rng.permutation(nI)[:rng.integers(nI - 250, nI + 1)].astype(np.int32) for _ in range(nU)]     # 0 .. 250 unlisted items
    hist[0] = np.arange(nI, dtype=np.int32)                    # everything listed
    hist[1] = np.concatenate([hist[1], hist[1][:40]])          # duplicates count once
    users = np.arange(nU, dtype=np.int32)
    for K in (257, 300, 600):
        for head, p in ((0, None), (1, pop)):
            idx, val = run_deep(dev, U, I, users, K, head, p, hist, True)
            ridx, rval = c_oracle.score_topk(U, I, users, K, head, p, *csr(hist), order=1)
            short = np.array([nI - len(np.unique(h)) < K for h in hist])
            assert short.sum() >= 10
            np.testing.assert_array_equal(np.isneginf(val), np.isneginf(rval))
            if head == 0:
                np.testing.assert_array_equal(idx, ridx)
                np.testing.assert_array_equal(val, rval)
            else:
                tail = np.isneginf(rval)
                np.testing.assert_array_equal(idx[tail], ridx[tail])
                check_against_oracle(idx, val, U, I, users, K, head, p, hist, exact=False)


def test_equal_scores_rank_by_id(dev):
    rng = np.random.default_rng(3)
    nU, nI, d = 40, 1400, 64
    U, I, pop, _ = make_case(rng, nU, nI, d, max_hist=0)
    I[100:900] = I[50]                  # 801 items with bit-identical scores for every user
    I[1000:1020] = 0.0                  # exact zeros (+ -0.0 products)
    users = np.arange(nU, dtype=np.int32)
    for K in (300, 1000):
        idx, val = run_deep(dev, U, I, users, K, 0, None, None, False)
        ridx, rval = c_oracle.score_topk(U, I, users, K, 0, None, order=1)
        np.testing.assert_array_equal(idx, ridx)
        np.testing.assert_array_equal(val, rval)
        same = val[:, 1:] == val[:, :-1]
        assert np.all(idx[:, 1:][same] > idx[:, :-1][same])
        if K == 1000:                   # at most 599 items rank ahead of the 801 equal ones: at least 401 of them are in every list
            assert same.sum() >= nU * 400
    # popularity exactly 0 => head exactly 0 for every item: the list is the first K ids
    idx, val = run_deep(dev, U, I, users, 700, 1, np.zeros(nI, np.float32), None, False)
    np.testing.assert_array_equal(idx, np.tile(np.arange(700, dtype=np.int32), (nU, 1)))
    np.testing.assert_array_equal(val, np.zeros_like(val))


@pytest.mark.parametrize("d", [32, 128])
def test_k_equals_the_catalogue_and_one_user(dev, d):
    rng = np.random.default_rng(17 + d)
    nU, nI = 150, 1024
    U, I, pop, hist = make_case(rng, nU, nI, d)
    users = np.arange(nU, dtype=np.int32)
    idx, val = run_deep(dev, U, I, users, nI, 0, None, hist, True)               # K = n_items_local: every item, the listed ones last
    ridx, rval = c_oracle.score_topk(U, I, users, nI, 0, None, *csr(hist), order=1)
    np.testing.assert_array_equal(idx, ridx)
    np.testing.assert_array_equal(val, rval)
    assert (np.sort(idx, axis=1) == np.arange(nI)).all()
    one = np.array([77], dtype=np.int32)
    for K in (55, 1000):
        idx, val = run_deep(dev, U, I, one, K, 0, None, [hist[77]], False)
        ridx, rval = c_oracle.score_topk(U, I, one, K, 0, None, *csr([hist[77]]), order=1)
        np.testing.assert_array_equal(idx, ridx)
        np.testing.assert_array_equal(val, rval)


@pytest.mark.parametrize("d", [64, 128])
def test_nan_popularity_items_never_rank(dev, d):
    rng = np.random.default_rng(77 + d)
    nU, nI, K = 260, 3000, 300
    U, I, pop, hist = make_case(rng, nU, nI, d)
    nan_items = np.unique(np.concatenate([rng.choice(nI, 40, replace=False), np.argsort(-pop)[:3]]))      # (some of the most popular ones among them)
    pop_nan = pop.copy()
    pop_nan[nan_items] = np.nan
    users = np.arange(nU, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        idx, val = run_deep(dev, U, I, users, K, 1, pop_nan, hist, True)
    assert not np.isin(idx, nan_items).any() and np.isfinite(val).all()
    masked = [np.union1d(h, nan_items).astype(np.int32) for h in hist]           # the oracle: the same items masked instead
    check_against_oracle(idx, val, U, I, users, K, 1, pop, masked, exact=False)


@pytest.mark.parametrize("K", [1, 20, 50, 54])
@pytest.mark.parametrize("head", [0, 1])
def test_parity_with_the_short_list_route(dev, K, head):
    """At K <= 54 both routes exist: the deep call returns exactly what score_topk_keys + topk_merge return -- NaN popularities and short rows
    included."""
    from pda_amd import ops
    rng = np.random.default_rng(5 + K)
    for nU, nI, d, kind in ((173, 1999, 64, "plain"), (140, 3000, 128, "nan"), (33, 96, 64, "short")):
        if K > nI:
            continue
        U, I, pop, hist = make_case(rng, nU, nI, d)
        if kind == "nan":
            pop[rng.choice(nI, 40, replace=False)] = np.nan
        if kind == "short":
            hist = [rng.permutation(nI)[:rng.integers(40, nI + 1)].astype(np.int32) for _ in range(nU)]
            hist[0] = np.arange(nI, dtype=np.int32)
            if head == 1:
                pop[rng.choice(nI, 10, replace=False)] = np.nan
        users = np.arange(nU, dtype=np.int32)
        p = pop if head == 1 else None
        Ut, It, ut = torch.from_numpy(U).to(dev), torch.from_numpy(I).to(dev), torch.from_numpy(users).to(dev)
        pt = None if p is None else torch.from_numpy(p).to(dev)
        ip, ix = csr(hist)
        h = ops.HistoryCSR(torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev), by_user=True)
        with np.errstate(invalid="ignore"):
            ridx, rval = ops.topk_merge(ops.score_topk_keys(Ut, It, ut, K, head, pt, h), ut, h)
            idx, val = ops.recommend_topk_deep(Ut, It, ut, K, head, pt, h)
        assert torch.equal(idx, ridx), (kind, int((idx != ridx).sum()))
        assert torch.equal(val, rval), kind
        # and the packed keys are pda_topk_merge's
        rkeys = ops.topk_merge(ops.score_topk_keys(Ut, It, ut, K, head, pt, h), ut, h, want="keys")
        keys = ops.recommend_topk_deep(Ut, It, ut, K, head, pt, h, want="keys")
        assert torch.equal(keys, rkeys), kind


@pytest.mark.parametrize("d", [32, 64, 128, 256])
@pytest.mark.parametrize("head", [0, 1])
def test_bf16_tables_equal_the_widened_fp32_tables(dev, d, head):
    rng = np.random.default_rng(11 + d)
    nU, nI, K = 200, 2500, 300
    U, I, pop, hist = make_case(rng, nU, nI, d)
    U = torch.from_numpy(U).bfloat16().float().numpy()
    I = torch.from_numpy(I).bfloat16().float().numpy()
    users = some_users(rng, nU, 150)
    st16, st32 = {}, {}
    p = pop if head == 1 else None
    idx16, val16 = run_deep(dev, U, I, users, K, head, p, hist, True, bf16=True, stats=st16)
    idx32, val32 = run_deep(dev, U, I, users, K, head, p, hist, True, stats=st32)
    np.testing.assert_array_equal(idx16, idx32)
    np.testing.assert_array_equal(val16, val32)
    from pda_amd import ops
    assert ops.deep_kernel_identity(st16["kernel_id"][0])["bf16"] and not ops.deep_kernel_identity(st32["kernel_id"][0])["bf16"]


@pytest.mark.parametrize("d", [32, 64, 128, 256])
@pytest.mark.parametrize("head", [0, 1])
def test_identity_word_names_the_kernel(dev, d, head):
    from pda_amd import ops
    rng = np.random.default_rng(d)
    U, I, pop, hist = make_case(rng, 64, 700, d)
    st = {}
    run_deep(dev, U, I, np.arange(64, dtype=np.int32), 100, head, pop if head else None, hist, True, stats=st)
    assert ops.deep_kernel_identity(st["kernel_id"][0]) == {"generation": ops.DEEP_GENERATION, "head": head, "bf16": False, "d": d}
    assert st["workspace_bytes"] == ops.deep_workspace_bytes(64, 700, d, 100)


def test_chunked_users_equal_one_call(dev):
    """A workspace budget below the block's need: the users go in chunks (a history by block row is re-based per chunk), same lists."""
    from pda_amd import ops
    rng = np.random.default_rng(41)
    nU, nI, d, K = 700, 1999, 64, 100
    U, I, pop, hist = make_case(rng, nU, nI, d)
    users = some_users(rng, nU, 650)
    blk = [hist[u] for u in users]
    whole = run_deep(dev, U, I, users, K, 1, pop, blk, False)
    budget = ops.deep_workspace_bytes(256, nI, d, K)
    for by_user in (False, True):
        st = {}
        got = run_deep(dev, U, I, users, K, 1, pop, hist if by_user else blk, by_user, stats=st, budget=budget)
        assert st["chunk_users"] == 256
        np.testing.assert_array_equal(got[0], whole[0])
        np.testing.assert_array_equal(got[1], whole[1])


@pytest.mark.parametrize("k_cols", [50, 100, 1000])
def test_deep_metrics_against_the_oracle(dev, k_cols):
    from pda_amd import ops
    rng = np.random.default_rng(k_cols)
    nU, nI, d = 700, 1999, 32
    U, I, pop, hist = make_case(rng, nU, nI, d)
    users = np.arange(nU, dtype=np.int32)
    lists, _ = c_oracle.score_topk(U, I, users, k_cols, 0, None, *csr(hist), order=1)
    # targets: a few of the listed items (hits at every depth) and a few others, every row has at least one
    tg = [np.unique(np.concatenate([rng.choice(lists[r], rng.integers(1, 12), replace=False), rng.integers(0, nI, rng.integers(0, 20))])).astype(np.int32)
          for r in range(nU)]
    tp, tx = csr(tg)
    Ks = [k for k in (20, 50, 100, 500) if k <= k_cols]
    ref = c_oracle.metrics(lists, tp, tx, Ks)
    assert np.isfinite(ref).all() and (ref[1] > 0).all()
    args = (torch.from_numpy(lists).to(dev), torch.from_numpy(tp).to(dev), torch.from_numpy(tx).to(dev), torch.tensor(Ks, dtype=torch.int32, device=dev))
    got = ops.metrics_sums_deep(*args).cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-12)
    o1 = ops.metrics_sums_deep_ordered(*args).cpu().numpy()
    o2 = ops.metrics_sums_deep_ordered(*args).cpu().numpy()
    assert o1.tobytes() == o2.tobytes()
    np.testing.assert_allclose(o1, got, rtol=1e-12)
    # sums are added to: a second call doubles them
    acc = ops.metrics_sums_deep(*args)
    ops.metrics_sums_deep(*args, sums=acc)
    np.testing.assert_allclose(acc.cpu().numpy(), 2 * ref, rtol=1e-12)
    if k_cols <= 64:                     # where both exist, the short-list kernel agrees
        np.testing.assert_allclose(ops.metrics_sums(*args).cpu().numpy(), ref, rtol=1e-12)


# ---- end to end: --topk_max through the trainer, the evaluation and the export -------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from pda_amd import synthetic
    root = tmp_path_factory.mktemp("data")
    synthetic.write_dataset(str(root / "toy"), n_users=400, n_items=1500)
    return str(root) + "/"


def _argv(toy, save, train, extra=()):
    return ["--data_path", toy, "--dataset", "toy", "--train", train, "--test", train, "--epoch", "3", "--log_interval", "2",
            "--batch_size", "256", "--lr", "1e-2", "--regs", "1e-2", "--valid_set", "valid", "--pop_exp", "0.22",
            "--save_dir", save, "--Ks", "[20,50,100,300]", "--save_flag", "0", "--saveID", "t", "--cuda", "0", "--eval_block", "128",
            "--topk_max", "300"] + list(extra)


@pytest.mark.parametrize("train,extra", [("normal", ()), ("s_condition", ("--deterministic", "1"))])
def test_topk_max_end_to_end(dev, toy, tmp_path, capsys, train, extra):
    from pda_amd import export_topk
    from pda_amd import train_new_api as t
    save = str(tmp_path) + "/"
    argv = _argv(toy, save, train, extra)
    t.main(argv)
    out = capsys.readouterr().out
    assert "training and testing end!!!!" in out and "top K: [20, 50, 100, 300]" in out

    npz = str(tmp_path / "lists" / "top300.npz")
    exported = export_topk.main(argv + ["--export_out", npz])
    z = np.load(npz)
    assert z["users"].dtype == np.int32 and z["idx"].dtype == np.int32 and z["val"].dtype == np.float32
    assert z["idx"].shape == (len(z["users"]), 300) == z["val"].shape
    for k in ("users", "idx", "val"):
        np.testing.assert_array_equal(z[k], exported[k])

    args, model, ev, rec_type, popularity = export_topk.restore(argv)
    assert model.topk_max == 300 and rec_type == ("main_branch" if train == "normal" else "condition")
    d = t.data
    users = list(d.valid_user_list.keys())
    np.testing.assert_array_equal(z["users"], np.asarray(users, dtype=np.int32))
    # the export is recommend_device of the same model
    idx, val = model.recommend_device(ev.users_dev, None, rec_type, None if popularity is None else ev._pop_dev, ev._hist)
    np.testing.assert_array_equal(z["idx"], idx.cpu().numpy())
    np.testing.assert_array_equal(z["val"], val.cpu().numpy())

    # evaluation.eval on 300 columns == the metrics of the oracle's lists of the trained tables
    rec = model.Recommender
    U = rec.weights["user_embedding"].float().cpu().numpy()
    I = rec.weights["item_embedding"].float().cpu().numpy()
    hist = [np.asarray(sorted(d.train_user_list[u]), dtype=np.int32) for u in users]
    tgt = [np.asarray(d.valid_user_list[u], dtype=np.int32) for u in users]
    Ks = [20, 50, 100, 300]
    for rt, pop in (("main_branch", None),) + ((("condition", popularity),) if train == "s_condition" else ()):
        ev.set_testing_popularity(pop)
        got = ev.eval(model, None, rt)
        assert (np.diff(got["recall"]) >= 0).all() and got["recall"][-1] > 0
        p32 = None if pop is None else np.asarray(pop, dtype=np.float32)
        ridx, _ = c_oracle.score_topk(U, I, np.asarray(users, dtype=np.int32), 300, 0 if pop is None else 1, p32, *csr(hist), order=1)
        if pop is not None:                              # (the popularity head: the device's own lists where they differ by a near-tie only)
            gidx, gval = model.recommend_device(ev.users_dev, None, rt, ev._pop_dev, ev._hist)
            check_against_oracle(gidx.cpu().numpy(), gval.cpu().numpy(), U, I, np.asarray(users, dtype=np.int32), 300, 1, p32, hist, exact=False)
            ridx = gidx.cpu().numpy()
        ref = c_oracle.metrics(ridx, *csr(tgt), Ks) / float(len(users))
        for row, name in enumerate(("precision", "recall", "ndcg", "hit_ratio")):
            np.testing.assert_allclose(got[name], ref[row], rtol=0, atol=1e-6, err_msg=rt + " " + name)
