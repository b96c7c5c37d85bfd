"""GPU: BPR-PC (`python -m pda_amd.bpr_pc`) -- the item moments, the per-user statistics, the PC score call (sweep, finish and fallback) and
the driver end to end, against the numpy restatement of tests/pc_ref.py and the CPU oracle's exact fp32 score chain."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import c_oracle
from pc_ref import finish_stats, moments, pc_lists, stats_direct

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def to(dev, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


def csr(rows, dev, by_user):
    from pda_amd import ops
    lens = [len(r) for r in rows]
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum(lens)
    flat = np.concatenate([np.sort(np.asarray(r, np.int64)) for r in rows]).astype(np.int32) if rows else np.zeros(0, np.int32)
    return ops.HistoryCSR(*to(dev, indptr, flat), by_user=by_user)


def tables(rng, nU, nI, d, scale=0.1):
    U = (rng.standard_normal((nU, d)) * scale).astype(f32)
    I = (rng.standard_normal((nI, d)) * scale).astype(f32)
    pop = rng.integers(1, 200, nI).astype(f32)
    return U, I, pop


def histories(rng, n_rows, nI, kinds=True):
    hist = [np.sort(rng.choice(nI, rng.integers(0, 25), replace=False)) for _ in range(n_rows)]
    if kinds:
        hist[0] = np.sort(np.concatenate([hist[0], hist[0][:3], hist[0][:1]]))    # c = 2 and c = 3
        hist[1] = np.zeros(0, np.int64)                                           # empty
        hist[2] = np.delete(np.arange(nI), [3, 77, 400])                          # near-full
    return hist


@pytest.mark.parametrize("d", [64, 128, 256])
def test_item_moments(dev, d):
    from pda_amd import ops
    rng = np.random.default_rng(d)
    _, I, pop = tables(rng, 1, 1001, d, 0.3)
    mom = ops.pc_item_moments(*to(dev, I, pop)).cpu().numpy()
    G, H, h, P = moments(I, pop)
    got = ops.split_moments(torch.from_numpy(mom), d)
    for g, w in zip(got[:3], (G, H, h)):
        np.testing.assert_allclose(g.numpy(), w, rtol=1e-12, atol=1e-12 * np.abs(w).max())
    assert float(got[3]) == pytest.approx(P, rel=1e-12)


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("beta", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("mode", ["user_id", "block_row"])
def test_user_stats(dev, d, beta, mode):
    from pda_amd import ops
    rng = np.random.default_rng(d + int(10 * beta) + len(mode))
    nU, nI, nb = 400, 1001, 150
    U, I, pop = tables(rng, nU, nI, d)
    users = np.concatenate([np.arange(4), 4 + rng.permutation(nU - 4)[:nb - 4]]).astype(np.int32)   # rows 0 .. 3 are users 0 .. 3
    hist = histories(rng, nU if mode == "user_id" else nb, nI)
    hist[3] = np.arange(nI)                                                      # n_u = 0: k_u = 0
    rows = [hist[u] for u in users] if mode == "user_id" else hist
    Un, Uc, k = (x.cpu().numpy() for x in ops.pc_user_stats(*to(dev, U, I, users, pop), beta, csr(hist, dev, mode == "user_id")))
    wUn, wUc, wk = finish_stats(*stats_direct(U, I, users, rows, pop, beta))
    np.testing.assert_allclose(Un, wUn, rtol=2e-6)
    np.testing.assert_allclose(Uc, wUc, rtol=2e-6)
    np.testing.assert_allclose(k, wk, rtol=4e-6)
    assert Un[3] == 0 and Uc[3] == 0 and k[3] == 0 and (k[4:] > 0).all()


def oracle_lists(U, I, users, rows, pop, k, alpha, beta, K, block):
    s = c_oracle.scores_chain(U, I, users)
    return pc_lists(s, rows, pop, k, alpha, beta, K, block=block, return_r=True)


def run_pc(dev, U, I, users, pop, hist_rows, by_user, alpha, beta, K, rpm, hist_all=None):
    from pda_amd import ops
    h = csr(hist_all if hist_all is not None else hist_rows, dev, by_user)
    Ut, It, ut, pt = to(dev, U, I, users, pop)
    k = ops.pc_user_stats(Ut, It, ut, pt, beta, h)[2]
    stats = {}
    idx, val = ops.recommend_topk_pc(Ut, It, ut, pt, k, alpha, beta, K, h, rows_per_min=rpm, stats=stats)
    return idx.cpu().numpy(), val.cpu().numpy(), k.cpu().numpy(), stats


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("K", [1, 20, 50])
@pytest.mark.parametrize("mode", ["user_id", "block_row"])
def test_lists_bit_exact(dev, d, K, mode):
    """idx and val against the oracle given the library's k_u; 900 rows in groups of 256 (four m, the last group short)."""
    from pda_amd import ops
    rng = np.random.default_rng(d + K + len(mode))
    nU, nI, nb = 1200, 3001, 900
    U, I, pop = tables(rng, nU, nI, d)
    users = rng.permutation(nU)[:nb].astype(np.int32)
    hist = histories(rng, nU if mode == "user_id" else nb, nI, kinds=False)
    rows = [hist[u] for u in users] if mode == "user_id" else hist
    for alpha, beta in ((0.1, 0.5), (2.0, 0.0), (0.0, 1.0)):
        idx, val, k, stats = run_pc(dev, U, I, users, pop, rows, mode == "user_id", alpha, beta, K, 256, hist_all=hist)
        widx, wval, _ = oracle_lists(U, I, users, rows, pop, k, alpha, beta, K, 256)
        np.testing.assert_array_equal(idx, widx)
        np.testing.assert_array_equal(val, wval)
        assert stats["pc_fallback_rows"] == 0
        assert ops.pc_kernel_identity(stats["kernel_id"].cpu().numpy()[0]) == {"generation": 1, "pc_head": True, "d": d}


def test_forced_fallback(dev):
    """One extreme user drives m_B far below the others' ratings: the shift merges distinct r into equal g, the lower id then wins, and
    the rows the ranking by r cannot settle go through the fallback sweep."""
    rng = np.random.default_rng(11)
    d, nI, nb, K = 64, 4000, 300, 50
    U, I, pop = tables(rng, nb, nI, d, 0.02)
    U[7] = rng.standard_normal(d).astype(f32) * 1e4                             # its scores reach about -5e3
    users = np.arange(nb, dtype=np.int32)
    hist = [np.sort(rng.choice(nI, 10, replace=False)) for _ in range(nb)]
    for alpha, beta in ((0.1, 0.3), (1.0, 0.7)):
        idx, val, k, stats = run_pc(dev, U, I, users, pop, hist, False, alpha, beta, K, 2048)
        widx, wval, r = oracle_lists(U, I, users, hist, pop, k, alpha, beta, K, 2048)
        assert r.min() < -1e3
        by_r = np.array([np.lexsort((np.arange(nI), -np.where(np.isin(np.arange(nI), hist[u]), -np.inf, r[u])))[:K] for u in range(nb)])
        assert (by_r != widx).any(), "the test needs rows whose g order differs from their r order"
        np.testing.assert_array_equal(idx, widx)
        np.testing.assert_array_equal(val, wval)
        assert stats["pc_fallback_rows"] > 0


def test_fill_rows_with_few_unmasked_items(dev):
    rng = np.random.default_rng(5)
    d, nI, nb, K = 128, 90, 40, 50
    U, I, pop = tables(rng, nb, nI, d)
    users = np.arange(nb, dtype=np.int32)
    hist = [np.sort(rng.choice(nI, rng.integers(0, 30), replace=False)) for _ in range(nb)]
    hist[0] = np.delete(np.arange(nI), [4, 60])                                  # 2 unmasked, 88 listed once
    rest = np.delete(np.arange(nI), [8, 9, 10])
    hist[1] = np.sort(np.concatenate([rest, rest[:70], [rest[0]]]))             # listed twice, three times, once
    hist[2] = np.sort(np.concatenate([np.delete(np.arange(nI), [1]), [5]]))    # one duplicate entry
    for mode in ("block_row", "user_id"):
        idx, val, k, stats = run_pc(dev, U, I, users, pop, hist, mode == "user_id", 0.5, 0.4, K, 2048)
        widx, wval, _ = oracle_lists(U, I, users, hist, pop, k, 0.5, 0.4, K, 2048)
        np.testing.assert_array_equal(idx, widx)
        np.testing.assert_array_equal(val, wval)
    assert (wval[1, 3:] <= 0).all() and (wval[1, -10:] < 0).all()


def _model(dev, toy, d=64):
    from pda_amd import train_new_api as t
    from pda_amd.sampler import host_generator
    t.configure(["--data_path", toy, "--dataset", "toy", "--train", "normal", "--Ks", "[20,50]", "--embed_size", str(d)])
    data = t.data
    model = t.DatasetApi_Model(t.args, {"n_users": data.n_users, "n_items": data.n_items}, 256, (lambda: host_generator(data, False)), dev)
    return t, data, model


def test_block_size_invariance(dev, tmp_path):
    from pda_amd import synthetic
    from pda_amd.bpr_pc import PC_model, get_dataset_tot_popularity_for_PC
    toy = str(tmp_path / "data") + "/"
    synthetic.write_dataset(toy + "toy", n_users=20000, n_items=300, mean_hist=8)
    t, data, model = _model(dev, toy)
    pc = PC_model(model, 50, 0.4, 0.2)
    pop = get_dataset_tot_popularity_for_PC(data)
    rets = []
    for blk in (2048, 4096, 262144):
        ev = t.evaluation(data, [20, 50], dev, block=blk)
        ev.set_evaluate_obj_pre("test")
        assert ev.tot_user > 4096
        ev.set_clicked_value_type("pc")
        ev.set_testing_popularity(pop)
        rets.append(ev.eval(pc, None, rec_type="main_branch"))
    for r in rets[1:]:
        for key in ("recall", "precision", "ndcg", "hit_ratio"):
            np.testing.assert_allclose(r[key], rets[0][key], rtol=1e-12, atol=0)
    ev = t.evaluation(data, [20, 50], dev, block=3000)
    ev.set_evaluate_obj_pre("test")
    ev.set_testing_popularity(pop)
    with pytest.raises(ValueError, match="whole reference blocks"):
        ev.eval(pc, None, rec_type="main_branch")


def test_do_recommendation_protocol(dev, tmp_path):
    """The reference's protocol: one call per 2 048-user block with the COO triple of value 1.0 gives the oracle's lists."""
    from pda_amd import synthetic
    from pda_amd.bpr_pc import PC_model, get_dataset_tot_popularity_for_PC
    toy = str(tmp_path / "data") + "/"
    synthetic.write_dataset(toy + "toy", n_users=2500, n_items=200, mean_hist=8)
    t, data, model = _model(dev, toy)
    pc = PC_model(model, 50, 0.3, 0.6)
    pop = get_dataset_tot_popularity_for_PC(data)
    users = np.asarray(list(data.test_user_list.keys()), dtype=np.int32)[:2048]
    index = np.array([(r, it) for r, u in enumerate(users) for it in data.train_user_list[u]], dtype=np.int64)
    got = pc.do_recommendation(None, users, list(range(data.n_items)), "main_branch", pos_pop=pop,
                               sparse_cliked_matrix=(index, np.ones(len(index), np.float32), np.array([len(users), data.n_items])))
    U, I = (x.cpu().numpy() for x in model.Recommender.score_tables())
    k = pc.scale(*to(dev, users), *to(dev, pop.astype(f32)), csr([data.train_user_list[u] for u in users], dev, False)).cpu().numpy()
    want, _, _ = oracle_lists(U, I, users, [data.train_user_list[u] for u in users], pop, k, 0.3, 0.6, 50, 2048)
    np.testing.assert_array_equal(got, want)
    with pytest.raises(NotImplementedError):
        pc.do_recommendation(None, users, list(range(10)), "main_branch", pos_pop=pop, sparse_cliked_matrix=(index, np.ones(len(index)), (2048, 10)))


def test_ctypes_only_caller(dev):
    """the C ABI through ctypes alone (no pda_amd), device buffers from torch."""
    from pda_amd import ops
    rng = np.random.default_rng(3)
    d, nI, nb, K = 128, 2000, 300, 20
    U, I, pop = tables(rng, nb, nI, d)
    users = np.arange(nb, dtype=np.int32)
    hist = [np.sort(rng.choice(nI, 12, replace=False)) for _ in range(nb)]
    h = csr(hist, dev, False)
    Ut, It, ut, pt = to(dev, U, I, users, pop)
    lib = C.CDLL(os.path.join(ROOT, "pda_amd", "csrc", "libpda_hip.so"))
    vp, sz = C.c_void_p, C.c_size_t
    lib.pda_pc_moments_workspace_bytes.restype = sz
    lib.pda_pc_score_workspace_bytes.restype = sz
    p = lambda t: vp(t.data_ptr())
    mom = torch.empty(2 * d * d + d + 1, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.pda_pc_moments_workspace_bytes(nI, d), dtype=torch.uint8, device=dev)
    stream = vp(torch.cuda.current_stream().cuda_stream)
    assert lib.pda_pc_item_moments_f32(p(It), p(pt), nI, d, p(mom), p(ws), stream) == 0
    st = torch.empty((3, nb), dtype=torch.float32, device=dev)
    assert lib.pda_pc_user_stats_f32(p(Ut), p(It), p(pt), p(mom), p(ut), nb, nI, d, p(h.indptr), p(h.indices), 0, C.c_double(0.3),
                                     p(st[0]), p(st[1]), p(st[2]), stream) == 0
    idx = torch.empty((nb, K), dtype=torch.int32, device=dev)
    val = torch.empty((nb, K), dtype=torch.float32, device=dev)
    wsz = lib.pda_pc_score_workspace_bytes(nb, nI, d, K)
    ws2 = torch.empty(wsz, dtype=torch.uint8, device=dev)       # (the caching allocator hands out 512-byte aligned blocks)
    assert ws2.data_ptr() % 256 == 0
    assert lib.pda_pc_score_topk_f32(p(Ut), p(It), p(pt), p(st[2]), p(ut), nb, nI, d, p(h.indptr), p(h.indices), 0, C.c_double(0.7),
                                     C.c_double(0.3), 2048, K, p(idx), p(val), p(ws2), stream) == 0
    widx, wval = ops.recommend_topk_pc(Ut, It, ut, pt, st[2].clone(), 0.7, 0.3, K, h)
    assert torch.equal(idx, widx) and torch.equal(val, wval)


def _cli(module, toy, save, extra=()):
    argv = [sys.executable, "-m", module, "--data_path", toy, "--dataset", "toy", "--train", "normal", "--test", "normal", "--epoch", "2",
            "--log_interval", "1", "--batch_size", "256", "--lr", "1e-2", "--regs", "1e-2", "--valid_set", "valid", "--save_dir", save,
            "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t", "--cuda", "0", *extra]
    r = subprocess.run(argv, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_cli_end_to_end(dev, tmp_path):
    from pda_amd import ops, synthetic
    from pda_amd.bpr_pc import get_dataset_tot_popularity_for_PC
    toy = str(tmp_path / "data") + "/"
    synthetic.write_dataset(toy + "toy", n_users=2600, n_items=300, mean_hist=10)
    save = str(tmp_path / "save") + "/"
    _cli("pda_amd.train_new_api", toy, save)
    out = _cli("pda_amd.bpr_pc", toy, save, ("--pc_alpha", "0.5", "--pc_beta", "0.3"))
    order = ["popularity information-- mean:", "valid in valid set", "loading prtraining model", "pc model: 300", "do not consider popularity",
             "BPR result of valuation:", "BPR-PC result of valuation:", "BPR result of testing", "BPR-PC result of testing:"]
    pos = [out.index(x) for x in order]
    assert pos == sorted(pos), out
    lines = [l for l in out.splitlines() if l.startswith("||----")]
    assert len(lines) == 4
    rec = [float(re.search(r"recall=\[([0-9.]+)", l).group(1)) for l in lines]

    ck = [os.path.join(dp, f) for dp, _, fs in os.walk(save) for f in fs if f == "best_ckpt.ckpt"]
    assert len(ck) == 1
    t, data, model = _model(dev, toy)
    model.Recommender.load_state_dict(torch.load(ck[0], map_location=dev))
    for where, line in (("valid", lines[0]), ("test", lines[2])):                 # the BPR lines: main_branch on the checkpoint
        ev = t.evaluation(data, [20, 50], dev)
        ev.set_evaluate_obj_pre(where)
        r = ev.eval(model, None, rec_type="main_branch")
        assert line == "||---------------------------------------------- recall=[%.5f, %.5f], precision=[%.5f, %.5f], hit=[%.5f, %.5f], ndcg=[%.5f, %.5f]" % (
            r["recall"][0], r["recall"][-1], r["precision"][0], r["precision"][-1], r["hit_ratio"][0], r["hit_ratio"][-1], r["ndcg"][0], r["ndcg"][-1])

    # the BPR-PC test recall@20 from the checkpoint's tables and the library's k_u
    pop = get_dataset_tot_popularity_for_PC(data)
    users = np.asarray(list(data.test_user_list.keys()), dtype=np.int32)
    rows = [np.asarray(data.train_user_list[u], np.int64) for u in users]
    ip, ix, _ = data.train_csr(dev)
    k = ops.pc_user_stats(*model.Recommender.score_tables(), *to(dev, users, pop.astype(f32)), 0.3, ops.HistoryCSR(ip, ix, True))[2].cpu().numpy()
    U, I = (x.cpu().numpy() for x in model.Recommender.score_tables())
    top, _, _ = oracle_lists(U, I, users, rows, pop, k, 0.5, 0.3, 50, 2048)
    rec20 = np.mean([len(set(top[r, :20]) & set(data.test_user_list[u])) / len(data.test_user_list[u]) for r, u in enumerate(users)])
    assert rec[3] == pytest.approx(rec20, abs=6e-6)
