"""GPU: calibrated popularity (`python -m pda_amd.calib`, include/pda_hip_calib.h) -- pda_calib_rerank against the float64 numpy restatement of
tests/calib_ref.py (the naive arg-max over all unpicked candidates at every step): ids, values and divergences bit for bit on every row the
reference does not flag as fragile (a divergence within 2^-40 of a boundary of the 2^-20 grid; at most two rows of a case); pda_calib_profile
and pda_calib_list_counts against numpy exactly; and the driver end to end."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import calib_cases as cc
from calib_ref import calib_ref, list_counts_ref, profile_ref, valid_prefix

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
N_ITEMS = cc.N_ITEMS


def to(dev, *xs):
    return [torch.from_numpy(np.array(x)).to(dev) for x in xs]      # (a copy: the shared cases are read-only)


def csr(rows, dev, by_user):
    from pda_amd import ops
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    flat = np.concatenate([np.sort(np.asarray(r, np.int64)) for r in rows]).astype(np.int32) if rows else np.zeros(0, np.int32)
    return ops.HistoryCSR(*to(dev, indptr, flat), by_user=by_user)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def check(got, want, fragile=None):
    """Bit for bit on the rows that are not fragile (-0.0 and 0.0 differ here)."""
    keep = np.ones(got[0].shape[0], bool) if fragile is None else ~fragile
    for g, w in zip(got, want):
        np.testing.assert_array_equal(bits(g)[keep], bits(w)[keep])


def rerank(dev, idx, val, prof, item_group, G, lam, K, div, alpha=cc.ALPHA):
    from pda_amd import ops
    ti, tv, tp, tg = to(dev, idx, val, np.asarray(prof, np.int32), item_group)
    gi, gv, gd = ops.calib_rerank(ti, tv, tp, tg, G, lam, K, div, alpha)
    assert gi.shape == gv.shape == gd.shape == (idx.shape[0], K)
    assert gi.dtype == torch.int32 and gv.dtype == torch.float32 and gd.dtype == torch.float32
    return gi.cpu().numpy(), gv.cpu().numpy(), gd.cpu().numpy()


def reference(idx, val, prof, item_group, G, lam, K, div, alpha=cc.ALPHA):
    wi, wv, wd, fragile = calib_ref(idx, val, prof, item_group, G, lam, K, div, alpha)
    assert fragile.sum() <= cc.MAX_FRAGILE, "change the seed: %d fragile rows" % fragile.sum()
    return (wi, wv, wd), fragile


def setup(seed, R, N, G, ties=True):
    rng = np.random.default_rng(seed)
    counts = cc.long_tail_counts(rng)
    item_group = cc.groups_of(counts, G)
    idx, val = cc.candidates(rng, R, N, ties=ties)
    rows = cc.histories(rng, R, counts)
    return rng, counts, item_group, idx, val, rows, profile_ref(rows, item_group, G)


# ---- the shared cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, K, G, div, lam", cc.CASES, ids=cc.CASE_IDS)
def test_lists_bit_exact(dev, N, K, G, div, lam):
    """The profile by user id and by block row (duplicate entries), then the selection from it: every non-fragile row bit for bit."""
    from pda_amd import ops
    c = cc.case(N, K, G, div, lam)
    assert c["fragile"].sum() <= cc.MAX_FRAGILE
    tg, tu = to(dev, c["item_group"], c["users"])
    by_user = ops.calib_profile(tg, G, cc.ROWS, tu, csr(c["hist"], dev, True)).cpu().numpy()
    by_row = ops.calib_profile(tg, G, cc.ROWS, None, csr(c["rows"], dev, False)).cpu().numpy()
    np.testing.assert_array_equal(by_user, c["prof"])
    np.testing.assert_array_equal(by_row, c["prof"])
    for prof in (by_user, by_row):
        check(rerank(dev, c["idx"], c["val"], prof, c["item_group"], G, lam, K, div), c["want"], c["fragile"])
    if lam > 0 and N >= 50 and K >= 20:
        assert (c["want"][0] != c["idx"][:, :K]).any(), "the case should change the order of some row"


# ---- profile and list counts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", cc.GROUPS)
def test_profile_equals_numpy(dev, G):
    from pda_amd import ops
    rng = np.random.default_rng(G)
    counts = cc.long_tail_counts(rng)
    item_group = cc.groups_of(counts, G).copy()
    item_group[rng.integers(0, N_ITEMS, 300)] = rng.integers(G, 256, 300)                 # items of no group
    rows = cc.histories(rng, 300, counts)
    rows[3] = np.zeros(0, np.int64)
    rows[4] = np.array([-5, N_ITEMS, N_ITEMS + 7, 2 ** 31 - 1])                          # outside the catalogue only
    rows[5] = np.concatenate([rng.integers(0, N_ITEMS, 200), [7] * 70])                  # longer than a chunk, a run of duplicates across chunks
    rows[6] = np.full(130, 11)
    want = profile_ref(rows, item_group, G)
    tg = to(dev, item_group)[0]
    np.testing.assert_array_equal(ops.calib_profile(tg, G, 300, None, csr(rows, dev, False)).cpu().numpy(), want)
    users = rng.permutation(300).astype(np.int32)[:257]
    got = ops.calib_profile(tg, G, 257, to(dev, users)[0], csr(rows, dev, True)).cpu().numpy()
    np.testing.assert_array_equal(got, want[users])
    assert want[3].sum() == 0 and want[4].sum() == 0 and want[6].sum() <= 1
    none = ops.calib_profile(tg, G, 5)                                                    # a NULL history
    assert none.dtype == torch.int32 and none.shape == (5, G) and not none.any()


@pytest.mark.parametrize("G, K, Ks", [(2, 50, [20, 50]), (3, 64, [1, 5, 63, 64]), (8, 1024, [1, 64, 65, 100, 128, 500, 1000, 1024]), (3, 130, [129]),
                                      (8, 1, [1])])
def test_list_counts_equal_numpy(dev, G, K, Ks):
    from pda_amd import ops
    rng = np.random.default_rng(K + G)
    item_group = cc.groups_of(cc.long_tail_counts(rng), G).copy()
    item_group[rng.integers(0, N_ITEMS, 300)] = rng.integers(G, 256, 300)
    R = 131
    idx = rng.integers(0, N_ITEMS, (R, K)).astype(np.int32)
    idx[rng.random((R, K)) < 0.1] = -1
    idx[rng.random((R, K)) < 0.05] = N_ITEMS + 3
    idx[0] = -1
    idx[1, K // 2:] = -1
    got = ops.calib_list_counts(*to(dev, idx, item_group), G, Ks)
    assert got.dtype == torch.int32 and got.shape == (R, len(Ks), G)
    np.testing.assert_array_equal(got.cpu().numpy(), list_counts_ref(idx, item_group, G, Ks))
    assert not got[0].any()


# ---- edge cases of the selection -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("suffix", ["minus_one", "large_id", "minus_inf", "nan", "no_group"])
@pytest.mark.parametrize("N, K, G", [(100, 20, 3), (1000, 50, 8), (64, 64, 2)])
def test_short_rows(dev, N, K, G, suffix):
    """n_valid in {0, 1, K - 1, K, N} and at chunk boundaries: the outputs end in -1 / -inf / -inf."""
    ends = sorted({0, 1, K - 1, K, N, 63, 64, 65, 128, N // 2, N - 1} & set(range(N + 1)))
    R = 3 * len(ends)
    rng = np.random.default_rng(N + K + len(suffix))
    counts = cc.long_tail_counts(rng)
    item_group = cc.groups_of(counts, G).copy()
    item_group[4000:] = G + np.arange(1000) % (256 - G)                                   # the last 1 000 items have no group ...
    idx, val = cc.candidates(rng, R, N, n_items=4000)                                     # ... and are no candidates
    rows = cc.histories(rng, R, counts)
    for r in range(R):
        nv = ends[r % len(ends)]
        if suffix == "minus_one":
            idx[r, nv:] = -1
        elif suffix == "large_id":
            idx[r, nv:] = N_ITEMS + np.arange(N - nv) * (2 ** 31 // N - 8)              # from n_items up to near 2^31
        elif suffix == "minus_inf":
            val[r, nv:] = -np.inf
        elif suffix == "nan":
            val[r, nv:] = np.nan
        else:
            idx[r, nv:] = 4000 + rng.permutation(1000)[:N - nv]
    assert sorted(set(valid_prefix(idx, val, item_group, G).tolist())) == ends
    prof = profile_ref(rows, item_group, G)
    for div in cc.DIVS:
        want, fragile = reference(idx, val, prof, item_group, G, 0.5, K, div)
        got = rerank(dev, idx, val, prof, item_group, G, 0.5, K, div)
        check(got, want, fragile)
        for r in range(R):
            n = min(K, ends[r % len(ends)])
            assert (got[0][r, :n] >= 0).all() and (got[0][r, n:] == -1).all() and np.isfinite(got[1][r, :n]).all() and np.isfinite(got[2][r, :n]).all()
            assert np.isneginf(got[1][r, n:]).all() and np.isneginf(got[2][r, n:]).all()


@pytest.mark.parametrize("G", cc.GROUPS)
def test_candidates_of_one_group(dev, G):
    """Every candidate in the last group: every chunk of the row is read, and the order of the candidates stays."""
    rng, counts, item_group, idx, val, rows, prof = setup(50 + G, 40, 1000, G)
    one = np.full(N_ITEMS, G - 1, np.uint8)
    for div in cc.DIVS:
        want, fragile = reference(idx, val, prof, one, G, 0.5, 50, div)
        got = rerank(dev, idx, val, prof, one, G, 0.5, 50, div)
        check(got, want, fragile)
        np.testing.assert_array_equal(got[0], idx[:, :50])


@pytest.mark.parametrize("G", cc.GROUPS)
def test_profile_of_one_group_and_no_profile(dev, G):
    rng, counts, item_group, idx, val, rows, prof = setup(60 + G, 60, 500, G)
    prof = np.zeros_like(prof)
    prof[np.arange(60), np.arange(60) % G] = 1 + np.arange(60) % 20
    prof[::7] = 0                                                                         # H = 0: the candidates' order
    for div in cc.DIVS:
        want, fragile = reference(idx, val, prof, item_group, G, 0.9, 50, div)
        got = rerank(dev, idx, val, prof, item_group, G, 0.9, 50, div)
        check(got, want, fragile)
        np.testing.assert_array_equal(got[0][::7], idx[::7, :50])
        assert not got[2][::7].any()
    assert (got[0] != idx[:, :50]).any()


def test_all_values_equal(dev):
    """rng = 0: the picks follow the divergence, then the position."""
    rng, counts, item_group, idx, val, rows, prof = setup(31, 60, 130, 3)
    val = np.full_like(val, f32(-1.75))
    for div in cc.DIVS:
        want, fragile = reference(idx, val, prof, item_group, 3, 0.5, 64, div)
        got = rerank(dev, idx, val, prof, item_group, 3, 0.5, 64, div)
        check(got, want, fragile)
    assert (got[0] != idx[:, :64]).any()


def test_lambda_zero_and_one(dev):
    rng, counts, item_group, idx, val, rows, prof = setup(41, 80, 1000, 3)
    idx[5, 30:] = -1
    for div in cc.DIVS:
        want, fragile = reference(idx, val, prof, item_group, 3, 0.0, 50, div)
        got = rerank(dev, idx, val, prof, item_group, 3, 0.0, 50, div)
        check(got, want, fragile)
        np.testing.assert_array_equal(got[0][np.arange(80) != 5], idx[np.arange(80) != 5, :50])      # lambda = 0: the candidates' order
        np.testing.assert_array_equal(got[0][5, :30], idx[5, :30])
        want, fragile = reference(idx, val, prof, item_group, 3, 1.0, 50, div)
        got = rerank(dev, idx, val, prof, item_group, 3, 1.0, 50, div)
        check(got, want, fragile)
        flat = np.full_like(val, f32(3))                                                             # lambda = 1: relevance is ignored
        flat[5, 30:] = -np.inf
        np.testing.assert_array_equal(rerank(dev, idx, flat, prof, item_group, 3, 1.0, 50, div)[0][~fragile], got[0][~fragile])


@pytest.mark.parametrize("R", [1, 3, 257])
def test_row_counts(dev, R):
    rng, counts, item_group, idx, val, rows, prof = setup(R, R, 300, 8)
    for div in cc.DIVS:
        want, fragile = reference(idx, val, prof, item_group, 8, 0.5, 50, div)
        check(rerank(dev, idx, val, prof, item_group, 8, 0.5, 50, div), want, fragile)


@pytest.mark.parametrize("N", [63, 257])
def test_rows_off_16_byte_boundaries(dev, N):
    from pda_amd import ops
    R, K, G = 33, 50, 3
    rng, counts, item_group, idx, val, rows, prof = setup(N, R, N, G)
    want, fragile = reference(idx, val, prof, item_group, G, 0.5, K, "js")
    tg, tp = to(dev, item_group, prof)
    for off in (1, 2, 3):                                                       # the buffers start 4, 8 and 12 bytes behind a 16-byte boundary
        bi = torch.zeros(R * N + off, dtype=torch.int32, device=dev)
        bv = torch.zeros(R * N + off, dtype=torch.float32, device=dev)
        ti, tv = bi[off:].view(R, N), bv[off:].view(R, N)
        ti.copy_(torch.from_numpy(idx))
        tv.copy_(torch.from_numpy(val))
        assert ti.data_ptr() % 16 == 4 * off
        got = ops.calib_rerank(ti, tv, tp, tg, G, 0.5, K, "js")
        check([g.cpu().numpy() for g in got], want, fragile)


def test_non_default_stream(dev):
    from pda_amd import ops
    rng, counts, item_group, idx, val, rows, prof = setup(77, 100, 1000, 3)
    want, fragile = reference(idx, val, prof, item_group, 3, 0.5, 50, "kl")
    ti, tv, tp, tg = to(dev, idx, val, prof, item_group)
    h = csr(rows, dev, False)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gp = ops.calib_profile(tg, 3, 100, None, h)
        got = ops.calib_rerank(ti, tv, gp, tg, 3, 0.5, 50, "kl", cc.ALPHA)
        cnt = ops.calib_list_counts(got[0], tg, 3, [20, 50])
    s.synchronize()
    np.testing.assert_array_equal(gp.cpu().numpy(), prof)
    check([g.cpu().numpy() for g in got], want, fragile)
    np.testing.assert_array_equal(cnt.cpu().numpy(), list_counts_ref(want[0], item_group, 3, [20, 50]))


@pytest.mark.parametrize("div", cc.DIVS)
def test_every_slot_is_written_whatever_the_buffers_held(dev, div):
    """Through the binding itself: outputs pre-filled with 0x00, 0xFF and 0xA5 give the same bits, tails included, with and without out_div."""
    from pda_amd import _lib
    lib = _lib.load()
    R, N, K, G = 37, 200, 50, 3
    rng, counts, item_group, idx, val, rows, prof = setup(5 + len(div), R, N, G)
    idx[::4, 7:] = -1                                                            # short rows: tails of -1 / -inf / -inf
    idx[1] = -1
    want, fragile = reference(idx, val, prof, item_group, G, 0.5, K, div)
    ti, tv, tp, tg = to(dev, idx, val, prof, item_group)
    null = C.c_void_p(None)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    seen = []
    for fill in (0x00, 0xFF, 0xA5):
        for with_div in (True, False):
            oi, ov, od = (torch.full((4 * R * K,), fill, dtype=torch.uint8, device=dev).view(dt).view(R, K)
                          for dt in (torch.int32, torch.float32, torch.float32))
            rc = lib.pda_calib_rerank(_lib.ptr(ti), _lib.ptr(tv), R, N, _lib.ptr(tp), _lib.ptr(tg), N_ITEMS, G, 0.5,
                                      _lib.CALIB_JS if div == "js" else _lib.CALIB_KL, cc.ALPHA, K,
                                      _lib.ptr(oi), _lib.ptr(ov), _lib.ptr(od) if with_div else null, stream)
            assert rc == 0
            torch.cuda.synchronize()
            got = (oi.cpu().numpy(), ov.cpu().numpy(), od.cpu().numpy())
            check(got[:2], want[:2], fragile)
            if with_div:
                check(got[2:], want[2:], fragile)
                seen.append(got)
            else:
                assert (got[2].view(np.uint8) == fill).all()                     # a NULL out_div: nothing of it is touched
            assert (got[0][1] == -1).all() and np.isneginf(got[1][1]).all()
    for got in seen[1:]:
        check(got, seen[0])                                                      # fragile rows too: the same bits whatever the buffers held


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
FLAGS = ["--dataset", "toy", "--train", "normal", "--test", "normal", "--epoch", "2", "--log_interval", "1", "--batch_size", "256", "--lr", "1e-2",
         "--regs", "1e-2", "--valid_set", "valid", "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t", "--cuda", "0"]


def _cli(module, toy, save, extra=()):
    argv = [sys.executable, "-m", module, "--data_path", toy, "--save_dir", save, *FLAGS, *extra]
    r = subprocess.run(argv, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.fixture(scope="module")
def trained(dev, tmp_path_factory):
    """The toy of tests/test_gpu_xquad.py (2 600 users x 300 items: room for 100 candidates), trained for two epochs."""
    from pda_amd import synthetic
    base = tmp_path_factory.mktemp("calib")
    toy, save = str(base / "data") + "/", str(base / "save") + "/"
    synthetic.write_dataset(toy + "toy", n_users=2600, n_items=300, mean_hist=10)
    _cli("pda_amd.train_new_api", toy, save)
    return toy, save


def test_cli_lambda_zero_prints_the_bpr_lines(dev, trained):
    toy, save = trained
    out = _cli("pda_amd.calib", toy, save, ("--cp_lambda", "0", "--cp_candidates", "100", "--deterministic", "1"))
    order = ["valid in valid set", "loading prtraining model", "calib model: 300", "BPR result of valuation:", "CP result of valuation:",
             "BPR result of testing", "CP result of testing:"]
    pos = [out.index(x) for x in order]
    assert pos == sorted(pos), out
    lines = [l for l in out.splitlines() if l.startswith("||----")]
    assert len(lines) == 8 and ["recall=" in l for l in lines] == [True, False] * 4
    assert all("upd@[20, 50]=[" in l and " users=" in l for l in lines[1::2])
    assert lines[0] == lines[2] and lines[1] == lines[3] and lines[4] == lines[6] and lines[5] == lines[7]


def test_cli_takes_the_bias_report_and_the_kl_divergence(dev, trained):
    toy, save = trained
    out = _cli("pda_amd.calib", toy, save, ("--cp_lambda", "0.5", "--cp_candidates", "100", "--cp_div", "kl", "--cp_cuts", "[0.5]", "--bias_report", "1"))
    assert "calib model: 300 items per group: [" in out and out.count("||--- bias@") >= 4
    lines = [l for l in out.splitlines() if "upd@[20, 50]=[" in l]
    assert len(lines) == 4 and lines[0] != lines[1] and lines[2] != lines[3]


def test_driver_end_to_end(dev, trained):
    from pda_amd import calib
    from pda_amd import train_new_api as t
    from pda_amd.xquad import train_counts
    toy, save = trained
    argv = ["--data_path", toy, "--save_dir", save, *FLAGS, "--deterministic", "1"]
    # lambda = 0: the CP metrics are the BPR metrics, exactly (the ordered reduction: the same rows in the same order give the same bits)
    res = calib.main(argv + ["--cp_lambda", "0", "--cp_candidates", "100"])
    for where in ("valid", "test"):
        for key in ("recall", "precision", "ndcg", "hit_ratio"):
            np.testing.assert_array_equal(res[where]["cp"][key], res[where]["bpr"][key])
        np.testing.assert_array_equal(res[where]["upd_cp"], res[where]["upd_bpr"])

    # lambda = 0.5 over the short and the deep candidate route: the lists are the reference's on the model's own candidates
    res = calib.main(argv + ["--cp_lambda", "0.5", "--cp_candidates", "100"])
    ck = [os.path.join(dp, f) for dp, _, fs in os.walk(save) for f in fs if f == "best_ckpt.ckpt"]
    assert len(ck) == 1
    t.configure(argv)
    data = t.data
    model = t.DatasetApi_Model(t.args, {"n_users": data.n_users, "n_items": data.n_items}, 256, None, dev)
    model.Recommender.load_state_dict(torch.load(ck[0], map_location=dev))
    item_group = calib.cut_groups(train_counts(data), [0.2, 0.8])
    assert all((item_group == g).any() for g in range(3))
    ev = t.evaluation(data, [20, 50], dev)
    ev.set_evaluate_obj_pre("test")
    users = ev.users_dev.cpu().numpy()
    rows = [data.train_user_list[u] for u in users]
    prof = profile_ref(rows, item_group, 3)
    changed = 0
    for nc in (30, 100):
        for div in cc.DIVS:
            cp = calib.Calib_model(model, 50 if nc >= 50 else 20, 0.5, nc, item_group, 3, div, 0.01)
            cidx, cval = cp.candidates(ev.users_dev, ev._hist)
            assert cidx.shape == (len(users), nc)
            np.testing.assert_array_equal(cp.profile(ev.users_dev, ev._hist).cpu().numpy(), prof)
            got = cp.recommend_device(ev.users_dev, None, "main_branch", None, ev._hist)
            wi, wv, wd, fragile = calib_ref(cidx.cpu().numpy(), cval.cpu().numpy(), prof, item_group, 3, 0.5, cp.topk, div, 0.01)
            assert fragile.sum() <= max(cc.MAX_FRAGILE, len(users) // 32)
            check((got[0].cpu().numpy(), got[1].cpu().numpy()), (wi, wv), fragile)
            changed += int((wi != cidx.cpu().numpy()[:, :cp.topk]).any())
            if nc == 100 and div == "js":
                lists = np.where(fragile[:, None], got[0].cpu().numpy(), wi)                         # (a fragile row: the reference cannot decide)
                want_upd, want_rows = calib.upd(prof, list_counts_ref(lists, item_group, 3, [20, 50]))
                np.testing.assert_allclose(res["test"]["upd_cp"], want_upd, rtol=0, atol=1e-12)      # the driver's figure (--cp_div js)
                np.testing.assert_array_equal(res["test"]["upd_users_cp"], want_rows)
    assert changed == 4

    # lambda = 0.9: the lists follow the users' popularity mix more closely than the model's own
    res = calib.main(argv + ["--cp_lambda", "0.9", "--cp_candidates", "100"])
    for where in ("valid", "test"):
        assert (res[where]["upd_cp"] < res[where]["upd_bpr"]).all(), (where, res[where]["upd_cp"], res[where]["upd_bpr"])
