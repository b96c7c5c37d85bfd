"""GPU: xQuAD (`python -m pda_amd.xquad`, include/pda_hip_xquad.h) -- pda_xquad_rerank against the numpy restatement of tests/xquad_ref.py (the
naive arg-max over all unpicked candidates at every step), ids and values bit for bit on every row, and the driver end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from xquad_ref import valid_prefix, xquad_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
N_ITEMS = 5000
LAMBDAS = (0.0, 0.1, 0.5, 0.9, 1.0)


def to(dev, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


def csr(rows, dev, by_user):
    from pda_amd import ops
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    flat = np.concatenate([np.sort(np.asarray(r, np.int64)) for r in rows]).astype(np.int32) if rows else np.zeros(0, np.int32)
    return ops.HistoryCSR(*to(dev, indptr, flat), by_user=by_user)


def candidates(rng, R, N, n_items=N_ITEMS, ties=True):
    """Distinct ids per row, values descending (rounded to halves: many ties)."""
    idx = np.argsort(rng.random((R, n_items)), axis=1)[:, :N].astype(np.int32)
    val = -np.sort(-rng.standard_normal((R, N)).astype(f32) * f32(2), axis=1)
    if ties:
        val = (np.round(val * 2) / 2).astype(f32)
    return idx, val


def histories(rng, n_rows, n_items=N_ITEMS):
    """Rows of 0 .. 40 entries, some of them twice or three times."""
    out = []
    for r in range(n_rows):
        h = rng.integers(0, n_items, rng.integers(0, 41))
        if r % 3 == 0 and len(h):
            h = np.concatenate([h, h[:3], h[:1]])
        out.append(h)
    return out


def run(dev, idx, val, is_head, lam, K, variant, hist=None, users=None):
    from pda_amd import ops
    ti, tv, th = to(dev, idx, val, is_head)
    tu = to(dev, users)[0] if users is not None else None
    gi, gv = ops.xquad_rerank(ti, tv, th, lam, K, variant, tu, hist)
    assert gi.shape == (idx.shape[0], K) and gi.dtype == torch.int32 and gv.dtype == torch.float32
    return gi.cpu().numpy(), gv.cpu().numpy()


def check(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


SHAPES = [(N, K) for N in (1, 50, 63, 64, 65, 100, 1000, 1024) for K in (1, 20, 50, 64) if K <= N]


@pytest.mark.parametrize("variant", ["smooth", "binary"])
@pytest.mark.parametrize("N, K", SHAPES)
def test_lists_bit_exact(dev, N, K, variant):
    """67 rows (the last workgroup holds three), the history by user id and by block row with duplicate entries, values with ties."""
    rng = np.random.default_rng(1000 * N + 10 * K + len(variant))
    R, n_users = 67, 150
    lam = LAMBDAS[(N + K + len(variant)) % 5]
    idx, val = candidates(rng, R, N)
    is_head = (rng.random(N_ITEMS) < 0.3).astype(np.uint8)
    users = rng.permutation(n_users)[:R].astype(np.int32)
    hist = histories(rng, n_users)
    rows = [hist[u] for u in users]
    want = xquad_ref(idx, val, is_head, rows, lam, K, variant)
    check(run(dev, idx, val, is_head, lam, K, variant, csr(hist, dev, True), users), want)
    check(run(dev, idx, val, is_head, lam, K, variant, csr(rows, dev, False)), want)
    if lam > 0 and N >= 50 and K >= 20:
        assert (want[0] != idx[:, :K]).any(), "the case should change the order of some row"


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("R", [1, 3, 257])
def test_row_counts_and_every_lambda(dev, R, lam):
    rng = np.random.default_rng(R + int(10 * lam))
    idx, val = candidates(rng, R, 300)
    is_head = (rng.random(N_ITEMS) < 0.2).astype(np.uint8)
    rows = histories(rng, R)
    for variant in ("smooth", "binary"):
        check(run(dev, idx, val, is_head, lam, 50, variant, csr(rows, dev, False)), xquad_ref(idx, val, is_head, rows, lam, 50, variant))


@pytest.mark.parametrize("suffix", ["minus_one", "large_id", "minus_inf", "nan"])
@pytest.mark.parametrize("N, K", [(100, 20), (1000, 50), (64, 64)])
def test_short_rows(dev, N, K, suffix):
    """n_valid in {0, 1, K - 1, K, N} and at chunk boundaries, in the middle and one before the end of the row: the outputs end in -1 / -inf."""
    rng = np.random.default_rng(N + K + len(suffix))
    ends = sorted({0, 1, K - 1, K, N, 63, 64, 65, 128, N // 2, N - 1} & set(range(N + 1)))
    R = 3 * len(ends)
    idx, val = candidates(rng, R, N)
    for r in range(R):
        nv = ends[r % len(ends)]
        if suffix == "minus_one":
            idx[r, nv:] = -1
        elif suffix == "large_id":
            idx[r, nv:] = N_ITEMS + np.arange(N - nv) * (2 ** 31 // N - 8)      # from n_items up to near 2^31
        elif suffix == "minus_inf":
            val[r, nv:] = -np.inf
        else:
            val[r, nv:] = np.nan
    assert sorted(set(valid_prefix(idx, val, N_ITEMS).tolist())) == ends
    is_head = (rng.random(N_ITEMS) < 0.4).astype(np.uint8)
    rows = histories(rng, R)
    for variant in ("smooth", "binary"):
        want = xquad_ref(idx, val, is_head, rows, 0.5, K, variant)
        got = run(dev, idx, val, is_head, 0.5, K, variant, csr(rows, dev, False))
        check(got, want)
        for r in range(R):
            n = min(K, ends[r % len(ends)])
            assert (got[0][r, :n] >= 0).all() and (got[0][r, n:] == -1).all() and np.isneginf(got[1][r, n:]).all() and np.isfinite(got[1][r, :n]).all()


@pytest.mark.parametrize("head", [0, 1])
def test_candidates_of_one_category(dev, head):
    """All head or all tail: every chunk of the row is read, and the order of the candidates stays."""
    rng = np.random.default_rng(head)
    idx, val = candidates(rng, 40, 1000)
    is_head = np.full(N_ITEMS, head, np.uint8)
    rows = histories(rng, 40)
    for variant in ("smooth", "binary"):
        got = run(dev, idx, val, is_head, 0.5, 50, variant, csr(rows, dev, False))
        check(got, xquad_ref(idx, val, is_head, rows, 0.5, 50, variant))
        np.testing.assert_array_equal(got[0], idx[:, :50])


def test_empty_history_keeps_the_first_k(dev):
    rng = np.random.default_rng(8)
    idx, val = candidates(rng, 50, 200)
    is_head = (rng.random(N_ITEMS) < 0.3).astype(np.uint8)
    rows = [np.zeros(0, np.int64) if r % 2 else np.array([N_ITEMS + 5, -3]) for r in range(50)]      # empty, or ids outside the catalogue only
    rows[0] = np.array([7])
    for lam in LAMBDAS:
        for variant in ("smooth", "binary"):
            got = run(dev, idx, val, is_head, lam, 50, variant, csr(rows, dev, False))
            check(got, xquad_ref(idx, val, is_head, rows, lam, 50, variant))
            np.testing.assert_array_equal(got[0][1:], idx[1:, :50])
            none = run(dev, idx, val, is_head, lam, 50, variant)                                     # no history at all
            check(none, xquad_ref(idx, val, is_head, None, lam, 50, variant))
            np.testing.assert_array_equal(none[0], idx[:, :50])


@pytest.mark.parametrize("head", [0, 1])
def test_history_of_one_category(dev, head):
    rng = np.random.default_rng(20 + head)
    idx, val = candidates(rng, 60, 500)
    is_head = (rng.random(N_ITEMS) < 0.3).astype(np.uint8)
    pool = np.nonzero(is_head == head)[0]
    rows = [rng.choice(pool, 1 + r % 20) for r in range(60)]
    for variant in ("smooth", "binary"):
        check(run(dev, idx, val, is_head, 0.9, 50, variant, csr(rows, dev, False)), xquad_ref(idx, val, is_head, rows, 0.9, 50, variant))


def test_all_values_equal(dev):
    """rng = 0: the picks follow the bonus, then the position."""
    rng = np.random.default_rng(31)
    idx, val = candidates(rng, 60, 130)
    val[:] = f32(-1.75)
    is_head = (rng.random(N_ITEMS) < 0.5).astype(np.uint8)
    rows = histories(rng, 60)
    for variant in ("smooth", "binary"):
        got = run(dev, idx, val, is_head, 0.5, 64, variant, csr(rows, dev, False))
        check(got, xquad_ref(idx, val, is_head, rows, 0.5, 64, variant))
    assert (got[0] != idx[:, :64]).any()


def test_lambda_zero_and_one(dev):
    rng = np.random.default_rng(41)
    idx, val = candidates(rng, 80, 1000)
    idx[5, 30:] = -1
    is_head = (rng.random(N_ITEMS) < 0.3).astype(np.uint8)
    rows = histories(rng, 80)
    h = csr(rows, dev, False)
    for variant in ("smooth", "binary"):
        got = run(dev, idx, val, is_head, 0.0, 50, variant, h)
        check(got, xquad_ref(idx, val, is_head, rows, 0.0, 50, variant))
        np.testing.assert_array_equal(got[0][np.arange(80) != 5], idx[np.arange(80) != 5, :50])      # lambda = 0: the candidates' order
        np.testing.assert_array_equal(got[0][5, :30], idx[5, :30])
        got = run(dev, idx, val, is_head, 1.0, 50, variant, h)
        check(got, xquad_ref(idx, val, is_head, rows, 1.0, 50, variant))
        flat = val.copy()
        flat[:] = f32(3)                                                                               # lambda = 1: relevance is ignored
        flat[5, 30:] = -np.inf
        np.testing.assert_array_equal(run(dev, idx, flat, is_head, 1.0, 50, variant, h)[0], got[0])


@pytest.mark.parametrize("N", [63, 257])
def test_rows_off_16_byte_boundaries(dev, N):
    from pda_amd import ops
    rng = np.random.default_rng(N)
    R, K = 33, 50
    idx, val = candidates(rng, R, N)
    is_head = (rng.random(N_ITEMS) < 0.3).astype(np.uint8)
    rows = histories(rng, R)
    want = xquad_ref(idx, val, is_head, rows, 0.5, K, "smooth")
    th = to(dev, is_head)[0]
    h = csr(rows, dev, False)
    for off in (1, 2, 3):                                                       # the buffers start 4, 8 and 12 bytes behind a 16-byte boundary
        bi = torch.zeros(R * N + off, dtype=torch.int32, device=dev)
        bv = torch.zeros(R * N + off, dtype=torch.float32, device=dev)
        ti, tv = bi[off:].view(R, N), bv[off:].view(R, N)
        ti.copy_(torch.from_numpy(idx))
        tv.copy_(torch.from_numpy(val))
        assert ti.data_ptr() % 16 == 4 * off
        gi, gv = ops.xquad_rerank(ti, tv, th, 0.5, K, "smooth", None, h)
        check((gi.cpu().numpy(), gv.cpu().numpy()), want)


def test_non_default_stream(dev):
    from pda_amd import ops
    rng = np.random.default_rng(77)
    idx, val = candidates(rng, 100, 1000)
    is_head = (rng.random(N_ITEMS) < 0.3).astype(np.uint8)
    rows = histories(rng, 100)
    want = xquad_ref(idx, val, is_head, rows, 0.5, 50, "smooth")
    ti, tv, th = to(dev, idx, val, is_head)
    h = csr(rows, dev, False)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gi, gv = ops.xquad_rerank(ti, tv, th, 0.5, 50, "smooth", None, h)
    s.synchronize()
    check((gi.cpu().numpy(), gv.cpu().numpy()), want)


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
    """The toy of tests/test_gpu_bpr_pc.py (300 items: room for 100 candidates), trained for two epochs."""
    from pda_amd import synthetic
    base = tmp_path_factory.mktemp("xquad")
    toy, save = str(base / "data") + "/", str(base / "save") + "/"
    synthetic.write_dataset(toy + "toy", n_users=2600, n_items=300, mean_hist=10)
    _cli("pda_amd.train_new_api", toy, save)
    return toy, save


def test_cli_lambda_zero_prints_the_bpr_lines(dev, trained):
    toy, save = trained
    out = _cli("pda_amd.xquad", toy, save, ("--xq_lambda", "0", "--xq_candidates", "100", "--deterministic", "1"))
    order = ["valid in valid set", "loading prtraining model", "xquad model: 300", "BPR result of valuation:", "xQuAD result of valuation:",
             "BPR result of testing", "xQuAD result of testing:"]
    pos = [out.index(x) for x in order]
    assert pos == sorted(pos), out
    lines = [l for l in out.splitlines() if l.startswith("||----")]
    assert len(lines) == 8 and ["recall=" in l for l in lines] == [True, False] * 4 and all("aplt@[20, 50]=" in l for l in lines[1::2])
    assert lines[0] == lines[2] and lines[1] == lines[3] and lines[4] == lines[6] and lines[5] == lines[7]


def test_driver_end_to_end(dev, trained):
    from pda_amd import train_new_api as t
    from pda_amd import xquad
    toy, save = trained
    argv = ["--data_path", toy, "--save_dir", save, *FLAGS, "--deterministic", "1"]
    # lambda = 0: the xQuAD metrics are the BPR metrics, exactly (the ordered reduction: the same rows in the same order give the same bits)
    res = xquad.main(argv + ["--xq_lambda", "0", "--xq_candidates", "100"])
    for where in ("valid", "test"):
        for key in ("recall", "precision", "ndcg", "hit_ratio"):
            np.testing.assert_array_equal(res[where]["xquad"][key], res[where]["bpr"][key])
        np.testing.assert_array_equal(res[where]["aplt_xquad"], res[where]["aplt_bpr"])

    # lambda = 0.5 over the short and the deep candidate route: the lists are the reference's on the model's own candidates
    res = xquad.main(argv + ["--xq_lambda", "0.5", "--xq_candidates", "100"])
    ck = [os.path.join(dp, f) for dp, _, fs in os.walk(save) for f in fs if f == "best_ckpt.ckpt"]
    assert len(ck) == 1
    t.configure(argv)
    data = t.data
    model = t.DatasetApi_Model(t.args, {"n_users": data.n_users, "n_items": data.n_items}, 256, None, dev)
    model.Recommender.load_state_dict(torch.load(ck[0], map_location=dev))
    is_head = xquad.head_items(xquad.train_counts(data), 0.8)
    assert 0 < is_head.sum() < data.n_items
    ev = t.evaluation(data, [20, 50], dev)
    ev.set_evaluate_obj_pre("test")
    users = ev.users_dev.cpu().numpy()
    rows = [data.train_user_list[u] for u in users]
    changed = 0
    for nc in (30, 100):
        for variant in ("smooth", "binary"):
            xq = xquad.XQuAD_model(model, 50 if nc >= 50 else 20, 0.5, nc, is_head, variant)
            cidx, cval = xq.candidates(ev.users_dev, ev._hist)
            assert cidx.shape == (len(users), nc)
            got = xq.recommend_device(ev.users_dev, None, "main_branch", None, ev._hist)
            want = xquad_ref(cidx.cpu().numpy(), cval.cpu().numpy(), is_head, rows, 0.5, xq.topk, variant)
            check((got[0].cpu().numpy(), got[1].cpu().numpy()), want)
            changed += int((want[0] != cidx.cpu().numpy()[:, :xq.topk]).any())
            if nc == 100 and variant == "smooth":
                lists = want[0]
                tail = (lists >= 0) & (is_head[np.clip(lists, 0, None)] == 0)
                count = np.array([tail[:, :k].sum(axis=1).mean() / k for k in (20, 50)])
                np.testing.assert_allclose(xquad.aplt(got[0], xq.is_head, [20, 50]), count, rtol=1e-12)
                np.testing.assert_allclose(res["test"]["aplt_xquad"], count, rtol=1e-12)             # the driver's figure (--xq_variant smooth)
    assert changed == 4
