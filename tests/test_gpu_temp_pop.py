"""GPU: BPRMF(t)-pop (`--train temp_pop`) -- the fused step of the four tables, the Adam sweep over them, the bias-head score kernel and the
trainer end to end, against the float64 restatement of tests/temp_pop_ref.py and the CPU oracle."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import c_oracle
from temp_pop_ref import adam_steps, forward_grads, item_beta, scores_bias

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def to(dev, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


def make(rng, nU, nI, d, T, B, kind):
    U = (rng.standard_normal((nU, d)) * 0.2).astype(np.float32)
    I = (rng.standard_normal((nI, d)) * 0.2).astype(np.float32)
    bu = (rng.standard_normal((nU, 1)) * 0.3).astype(np.float32)
    Cm = (rng.standard_normal((nI, T + 1)) * 0.3).astype(np.float32)
    users = rng.integers(0, nU, B).astype(np.int32)             # repeated users
    pos = rng.integers(0, max(2, nI // 10), B).astype(np.int32)  # repeated positives
    neg = rng.integers(0, nI, B).astype(np.int32)
    if kind == "hot":
        pos[: B // 3] = 7                                        # one item a third of the batch
    lo = 1 if (kind == "no_stage0" and T > 1) else 0
    temps = rng.integers(lo, T, B).astype(np.float32)
    return U, I, bu, Cm, users, pos, neg, temps


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("T", [1, 3, 10])
@pytest.mark.parametrize("kind", ["mixed", "no_stage0", "hot"])
def test_step_loss_and_gradients(dev, d, T, kind):
    from pda_amd import ops
    rng = np.random.default_rng(d + 10 * T + len(kind))
    nU, nI, B, regs = 700, 500, 2048, 1e-2
    U, I, bu, Cm, users, pos, neg, temps = make(rng, nU, nI, d, T, B, kind)
    ref_loss, ref_g = forward_grads(U, I, bu, Cm, users, pos, neg, temps, regs, B)
    tabs = to(dev, U, I, bu, Cm)
    st = ops.TempPopState(*tabs)
    loss = torch.zeros(3, device=dev)
    ops.temp_pop_grads(*tabs, *to(dev, users, pos, neg, temps), st, regs=regs, reg_div=B, step=1, loss_acc=loss)
    np.testing.assert_allclose(loss.cpu().numpy(), ref_loss, rtol=1e-5, atol=1e-5)
    for g, r in zip(st.g, ref_g):
        # entries are ~1e-6 .. 1e-3: relative to each entry (fp32 atomics against float64), a floor far below the regulariser terms
        np.testing.assert_allclose(g.cpu().numpy(), r, rtol=1e-4, atol=1e-9)
    assert (st.tagU.cpu().numpy()[users] == 1).all() and (st.tagI.cpu().numpy()[np.concatenate([pos, neg])] == 1).all()
    for t, x in zip(tabs, (U, I, bu, Cm)):
        assert torch.equal(t.cpu(), torch.from_numpy(x))       # gradients only


@pytest.mark.parametrize("d, T", [(64, 10), (128, 3), (256, 1)])
def test_three_adam_steps_over_the_four_tables(dev, d, T):
    """Against the float64 restatement: every row moves (dense decay); 2e-5 (the convention of the existing Adam tests on repeated rows:
    atomics add in any order and Adam amplifies the residue of cancellations)."""
    from pda_amd import ops
    rng = np.random.default_rng(d + T)
    nU, nI, B, regs, lr = 900, 600, 1024, 1e-2, 1e-3
    U, I, bu, Cm, *_ = make(rng, nU, nI, d, T, B, "mixed")
    batches = [make(rng, nU, nI, d, T, B, "mixed")[4:] for _ in range(3)]
    want, want_losses = adam_steps([x.astype(np.float64) for x in (U, I, bu, Cm)], batches, regs, B, lr)
    tabs = to(dev, U, I, bu, Cm)
    st = ops.TempPopState(*tabs)
    for step, b in enumerate(batches, 1):
        loss = torch.zeros(3, device=dev)
        ops.temp_pop_adam_step(*tabs, *to(dev, *b), st, regs=regs, reg_div=B, step=step, lr_t=ops.adam_lr_t(lr, step), loss_acc=loss)
        np.testing.assert_allclose(loss.cpu().numpy(), want_losses[step - 1], rtol=1e-5, atol=1e-5)
    for t, w in zip(tabs, want):
        np.testing.assert_allclose(t.cpu().numpy(), w, atol=2e-5)
    for g in st.g:
        assert not g.cpu().numpy().any(), "the sweep clears the gradient accumulators behind itself"


def test_sweep_is_bit_exact_against_an_fp32_emulation(dev):
    """The sweep's per-element arithmetic (that of pda_adam_dense_sweep_f32) emulated in float32 on the gradients the step kernel produced:
    every element of all four tables and moments, bit for bit, over three steps -- touched rows and idle ones (g = 0, decay only)."""
    from pda_amd import ops
    rng = np.random.default_rng(3)
    nU, nI, d, B, T, regs, lr = 500, 300, 64, 512, 10, 1e-2, 1e-3
    U, I, bu, Cm, *_ = make(rng, nU, nI, d, T, B, "mixed")
    tabs = to(dev, U, I, bu, Cm)
    st = ops.TempPopState(*tabs)
    f = np.float32
    x = [t.cpu().numpy().copy() for t in tabs]
    m = [np.zeros_like(v) for v in x]
    v = [np.zeros_like(w) for w in x]
    b1, b2, eps = f(ops.ADAM_BETA1), f(ops.ADAM_BETA2), f(ops.ADAM_EPS)
    for step in (1, 2, 3):
        b = make(rng, nU, nI, d, T, B, "mixed")[4:]
        ops.temp_pop_grads(*tabs, *to(dev, *b), st, regs=regs, reg_div=B, step=step)
        g = [t.cpu().numpy().copy() for t in st.g]
        lr_t = f(ops.adam_lr_t(lr, step))
        ops.temp_pop_sweep(*tabs, st, step=step, lr_t=float(lr_t))
        for q in range(4):
            m[q] = b1 * m[q] + (f(1) - b1) * g[q]
            v[q] = b2 * v[q] + (f(1) - b2) * g[q] * g[q]
            x[q] = x[q] - lr_t * m[q] / (np.sqrt(v[q]) + eps)
        for q in range(4):
            np.testing.assert_array_equal(st.m[q].cpu().numpy(), m[q])
            np.testing.assert_array_equal(st.v[q].cpu().numpy(), v[q])
            np.testing.assert_array_equal(tabs[q].cpu().numpy(), x[q])


def oracle_bias_topk(U, I, users, alpha, beta, K, hist_rows):
    s = scores_bias(c_oracle.scores_chain(U, I, users), alpha, beta)
    for r, items in enumerate(hist_rows):
        s[r, items] = -np.inf
    return c_oracle.arg_topk_2d(s, K), s


KERNELS = {"exact": 1, "prefiltered": 3}      # PDA_TEMP_POP_KERNEL -> the generation whose identity the call must leave


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("K", [1, 20, 50])
@pytest.mark.parametrize("mode", ["user_id", "block_row"])
def test_bias_kernels_equal_the_oracle(dev, monkeypatch, kernel, d, K, mode):
    """Both kernels of the bias head return the oracle's keys (fp32 chain + fl(alpha beta), mask, top-K) bit for bit -- the pre-filtered
    one therefore the exact one's -- with negative alpha, a beta that dominates the dot, ties among those items, masked ones, and a
    catalogue that is not a multiple of any tile."""
    from pda_amd import ops
    monkeypatch.setenv("PDA_TEMP_POP_KERNEL", kernel)
    rng = np.random.default_rng(d + K + len(mode))
    nU, nI, nb = 900, 3001, 300                                  # n_items not a multiple of the tile
    U = (rng.standard_normal((nU, d)) * 0.1).astype(np.float32)
    I = (rng.standard_normal((nI, d)) * 0.1).astype(np.float32)
    users = rng.permutation(nU)[:nb].astype(np.int32)
    alpha = rng.uniform(-1.5, 2.0, nb).astype(np.float32)       # negative alpha too
    beta = (rng.standard_normal(nI) * 0.05).astype(np.float32)
    beta[:40] = 5.0                                              # beta that dominates the dot, and ties among those items
    beta[40:60] = -5.0
    hist = [np.unique(rng.integers(0, nI, rng.integers(0, 30))) for _ in range(nU if mode == "user_id" else nb)]
    hist[0] = np.arange(0, 30)                                   # masks some of the dominating items
    indptr = np.zeros(len(hist) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(h) for h in hist])
    indices = np.concatenate(hist).astype(np.int32)
    rows = [hist[u] for u in users] if mode == "user_id" else hist
    want, sc = oracle_bias_topk(U, I, users, alpha, beta, K, rows)
    h = ops.HistoryCSR(*to(dev, indptr, indices), by_user=(mode == "user_id"))
    stats = {}
    idx, val = ops.recommend_topk_bias(*to(dev, U, I, users, alpha, beta), K, h, stats=stats)
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    np.testing.assert_array_equal(val.cpu().numpy(), np.take_along_axis(sc, want.astype(np.int64), 1))
    ident = ops.bias_kernel_identity(stats["kernel_id"].cpu().numpy()[0])
    assert ident == {"generation": KERNELS[kernel], "bias_head": True, "d": d}


def test_the_library_picks_the_prefiltered_kernel(dev, monkeypatch):
    from pda_amd import ops
    monkeypatch.delenv("PDA_TEMP_POP_KERNEL", raising=False)
    rng = np.random.default_rng(9)
    U, I = (rng.standard_normal((300, 64)) * 0.1).astype(np.float32), (rng.standard_normal((5000, 64)) * 0.1).astype(np.float32)
    users, alpha, beta = np.arange(300, dtype=np.int32), np.ones(300, np.float32), np.zeros(5000, np.float32)
    stats = {}
    ops.recommend_topk_bias(*to(dev, U, I, users, alpha, beta), 50, None, stats=stats)
    assert ops.bias_kernel_identity(stats["kernel_id"].cpu().numpy()[0])["generation"] == 3


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_bias_kernel_worst_case_rounding_row(dev, monkeypatch, kernel):
    """A row whose dot and alpha beta are of the same size and opposite sign: fl(s + fl(alpha beta)) has to be formed exactly as stated."""
    from pda_amd import ops
    monkeypatch.setenv("PDA_TEMP_POP_KERNEL", kernel)
    d, nI = 64, 4096
    U = np.zeros((4, d), np.float32)
    U[:, 0] = np.float32(1 + 2 ** -23)
    I = np.zeros((nI, d), np.float32)
    I[:, 0] = np.float32(1) + np.arange(nI, dtype=np.float32) * np.float32(2 ** -20)
    users = np.arange(4, dtype=np.int32)
    alpha = np.float32([1.0, -1.0, 1 + 2 ** -22, 3.0])
    beta = -I[:, 0] * np.float32(1 - 2 ** -24)
    want, _ = oracle_bias_topk(U, I, users, alpha, beta, 50, [np.zeros(0, np.int64)] * 4)
    stats = {}
    idx, _ = ops.recommend_topk_bias(*to(dev, U, I, users, alpha, beta), 50, None, stats=stats)
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    assert ops.bias_kernel_identity(stats["kernel_id"].cpu().numpy()[0])["generation"] == KERNELS[kernel]


def _cli(toy, save, block, epochs=2):
    argv = [sys.executable, "-m", "pda_amd.train_new_api", "--data_path", toy, "--dataset", "toy", "--train", "temp_pop", "--test", "temp_pop",
            "--epoch", str(epochs), "--log_interval", "1", "--batch_size", "256", "--lr", "1e-2", "--regs", "1e-2", "--valid_set", "valid",
            "--save_dir", save, "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t", "--cuda", "0", "--eval_block", str(block)]
    r = subprocess.run(argv, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_cli_end_to_end(dev, tmp_path):
    from pda_amd import synthetic
    from pda_amd import train_new_api as t
    from pda_amd.model_api import BPRMFTempPop
    toy = str(tmp_path / "data") + "/"
    synthetic.write_dataset(toy + "toy", n_users=2600, n_items=300, mean_hist=10)     # more than one reference block of evaluation users
    out = _cli(toy, str(tmp_path / "s3000") + "/", 3000)
    for line in ("running temproal pop MF", "save_ID", "dataset api with pop or temp", "Epoch 1 [", "test: time:",
                 "---- result with last pop bias for temp_pop model:", "training and testing end!!!!"):
        assert line in out, line
    ck = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path / "s3000") for f in fs if f == "best_ckpt.ckpt"]
    assert len(ck) == 1
    sd = torch.load(ck[0], map_location=dev)
    assert sd["model"] == "temp_pop" and sd["item_temp_init_bias"].shape[1] == sd["temp_num"] + 1

    # the final test line, restated from the saved tables: fp32 chain + fl(alpha beta), alpha of each 2 048-user block's first user
    t.configure(["--data_path", toy, "--dataset", "toy", "--train", "temp_pop", "--Ks", "[20,50]"])
    d = t.data
    users = np.asarray(list(d.test_user_list.keys()), dtype=np.int32)
    U, I = sd["user_embedding"].cpu().numpy(), sd["item_embedding"].cpu().numpy()
    bu, Cm = sd["user_temp_bias"].cpu().numpy(), sd["item_temp_init_bias"].cpu().numpy()
    first = users[(np.arange(len(users)) // 2048) * 2048]
    alpha = (bu[first, 0] + np.float32(1)).astype(np.float32)
    top, _ = oracle_bias_topk(U, I, users, alpha, item_beta(Cm), 50, [np.asarray(d.train_user_list[u], np.int64) for u in users])
    rec20 = np.mean([len(set(top[r, :20]) & set(d.test_user_list[u])) / len(d.test_user_list[u]) for r, u in enumerate(users)])
    final = out[out.index("---- result with last pop bias for temp_pop model:"):]
    assert float(re.search(r"recall=\[([0-9.]+)", final).group(1)) == pytest.approx(rec20, abs=6e-6)

    # quirk 2 on ONE set of tables: the saved checkpoint evaluated in blocks of 2 048, 3 000 and 262 144 users gives the same metrics
    from pda_amd.sampler import DeviceSampler
    model = t.DatasetApi_Model(t.args, {"n_users": d.n_users, "n_items": d.n_items, "temp_num": sd["temp_num"]}, 256,
                               DeviceSampler(d, dev, False, temp_slots=sd["temp_num"]), dev)
    model.Recommender.load_state_dict(sd)
    rets = []
    for blk in (2048, 3000, 262144):
        ev = t.evaluation(d, [20, 50], dev, block=blk)
        ev.set_evaluate_obj_pre("test")
        ev.set_testing_popularity(None)
        rets.append(ev.eval(model, None, rec_type="main_branch"))
    for r in rets[1:]:
        for key in ("recall", "precision", "ndcg", "hit_ratio"):
            # (the per-user metrics are summed block by block: only the float64 summation order may differ)
            np.testing.assert_allclose(r[key], rets[0][key], rtol=1e-12, atol=0)
    assert rets[0]["recall"][0] == pytest.approx(rec20, abs=1e-12)

    # the device sampler hands out the slot of the drawn positive (as a float), and slots in [0, T) for users without clicks
    samp = DeviceSampler(d, dev, False, temp_slots=sd["temp_num"], ahead=1)
    for _ in range(3):
        u, p, n, tp, _tn = (x.cpu().numpy() for x in samp.batch())
        for uu, pp, tt in zip(u, p, tp):
            items, times = d.train_user_list[uu], d.train_user_list_time[uu]
            if items:
                assert tt in {times[k] for k, it in enumerate(items) if it == pp}, (uu, pp, tt)
            else:
                assert 0 <= tt < sd["temp_num"] and tt == int(tt)

    # round trip: the checkpoint loads into a fresh model and gives back the same tables; other model kinds refuse it
    args = t.args
    m = BPRMFTempPop(args, {"n_users": d.n_users, "n_items": d.n_items, "temp_num": sd["temp_num"]}, device=dev)
    m.load_state_dict(sd)
    sd2 = m.state_dict()
    for k in ("user_embedding", "item_embedding", "user_temp_bias", "item_temp_init_bias", "mC", "vbu"):
        assert torch.equal(sd2[k], sd[k]), k
    from pda_amd.model_api import BPRMF
    with pytest.raises(ValueError):
        BPRMF(args, {"n_users": d.n_users, "n_items": d.n_items}, device=dev).load_state_dict(sd)
