"""CPU suite for BPRMF(t)-pop (`--train temp_pop`): a float64 restatement of the reference's step cross-checked against torch.autograd on a
direct transcription of the TF graph, the host temp sampler, the alpha rule of the evaluation blocks, and the C entry points' argument checks."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from temp_pop_ref import adam_steps, forward_grads, scores_bias

B1, B2, EPS = 0.9, 0.999, 1e-8


def batch(rng, nU, nI, T, B, stage0=True):
    users = rng.integers(0, nU, B)
    pos = rng.integers(0, nI, B)
    neg = rng.integers(0, nI, B)
    temps = rng.integers(0 if stage0 else 1, T, B)
    return users, pos, neg, temps


def tf_graph_loss(U, I, bu, Cm, users, pos, neg, temps, regs, batch_size):
    """MF/model_api.py:336-374 op for op; gather_nd out of range gives 0 (and no gradient), as TF 1.14's GPU kernel does."""
    T = Cm.shape[1] - 1
    B = len(users)
    raw = torch.arange(B)
    t = torch.as_tensor(temps)
    ue, pe, ne = U[users], I[pos], I[neg]
    ub_all, pb_all, nb_all = bu[users], Cm[pos], Cm[neg]                       # [B, 1], [B, T + 1], [B, T + 1]

    def gather_nd(x, rows, cols):
        ok = cols < x.shape[1]
        return torch.where(ok, x[rows, cols.clamp(max=x.shape[1] - 1)], torch.zeros((), dtype=x.dtype))

    user_temp_bias = gather_nd(ub_all, raw, t)
    pos_bias = (user_temp_bias + 1.0) * (pb_all[:, T] + gather_nd(pb_all, raw, t))
    neg_bias = (user_temp_bias + 1.0) * (nb_all[:, T] + gather_nd(nb_all, raw, t))
    sp = pos_bias + (ue * pe).sum(1)
    sn = neg_bias + (ue * ne).sum(1)
    mf = -torch.log(torch.sigmoid(sp - sn) + 1e-10).mean()
    reg = regs * ((ue ** 2).sum() / 2 + (pe ** 2).sum() / 2 + (ne ** 2).sum() / 2) / batch_size
    return mf + reg, mf, reg


@pytest.mark.parametrize("T, stage0", [(1, True), (3, True), (3, False), (10, True), (10, False)])
def test_restatement_matches_autograd_of_the_tf_graph(T, stage0):
    rng = np.random.default_rng(T * 7 + stage0)
    nU, nI, d, B, regs = 40, 30, 8, 64, 1e-2
    U, I = rng.standard_normal((nU, d)) * 0.3, rng.standard_normal((nI, d)) * 0.3
    bu, Cm = rng.standard_normal((nU, 1)) * 0.3, rng.standard_normal((nI, T + 1)) * 0.3
    users, pos, neg, temps = batch(rng, nU, nI, T, B, stage0)
    users[:5] = users[0]          # repeated users and items
    pos[:9] = pos[0]
    loss, grads = forward_grads(U, I, bu, Cm, users, pos, neg, temps, regs, B)
    tt = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (U, I, bu, Cm)]
    tl = tf_graph_loss(*tt, torch.as_tensor(users), torch.as_tensor(pos), torch.as_tensor(neg), temps, regs, B)
    tl[0].backward()
    np.testing.assert_allclose(loss, [float(x.detach()) for x in tl], rtol=1e-12, atol=1e-14)
    for g, t in zip(grads, tt):
        np.testing.assert_allclose(g, t.grad.numpy(), rtol=1e-10, atol=1e-14)
    if not stage0:
        assert not grads[2].any(), "quirk 1: without stage-0 triplets the user bias gets no gradient"


def test_three_adam_steps_match_torch_adam_on_the_tf_graph():
    """TF-1.14 dense-decay Adam on all four tables (the epsilon-hat form: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), x -= lr_t m / (sqrt(v) + eps))."""
    rng = np.random.default_rng(5)
    nU, nI, d, B, T, regs, lr = 30, 20, 8, 32, 3, 1e-2, 1e-2
    tabs = [rng.standard_normal((nU, d)) * 0.3, rng.standard_normal((nI, d)) * 0.3, rng.standard_normal((nU, 1)) * 0.3,
            rng.standard_normal((nI, T + 1)) * 0.3]
    batches = [batch(rng, nU, nI, T, B) for _ in range(3)]
    got, losses = adam_steps([x.copy() for x in tabs], batches, regs, B, lr)
    tt = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in tabs]
    m = [torch.zeros_like(x) for x in tt]
    v = [torch.zeros_like(x) for x in tt]
    for step, (u, p, n, t) in enumerate(batches, 1):
        for x in tt:
            x.grad = None
        tf_graph_loss(*tt, torch.as_tensor(u), torch.as_tensor(p), torch.as_tensor(n), t, regs, B)[0].backward()
        lr_t = lr * np.sqrt(1 - B2 ** step) / (1 - B1 ** step)
        with torch.no_grad():
            for x, mm, vv in zip(tt, m, v):
                mm.mul_(B1).add_((1 - B1) * x.grad)
                vv.mul_(B2).add_((1 - B2) * x.grad * x.grad)
                x.sub_(lr_t * mm / (vv.sqrt() + EPS))
    for a, b in zip(got, tt):
        np.testing.assert_allclose(a, b.detach().numpy(), rtol=1e-12, atol=1e-14)


def test_bias_head_scores_are_the_fp32_chain_plus_one_rounded_product():
    rng = np.random.default_rng(1)
    s = rng.standard_normal((3, 5)).astype(np.float32)
    alpha = np.float32([1.5, -0.25, 3.0])
    beta = rng.standard_normal(5).astype(np.float32)
    h = scores_bias(s, alpha, beta)
    assert h.dtype == np.float32
    np.testing.assert_array_equal(h, s + (alpha[:, None] * beta[None, :]).astype(np.float32))


class _Data:
    def __init__(self):
        self.batch_size, self.n_users = 6, 8
        self.train_user_list = {u: ([] if u == 3 else sorted(random.Random(u).sample(range(20), 4))) for u in range(8)}
        self.train_user_list_time = {u: [(u + k) % 3 for k in range(len(self.train_user_list[u]))] for u in range(8)}
        self.n_train = sum(len(v) for v in self.train_user_list.values())
        self.items = list(range(20))
        self.unique_times = [0, 1, 2]


def test_host_temp_sampler_draws_the_positive_slot():
    from pda_amd.sampler import host_generator_with_temp, n_batches
    random.seed(3)
    np.random.seed(3)
    d = _Data()
    seen_empty = False
    out = list(host_generator_with_temp(d))
    assert len(out) == n_batches(d)
    for users, pos, neg, temp, raw in out:
        np.testing.assert_array_equal(raw, np.arange(d.batch_size))
        assert len(set(users)) == len(users) == d.batch_size
        for u, p, n, t in zip(users, pos, neg, temp):
            items, times = d.train_user_list[u], d.train_user_list_time[u]
            assert n not in items
            if not items:
                seen_empty = True
                assert p == 0 and t in d.unique_times
            else:
                assert t == times[items.index(p)]
    assert seen_empty


@pytest.mark.parametrize("block", [2048, 3000, 262144])
def test_alpha_comes_from_the_first_user_of_each_reference_block(block):
    from pda_amd.train_new_api import reference_block_first
    n_eval = 300000
    got = np.concatenate([reference_block_first(i, min(block, n_eval - i)).numpy() for i in range(0, n_eval, block)])
    want = np.repeat(np.arange(0, n_eval, 2048), 2048)[:n_eval]      # the reference: blocks of 2 048 in evaluation-list order
    np.testing.assert_array_equal(got, want)


def test_temp_slots_at_or_beyond_T_are_refused():
    from pda_amd.train_new_api import check_temp_slots
    d = _Data()
    check_temp_slots(d, 3)
    with pytest.raises(ValueError):
        check_temp_slots(d, 2)


def test_checkpoints_of_other_model_kinds_are_refused():
    from pda_amd.model_api import BPRMFTempPop, _MFBase
    with pytest.raises(ValueError):
        _MFBase.load_state_dict(object.__new__(_MFBase), {"user_embedding": None, "model": "temp_pop"})
    with pytest.raises(ValueError):
        BPRMFTempPop.load_state_dict(object.__new__(BPRMFTempPop), {"user_embedding": None})


def test_temp_pop_entry_points_reject_null_pointers_without_gpu():
    from pda_amd import _lib
    lib = _lib.load()
    null = C.c_void_p(None)
    assert set(_lib.TEMP_POP_SIGNATURES) == {"pda_temp_pop_step_f32", "pda_temp_pop_sweep_f32", "pda_temp_pop_adam_step_f32",
                                             "pda_temp_pop_score_workspace_bytes", "pda_temp_pop_score_topk_f32"}
    assert not set(_lib.TEMP_POP_SIGNATURES) & set(_lib.SIGNATURES)
    assert lib.pda_temp_pop_step_f32(*([null] * 8), 16, 64, 10, 1e-2, 16.0, *([null] * 6), 1, null, null) == -1
    assert lib.pda_temp_pop_sweep_f32(*([null] * 5), 10, *([null] * 5), 10, *([null] * 8), 64, 10, 1, 1e-3, 0.9, 0.999, 1e-8, null) == -1
    assert lib.pda_temp_pop_adam_step_f32(*([null] * 5), 10, *([null] * 5), 10, *([null] * 12), 16, 64, 10, 1e-2, 16.0, 1, 1e-3, 0.9, 0.999,
                                          1e-8, null, null) == -1
    assert lib.pda_temp_pop_score_topk_f32(*([null] * 6), 16, 0, 100, 64, null, null, 0, 50, 1, null, null, null) == -1
    assert lib.pda_temp_pop_score_workspace_bytes(2048) >= 64 + 4 * 2048
