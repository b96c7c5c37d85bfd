"""GPU: DICE (`--train dice`, include/pda_hip_dice.h) -- the gradient step and the L_dis pass against the float64 restatement of
tests/dice_ref.py, the whole Adam step, PNSM against its numpy restatement bit for bit, the evaluation paths at row width 2d, and the CLI.

Tolerances: 1e-5 absolute on every loss term and every gradient element against float64, for every shape -- B = 2 048 on 50 x 40 tables
included (a gradient element there is a sum of ~100 atomics of ~1e-5 each: its fp32 rounding is ~1e-9, so the float32 comparison the issue
allows for that case is not needed and not used).  1e-5 on tables and moments after three Adam steps."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dice_ref import PARITY_CASES, PARITY_SEED, PARITY_STEP, dice_adam, dice_grads, parity_data, pnsm
from sampler_ref import REJECT_CAP

pytestmark = pytest.mark.gpu
TOL = 1e-5
NU, NI = 50, 40
KW = dict(w_int=0.3, w_con=0.2, regs=1e-2)


def tables(rng, d, nU=NU, nI=NI):
    return (rng.standard_normal((nU, 2 * d)) * 0.3).astype(np.float32), (rng.standard_normal((nI, 2 * d)) * 0.3).astype(np.float32)


def batch(rng, B, kind, nU=NU, nI=NI):
    users, pos, neg = (rng.integers(0, n, B).astype(np.int32) for n in (nU, nI, nI))
    mask = {"zeros": np.zeros(B), "ones": np.ones(B), "mixed": rng.integers(0, 2, B)}[kind].astype(np.uint8)
    return users, pos, neg, mask


def to(dev, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


def run_grads(dev, U, I, b, B_div, dis_kind, pen, step=1):
    from pda_amd import ops
    Ut, It, ut, pt, nt, mt = to(dev, U, I, *b)
    st = ops.DiceState(Ut, It)
    loss = torch.zeros(6, device=dev)
    ops.dice_grads(Ut, It, ut, pt, nt, mt, st, dis_pen=pen, dis_loss=dis_kind, reg_div=B_div, step=step, loss_acc=loss, **KW)
    return loss.cpu().numpy(), st.gU.cpu().numpy(), st.gI.cpu().numpy(), st


def check_against_ref(dev, U, I, b, dis_kind, pen):
    B = len(b[0])
    loss, gU, gI, st = run_grads(dev, U, I, b, B, dis_kind, pen)
    terms, rU, rI = dice_grads(U, I, *b, dis_pen=pen, dis_kind=dis_kind, reg_div=B, **KW)
    print("dice grads: max |loss err| %.3g  max |gU err| %.3g  max |gI err| %.3g" % (np.abs(loss - terms).max(), np.abs(gU - rU).max(),
                                                                                   np.abs(gI - rI).max()))
    np.testing.assert_allclose(loss, terms, atol=TOL, rtol=0)
    np.testing.assert_allclose(gU, rU, atol=TOL, rtol=0)
    np.testing.assert_allclose(gI, rI, atol=TOL, rtol=0)
    assert abs(loss[0] - (loss[1] + loss[2])) <= TOL
    # the tags and the row lists: exactly the batch's distinct rows
    users, pos, neg, _ = b
    S_u, S_i = np.unique(users), np.unique(np.concatenate([pos, neg]))
    ws = st.rows_ws.cpu().numpy()
    assert (ws[0], ws[1]) == (len(S_u), len(S_i))
    assert sorted(ws[4:4 + ws[0]]) == list(S_u) and sorted(ws[4 + B:4 + B + ws[1]]) == list(S_i)
    tagU, tagI = st.tagU.cpu().numpy(), st.tagI.cpu().numpy()
    assert (np.nonzero(tagU)[0] == S_u).all() and (np.nonzero(tagI)[0] == S_i).all() and set(tagU[S_u]) == {1} and set(tagI[S_i]) == {1}


@pytest.mark.parametrize("B", [1, 7, 2048])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_gradients_and_loss_against_the_float64_restatement(dev, d, B):
    rng = np.random.default_rng(100 * d + B)
    U, I = tables(rng, d)
    for kind in ("zeros", "ones", "mixed"):
        b = batch(rng, B, kind)
        for dis_kind, pen in (("l1", 0.05), ("l2", 0.05), ("l1", 0.0)):
            check_against_ref(dev, U, I, b, dis_kind, pen)


@pytest.mark.parametrize("d", [32, 128])
def test_a_batch_of_one_repeated_triplet(dev, d):
    """Every triplet the same (u, p, n): duplicate rows everywhere, |S_u| = 1, |S_i| = 2."""
    rng = np.random.default_rng(d)
    U, I = tables(rng, d)
    B = 70
    b = (np.full(B, 3, np.int32), np.full(B, 5, np.int32), np.full(B, 9, np.int32), rng.integers(0, 2, B).astype(np.uint8))
    for dis_kind in ("l1", "l2"):
        check_against_ref(dev, U, I, b, dis_kind, 0.05)


def test_l1_has_the_zero_subgradient_where_interest_equals_conformity(dev):
    d, B = 32, 33
    rng = np.random.default_rng(8)
    U, I = tables(rng, d)
    b = batch(rng, B, "mixed")
    u, p = int(b[0][0]), int(b[1][0])
    U[u, d:d + 5] = U[u, :5]
    I[p, d + 7:d + 20] = I[p, 7:20]
    loss, gU, gI, _ = run_grads(dev, U, I, b, B, "l1", 0.5)
    base, hU, hI, _ = run_grads(dev, U, I, b, B, "l1", 0.0)
    dU, dI = gU - hU, gI - hI                                       # the discrepancy's share of the gradient
    assert np.abs(dU[u, :5]).max() <= 1e-7 and np.abs(dU[u, d:d + 5]).max() <= 1e-7 and np.abs(dU[u, 5:d]).min() > 1e-5
    assert np.abs(dI[p, 7:20]).max() <= 1e-7 and np.abs(dI[p, d + 7:d + 20]).max() <= 1e-7
    check_against_ref(dev, U, I, b, "l1", 0.5)


def test_ops_checks_ids_mask_and_width(dev):
    from pda_amd import ops
    rng = np.random.default_rng(1)
    U, I = tables(rng, 32)
    Ut, It, ut, pt, nt, mt = to(dev, U, I, *batch(rng, 9, "mixed"))
    st = ops.DiceState(Ut, It)
    kw = dict(dis_pen=0.1, reg_div=9, step=1, **KW)
    bad = pt.clone()
    bad[4] = NI
    with pytest.raises(ValueError, match="outside the tables"):
        ops.dice_grads(Ut, It, ut, bad, nt, mt, st, **kw)
    with pytest.raises(TypeError, match="mask"):
        ops.dice_grads(Ut, It, ut, pt, nt, mt.int(), st, **kw)
    with pytest.raises(ValueError, match="embedding width"):
        ops.dice_grads(Ut[:, :48].contiguous(), It[:, :48].contiguous(), ut, pt, nt, mt, st, **kw)
    with pytest.raises(ValueError, match="l1"):
        ops.dice_grads(Ut, It, ut, pt, nt, mt, st, dis_loss="dcor", **kw)
    # the kernel skips a triplet with an id outside the tables (memory safety when the host check is off): the other eight still count, with
    # the mean over B = 9 -- 8/9 of their click / interest / conformity gradient, their L2 term, and L_dis over their distinct rows
    ops.dice_grads(Ut, It, ut, bad, nt, mt, st, check_ids=False, **kw)
    keep = np.arange(9) != 4
    b8 = [x.cpu().numpy()[keep] for x in (ut, pt, nt, mt)]
    ref = lambda pen, regs: dice_grads(U, I, *b8, w_int=0.3, w_con=0.2, dis_pen=pen, dis_kind="l1", regs=regs, reg_div=9)[1:]   # noqa: E731
    a, r, c = ref(0.0, 0.0), ref(0.0, 1e-2), ref(0.1, 0.0)
    for got, k in ((st.gU, 0), (st.gI, 1)):
        np.testing.assert_allclose(got.cpu().numpy(), 8 / 9 * a[k] + (r[k] - a[k]) + (c[k] - a[k]), atol=TOL, rtol=0)


def test_untouched_rows_take_the_dense_decay_of_the_bpr_step(dev):
    """After one pda_dice_adam_step_f32 the rows outside the batch equal, bit for bit, the idle rows of pda_adam_step_f32 on the same tables
    (the dense decay with g = 0), and both gradient tables are zero again."""
    from pda_amd import ops
    d, B, lr_t = 32, 16, 3e-3
    rng = np.random.default_rng(21)
    U, I = tables(rng, d, 300, 200)
    mom = [np.abs(rng.standard_normal(x.shape)).astype(np.float32) * 1e-3 for x in (U, U, I, I)]
    b = batch(rng, B, "mixed", 300, 200)
    Ut, It, ut, pt, nt, mt = to(dev, U, I, *b)
    st = ops.DiceState(Ut, It)
    for t, m in zip((st.mU, st.vU, st.mI, st.vI), mom):
        t.copy_(torch.from_numpy(m))
    ops.dice_adam_step(Ut, It, ut, pt, nt, mt, st, dis_pen=0.05, reg_div=B, step=1, lr_t=lr_t, **KW)
    U2, I2, mU, vU, mI, vI = to(dev, U, I, *mom)
    gU, gI = torch.zeros_like(U2), torch.zeros_like(I2)
    tagU, tagI = ops.adam_row_tags(300, 200, dev)
    ops.adam_step(U2, mU, vU, gU, tagU, I2, mI, vI, gI, tagI, ut, pt, nt, regs=1e-2, reg_div=B, step=1, lr_t=lr_t)
    idleU = np.setdiff1d(np.arange(300), b[0])
    idleI = np.setdiff1d(np.arange(200), np.concatenate([b[1], b[2]]))
    assert len(idleU) >= 280 and len(idleI) >= 160
    for got, ref, rows in ((Ut, U2, idleU), (st.mU, mU, idleU), (st.vU, vU, idleU), (It, I2, idleI), (st.mI, mI, idleI), (st.vI, vI, idleI)):
        r = torch.from_numpy(rows).to(dev)
        assert torch.equal(got[r], ref[r])
    assert not torch.equal(Ut[int(b[0][0])], U2[int(b[0][0])])        # (the batch's rows do differ: another model)
    assert float(st.gU.abs().max()) == 0.0 and float(st.gI.abs().max()) == 0.0


@pytest.mark.parametrize("dis_kind", ["l1", "l2"])
def test_three_whole_steps_against_the_restatement(dev, dis_kind):
    from pda_amd import ops
    d, B, lr = 32, 64, 1e-2
    rng = np.random.default_rng(33)
    U, I = tables(rng, d)
    Ut, It = to(dev, U, I)
    st = ops.DiceState(Ut, It)
    Ur, Ir, state = U.astype(np.float64), I.astype(np.float64), None
    for t in (1, 2, 3):
        b = batch(rng, B, "mixed")
        Ur, Ir, state, terms = dice_adam(Ur, Ir, state, t, lr, *b, dis_pen=0.05, dis_kind=dis_kind, reg_div=B, **KW)
        loss = torch.zeros(6, device=dev)
        ops.dice_adam_step(Ut, It, *to(dev, *b), st, dis_pen=0.05, dis_loss=dis_kind, reg_div=B, step=t, lr_t=ops.adam_lr_t(lr, t), loss_acc=loss,
                           check_ids=True, **KW)
        np.testing.assert_allclose(loss.cpu().numpy(), terms, atol=TOL, rtol=0)
        assert float(st.gU.abs().max()) == 0.0 and float(st.gI.abs().max()) == 0.0
    got = dict(U=Ut, I=It, mU=st.mU, vU=st.vU, mI=st.mI, vI=st.vI)
    ref = dict(U=Ur, I=Ir, **state)
    for k in got:
        err = np.abs(got[k].cpu().numpy() - ref[k]).max()
        print("dice three steps (%s): max |%s err| %.3g" % (dis_kind, k, err))
    for k in got:
        np.testing.assert_allclose(got[k].cpu().numpy(), ref[k], atol=TOL, rtol=0, err_msg=k)


def test_the_step_replays_from_a_captured_graph(dev):
    """pda_dice_adam_step_f32 reads nothing back on the host: two steps (tags 1 and 2) captured once and replayed give the tables of the same
    two steps launched directly."""
    from pda_amd import ops
    d, B = 64, 200
    rng = np.random.default_rng(5)
    U, I = tables(rng, d)
    bt = to(dev, *batch(rng, B, "mixed"))

    def two_steps(Ut, It, st, loss):
        for t in (1, 2):
            ops.dice_adam_step(Ut, It, *bt, st, dis_pen=0.05, reg_div=B, step=t, lr_t=ops.adam_lr_t(1e-2, t), loss_acc=loss, **KW)
    Ua, Ia = to(dev, U, I)
    sa, la = ops.DiceState(Ua, Ia), torch.zeros(6, device=dev)
    sa.ws(B)
    two_steps(Ua, Ia, sa, la)
    Ub, Ib = to(dev, U, I)
    sb, lb = ops.DiceState(Ub, Ib), torch.zeros(6, device=dev)
    sb.ws(B)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            two_steps(Ub, Ib, sb, lb)
    torch.cuda.synchronize()
    assert torch.equal(Ub.cpu(), torch.from_numpy(U))                 # capturing runs nothing
    g.replay()
    torch.cuda.synchronize()
    torch.testing.assert_close(Ub, Ua, atol=2e-6, rtol=0)
    torch.testing.assert_close(Ib, Ia, atol=2e-6, rtol=0)
    torch.testing.assert_close(lb, la, atol=1e-5, rtol=0)


# ---- PNSM ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def parity_inputs():
    return parity_data()


@functools.lru_cache(maxsize=None)
def parity_ref(B, M):
    indptr, indices, pop = parity_inputs()
    return pnsm(PARITY_SEED, PARITY_STEP, B, indptr, indices, pop, M, n_pool=len(indptr) - 1)


@pytest.mark.parametrize("B, M", PARITY_CASES)
def test_sampler_equals_the_restatement_bit_for_bit(dev, B, M):
    from pda_amd import ops
    indptr, indices, pop = parity_inputs()
    n_users = len(indptr) - 1
    ip, ix = to(dev, indptr, indices)
    dp = ops.DicePop(ix, len(pop))
    assert (dp.pop.cpu().numpy() == pop).all() and (dp.sorted_pop.cpu().numpy() == np.sort(pop)).all()
    ref = parity_ref(B, M)
    got = ops.dice_sample(ip, ix, dp, B, margin=M, seed=PARITY_SEED, step=PARITY_STEP, n_pool=n_users)
    for name, t in zip(("users", "pos", "neg", "mask"), got):
        np.testing.assert_array_equal(t.cpu().numpy(), ref[name], err_msg=name)
    # the _dev form: step and margin from device memory, step + 1 into the other slot
    out = tuple(torch.full((B,), -1, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.int32, torch.uint8))
    ctr = torch.tensor([PARITY_STEP, 0], dtype=torch.int64, device=dev)
    ops.dice_sample_into(out, ip, ix, dp, margin_dev=torch.tensor([M], dtype=torch.float32, device=dev), seed=PARITY_SEED, step_dev=ctr,
                         parity=0, n_pool=n_users)
    for name, t in zip(("users", "pos", "neg", "mask"), out):
        np.testing.assert_array_equal(t.cpu().numpy(), ref[name], err_msg=name + " (_dev)")
    assert ctr.tolist() == [PARITY_STEP, PARITY_STEP + 1]
    # users and positives are those of the plain sampler for the same (seed, step)
    u, p, _, _, _ = ops.sample_triplets(ip, ix, B, seed=PARITY_SEED, step=PARITY_STEP, n_pool=n_users, neg_range=(0, len(pop)))
    assert torch.equal(u, got[0]) and torch.equal(p, got[1])
    # the invariants, on every row that did not reach the cap (at least 99 % of them: tests/test_dice_host.py)
    users, pos, neg, mask = (t.cpu().numpy() for t in got)
    ok = ref["rejections"] < REJECT_CAP
    assert ok.mean() >= 0.99
    popf, Mf = pop.astype(np.float32), np.float32(M)
    for r in np.nonzero(ok)[0]:
        assert neg[r] not in indices[indptr[users[r]]:indptr[users[r] + 1]]
        if ref["whole"][r]:
            assert mask[r] == (pop[neg[r]] > pop[pos[r]])
        elif mask[r]:
            assert popf[neg[r]] > popf[pos[r]] + Mf
        else:
            assert popf[neg[r]] < popf[pos[r]] - Mf
    if B == 2048:
        assert (M == 1e9) == bool(ref["whole"].all()) and (M == 1e9 or (not ok.all() and 0.3 < mask.mean() < 0.7))


def test_sampler_with_given_users_and_the_margin_schedule(dev):
    from pda_amd import ops
    indptr, indices, pop = parity_inputs()
    ip, ix = to(dev, indptr, indices)
    dp = ops.DicePop(ix, len(pop))
    users = np.arange(1, 65, dtype=np.int32)
    ref = pnsm(7, 2, 64, indptr, indices, pop, 3.0, users=users)
    got = ops.dice_sample(ip, ix, dp, 64, margin=3.0, seed=7, step=2, users=torch.from_numpy(users).to(dev))
    for name, t in zip(("users", "pos", "neg", "mask"), got):
        np.testing.assert_array_equal(t.cpu().numpy(), ref[name], err_msg=name)


def test_sampler_dev_walks_the_two_slot_counter_and_reads_a_one_slot_one(dev):
    """pda_dice_sample_dev over consecutive steps: parity 0 then parity 1 on a two-slot counter (each call reads its slot and stores step + 1 into
    the other), then a one-slot counter that is only read.  B = 37 of 50 users (distinct, drawn by the kernel), 40 items, user 3 without train
    items, user 5 with all items but one.  Every output of every batch equals tests/dice_ref.pnsm at that step."""
    from pda_amd import ops
    n_users, n_items, B, M, seed, step = 50, 40, 37, 2.0, 0xD1B54A32D192ED03, 28
    rng = np.random.default_rng(8)
    rows = [np.sort(rng.permutation(n_items)[:rng.integers(1, 13)]) for _ in range(n_users)]
    rows[3] = np.zeros(0, np.int64)
    rows[5] = np.delete(np.arange(n_items), 17)
    indptr = np.zeros(n_users + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.concatenate(rows).astype(np.int32)
    pop = np.bincount(indices, minlength=n_items).astype(np.int32)
    ip, ix = to(dev, indptr, indices)
    dp = ops.DicePop(ix, n_items)
    margin_dev = torch.tensor([M], dtype=torch.float32, device=dev)
    out = tuple(torch.full((B,), -1, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.int32, torch.uint8))

    def check(at, what):
        ref = pnsm(seed, at, B, indptr, indices, pop, M, n_pool=n_users)
        assert len(np.unique(ref["users"])) == B
        for name, t in zip(("users", "pos", "neg", "mask"), out):
            np.testing.assert_array_equal(t.cpu().numpy(), ref[name], err_msg="%s, %s" % (name, what))
        return ref

    ctr = torch.tensor([step, -1], dtype=torch.int64, device=dev)
    ops.dice_sample_into(out, ip, ix, dp, margin_dev=margin_dev, seed=seed, step_dev=ctr, parity=0, n_pool=n_users)
    first = check(step, "parity 0")
    assert ctr.tolist() == [step, step + 1]
    ops.dice_sample_into(out, ip, ix, dp, margin_dev=margin_dev, seed=seed, step_dev=ctr, parity=1, n_pool=n_users)
    second = check(step + 1, "parity 1")
    assert ctr.tolist() == [step + 2, step + 1]
    assert not np.array_equal(first["users"], second["users"])          # (two steps, two batches)
    one = torch.tensor([step + 2], dtype=torch.int64, device=dev)
    ops.dice_sample_into(out, ip, ix, dp, margin_dev=margin_dev, seed=seed, step_dev=one, n_pool=n_users)
    third = check(step + 2, "one slot, read only")
    assert one.tolist() == [step + 2] and ctr.tolist() == [step + 2, step + 1]
    # the two rows the data was built for are in all three batches (the step was chosen for it): user 3 has positive 0; user 5's negative is the
    # one item it does not own where its side of the catalogue holds it (the first batch), else the draw of the last try
    for ref in (first, second, third):
        assert ref["pos"][ref["users"] == 3].tolist() == [0]
        r = np.nonzero(ref["users"] == 5)[0]
        assert r.size == 1 and (ref["neg"][r[0]] == 17) == (ref["rejections"][r[0]] < REJECT_CAP)
    assert first["neg"][first["users"] == 5].tolist() == [17] and second["rejections"].max() == REJECT_CAP


# ---- evaluation: the raw head at row width 2d -----------------------------------------------------------------------------------------------
def test_evaluation_paths_serve_the_concatenated_tables(dev):
    from pda_amd import ops
    from pda_amd import train_new_api as t
    from pda_amd.parse import parse_args
    nU, nI, K = 300, 500, 50
    args = parse_args(["--train", "dice", "--embed_size", "32", "--batch_size", "64", "--verbose", "0"])
    cfg = {"n_users": nU, "n_items": nI}
    model = t.DatasetApi_Model(args, cfg, 64, (lambda: iter(())), dev)
    rng = np.random.default_rng(2)
    rows = [np.sort(rng.choice(nI, size=rng.integers(0, 30), replace=False)).astype(np.int32) for _ in range(nU)]
    hist = ops.HistoryCSR.from_lists(rows, dev, by_user=True)
    users = torch.arange(0, nU, 2, dtype=torch.int32, device=dev)
    U, I = model.Recommender.score_tables()
    assert U.shape == (nU, 64) and I.shape == (nI, 64)
    idx, val = model.recommend_device(users, None, "main_branch", None, hist, K=K)
    ridx, rval = ops.recommend_topk(U, I, users, K, ops.HEAD_RAW, None, hist)
    assert torch.equal(idx, ridx) and torch.equal(val, rval)
    dense = model.testing(None, users.cpu().numpy(), list(range(nI)), "main_branch")
    np.testing.assert_allclose(dense, (U[users.long()].double() @ I.double().T).cpu().numpy(), atol=1e-5)
    for r, u in enumerate(users.tolist()):
        s = dense[r].copy()
        s[rows[u]] = -np.inf
        order = np.lexsort((np.arange(nI), -s))[:K]
        np.testing.assert_array_equal(idx[r].cpu().numpy(), order)
        np.testing.assert_array_equal(val[r].cpu().numpy(), s[order])
    # DICE-A: main_with_pop equals a BPRMF holding the same 2d-wide tables
    plain_args = parse_args(["--train", "normal", "--embed_size", "64", "--batch_size", "64", "--verbose", "0"])
    plain = t.DatasetApi_Model(plain_args, cfg, 64, (lambda: iter(())), dev)
    plain.Recommender.weights["user_embedding"].copy_(U)
    plain.Recommender.weights["item_embedding"].copy_(I)
    pop = torch.from_numpy((rng.uniform(0.01, 1, nI) ** 0.2).astype(np.float32)).to(dev)
    a = model.recommend_device(users, None, "main_with_pop", pop, hist, K=K)
    b = plain.recommend_device(users, None, "main_with_pop", pop, hist, K=K)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], idx)


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------------
def test_cli_trains_dice_and_export_topk_restores_it(dev, tmp_path):
    """python -m pda_amd.train_new_api --train dice --test normal in a child process, three epochs on the smallest synthetic dataset: it ends,
    prints the reference's result lines, writes best_ckpt.ckpt, lowers mf_loss, and export_topk restores the checkpoint."""
    import re
    from pda_amd import synthetic
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    synthetic.write_dataset(str(tmp_path / "data" / "toy"), n_users=200, n_items=150, mean_hist=12)
    argv = ["--data_path", str(tmp_path / "data") + "/", "--dataset", "toy", "--train", "dice", "--test", "normal", "--epoch", "3", "--embed_size", "32",
            "--log_interval", "1", "--batch_size", "128", "--lr", "1e-2", "--regs", "1e-3", "--valid_set", "valid", "--pop_exp", "0.22",
            "--save_dir", str(tmp_path / "ckpt") + "/", "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t", "--cuda", "0", "--eval_block", "128",
            "--dice_margin", "2"]
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "pda_amd.train_new_api"] + argv, cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert "running DICE" in out and "best expo" in out and "recall=[" in out and "BPRMF-A with injecting" in out and "training and testing end!!!!" in out
    mf = [float(m.group(1)) for m in re.finditer(r"Epoch \d+ \[[^\]]*\]: train==\[[-\d.]+=([-\d.]+) \+ [-\d.]+\]", out)]
    assert len(mf) == 3 and mf[2] < mf[0], mf
    ck = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path / "ckpt") for f in fs]
    assert any(f.endswith("best_ckpt.ckpt") for f in ck) and any("train_dice" in f for f in ck)
    sd = torch.load([f for f in ck if f.endswith("best_ckpt.ckpt")][0], map_location="cpu")
    assert sd["model"] == "dice" and sd["embed_size"] == 32 and sd["user_embedding"].shape[1] == 64 and "mU" in sd
    assert sd["dice_margin"] <= 2.0 and sd["dice_int_weight"] <= 0.1
    from pda_amd import export_topk
    res = export_topk.main(argv + ["--export_out", str(tmp_path / "lists.npz")])
    assert res["idx"].shape[1] == 50 and res["idx"].shape[0] == len(res["users"]) > 0 and np.isfinite(res["val"]).all()
    with pytest.raises(ValueError, match="dice model cannot be loaded into BPRMF"):
        export_topk.main([a if a != "dice" else "normal" for a in argv[:argv.index("--dice_margin")]] + ["--embed_size", "64", "--save_dir",
                         _as_normal_dir(tmp_path, ck), "--export_out", str(tmp_path / "x.npz")])


def _as_normal_dir(tmp_path, ck):
    """A --train normal checkpoint directory that holds the DICE file: what a user gets who points the wrong flags at it."""
    import shutil
    src = [f for f in ck if f.endswith("best_ckpt.ckpt")][0]
    dst_root = tmp_path / "ckpt2"
    rel = os.path.relpath(os.path.dirname(src), tmp_path / "ckpt").replace("train_dice", "train_normal")
    os.makedirs(dst_root / rel, exist_ok=True)
    shutil.copy(src, dst_root / rel / "best_ckpt.ckpt")
    return str(dst_root) + "/"
