"""GPU: the bit-reproducible training path (`--deterministic 1`, include/pda_hip_det.h) -- the planned gradient against the float64
oracle, the Adam step on it against the oracle's optimiser, bit identity run after run / across cache policies / across the sweep and
the replay, the rejected batch, the ordered metric reduction, and two whole CLI runs compared line for line.

Batches: positives Zipf(1.0) over a random permutation of the items, negatives uniform, users the first B of a permutation.  Every test
asserts with np.bincount, before it launches anything, that its batch reaches the path it is about (long segments: > 8 references of a
row; the multi-workgroup path of large batches: >= kXlMin = 512 references)."""
import json
import os
import re

import numpy as np
import pytest
import torch

import train_ref
from oracle import pda_oracle as po

pytestmark = pytest.mark.gpu
TOL = 1e-5
G = os.path.join(os.path.dirname(__file__), "golden")
SHORT, XL_MIN = 8, 512                    # launch B: entries summed by one lane group; pda_plan_common.h kXlMin
BIG = (50000, 20000)                      # C2's tables
SMALL = (2500, 700)                       # the shapes of test_reference_faithful_adam_three_steps


def zipf_batch(seed, nU, nI, B):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(nI)
    w = 1.0 / np.arange(1, nI + 1)
    pos = perm[rng.choice(nI, B, p=w / w.sum())].astype(np.int32)
    neg = rng.integers(0, nI, B).astype(np.int32)
    users = rng.permutation(nU)[:B].astype(np.int32)
    return users, pos, neg


def pops(seed, B):
    rng = np.random.default_rng(1000 + seed)
    return (rng.uniform(0, 1, B) ** 0.22).astype(np.float32), (rng.uniform(0, 1, B) ** 0.22).astype(np.float32)


def check_batch(users, pos, neg, nI, B):
    """The properties the tests rely on, on the CPU."""
    c = np.bincount(np.concatenate([pos, neg]), minlength=nI)
    assert len(np.unique(users)) == B, "users are distinct in a planned batch"
    assert (c > SHORT).sum() >= 10 and c.max() >= 100, "the long-segment path of launch B"
    if B > 4096:
        assert c.max() >= XL_MIN, "the multi-workgroup segments behind pda_triplet_plan_large"
    else:
        assert c.max() < XL_MIN
    return c


def to(dev, *xs):
    return [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


def tables(seed, nU, nI, d, scale):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((nU, d)) * scale).astype(np.float32), (rng.standard_normal((nI, d)) * scale).astype(np.float32)


def adam_close(got, ref):
    """tests/test_gpu_bpr_step.py's criterion, copied as it stands there: 1e-5 -- except where a summed gradient component is itself of the
    size of Adam's epsilon (1e-8): there lr m / (sqrt(v) + eps) turns a last-bit difference of the fp32 sum into 1e-5 .. 1e-4 of x.  A fixed
    fp32 order still differs from the float64 sum in such a component, so the criterion is not tightened here."""
    err = np.abs(got - ref)
    assert (err > TOL).mean() < 1e-3 and err.max() < 2e-4, ((err > TOL).mean(), err.max())


# ---- 3. gradient parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, B", [(SMALL, 1024), (BIG, 2048), (BIG, 32768)])
@pytest.mark.parametrize("with_pop", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_planned_gradient_matches_the_float64_oracle(dev, d, with_pop, shape, B):
    from pda_amd import ops
    (nU, nI), regs, seed, tag = shape, 1e-2, 31, 7
    users, pos, neg = zipf_batch(seed, nU, nI, B)
    cnt = check_batch(users, pos, neg, nI, B)
    U, I = tables(d + B, nU, nI, d, 0.3)                        # large enough that ELU sees both branches
    pp, pn = pops(seed, B) if with_pop else (None, None)
    fw = po.bpr_forward(U, I, users, pos, neg, pp, pn)
    ref_loss = po.bpr_loss(fw, regs, B)
    rgU, rgI = po.dense_grads(nU, nI, users, pos, neg, *po.bpr_grads(fw, regs, B, pp, pn))

    Ut, It, ut, pt, nt, ppt, pnt = to(dev, U, I, users, pos, neg, pp, pn)
    gU, gI = torch.zeros_like(Ut), torch.zeros_like(It)
    tagU, tagI = ops.adam_row_tags(nU, nI, dev)
    loss = torch.zeros(3, device=dev)
    plan = ops.triplet_plan(ut, pt, nt)[0]
    ops.bpr_grad_plan(Ut, It, ut, pt, nt, ppt, pnt, regs=regs, reg_div=B, plan=plan, gU=gU, gI=gI, tagU=tagU, tagI=tagI, step=tag, loss_acc=loss)
    torch.cuda.synchronize()
    got_loss, got_gU, got_gI = loss.cpu().numpy(), gU.cpu().numpy(), gI.cpu().numpy()
    print("loss err", np.abs(got_loss - ref_loss).max(), "gU err", np.abs(got_gU - rgU).max(), "gI err", np.abs(got_gI - rgI).max())
    np.testing.assert_allclose(got_loss, ref_loss, atol=TOL, rtol=TOL)
    np.testing.assert_allclose(got_gU, rgU, atol=TOL)
    np.testing.assert_allclose(got_gI, rgI, atol=TOL)
    # the same arrays within train_ref's a-priori rounding bound, which scales with 1 / B like the gradients (the median |gU| at B = 32768 is
    # 3e-6: atol = 1e-5 accepts zeros there)
    one = np.ones(B, np.float32)
    bnd = train_ref.bound(train_ref.Case(U, I, users, pos, neg, pp if with_pop else one, pn if with_pop else one, regs), with_pop, tables=False)
    for name, got, ref in (("gU", got_gU, rgU), ("gI", got_gI, rgI)):
        err = np.abs(got - ref)
        print(name, "largest err / bound", (err / np.where(bnd[name] > 0, bnd[name], 1.0)).max())
        assert (err <= bnd[name]).all(), name
    assert np.abs(got_loss - ref_loss).max() <= bnd["loss"].max() and (np.abs(got_loss - ref_loss) <= bnd["loss"]).all()
    in_u = np.zeros(nU, bool)
    in_u[users] = True
    in_i = cnt > 0
    assert not got_gU[~in_u].any() and not got_gI[~in_i].any(), "rows outside the batch stay zero"
    np.testing.assert_array_equal(tagU.cpu().numpy(), np.where(in_u, tag, 0))
    np.testing.assert_array_equal(tagI.cpu().numpy(), np.where(in_i, tag, 0))
    assert torch.equal(Ut.cpu(), torch.from_numpy(U)) and torch.equal(It.cpu(), torch.from_numpy(I)), "no table row is written"
    # without tags (the lazy phases): the same gradients, bit for bit
    gU2, gI2 = torch.zeros_like(Ut), torch.zeros_like(It)
    ops.bpr_grad_plan(Ut, It, ut, pt, nt, ppt, pnt, regs=regs, reg_div=B, plan=plan, gU=gU2, gI=gI2)
    assert torch.equal(gU2, gU) and torch.equal(gI2, gI)


# ---- 4. optimiser parity -------------------------------------------------------------------------------------------------------------
def _three_steps_oracle(U, I, batches, regs, B, lr):
    Ur, Ir, state, losses = U.astype(np.float64), I.astype(np.float64), None, []
    for t, (users, pos, neg, pp, pn) in enumerate(batches, 1):
        Ur, Ir, state, ref_loss = po.train_step(Ur, Ir, users, pos, neg, pp, pn, regs, B, lr, "adam", state, t)
        losses.append(ref_loss)
    return Ur, Ir, state, losses


def _small_case():
    (nU, nI), d, B, regs, lr = SMALL, 64, 1024, 1e-2, 1e-2
    U, I = tables(23, nU, nI, d, 0.1)
    batches = []
    for seed in (31, 32, 33):
        users, pos, neg = zipf_batch(seed, nU, nI, B)
        check_batch(users, pos, neg, nI, B)
        batches.append((users, pos, neg) + pops(seed, B))
    return nU, nI, d, B, regs, lr, U, I, batches


def _check_first_step(st, U, I, batch, regs):
    """After step 1 the tables the step read still equal the oracle's inputs bit for bit: all four moment tables against one oracle step, within
    train_ref's propagated rounding bound (max |v| is 1e-9 here: the atol = 1e-5 of _check_against_oracle cannot fail on it)."""
    users, pos, neg, pp, pn = batch
    c = train_ref.Case(U, I, users, pos, neg, pp, pn, regs)
    ref, bnd = train_ref.reference(c, True), train_ref.bound(c, True)
    for k in ("mU", "vU", "mI", "vI"):
        err = np.abs(st[k].cpu().numpy() - ref[k])
        print(k, "first step: largest err / bound", (err / np.where(bnd[k] > 0, bnd[k], 1.0)).max())
        assert (err <= bnd[k]).all(), k


def _check_against_oracle(got, ref, losses, ref_losses):
    (Ut, It, st), (Ur, Ir, state) = got, ref
    for l, r in zip(losses, ref_losses):
        print("loss err", np.abs(l - np.asarray(r)).max())
        np.testing.assert_allclose(l, r, atol=TOL, rtol=TOL)
    for k in ("mU", "vU", "mI", "vI"):
        print(k, "err", np.abs(st[k].cpu().numpy() - state[k]).max())
        np.testing.assert_allclose(st[k].cpu().numpy(), state[k], atol=TOL)
    for g, r in ((Ut, Ur), (It, Ir)):
        err = np.abs(g.cpu().numpy() - r)
        print("table err max", err.max(), "share > 1e-5", (err > TOL).mean())
        adam_close(g.cpu().numpy(), r)


def _adam_state(Ut, It):
    return {k: torch.zeros_like(t) for k, t in (("mU", Ut), ("vU", Ut), ("gU", Ut), ("mI", It), ("vI", It), ("gI", It))}


@pytest.mark.parametrize("path", ["adam_step_plan", "adam_step"])
def test_three_adam_steps_match_the_oracle(dev, path):
    """adam_step_plan, and as a companion the default two-launch step (ops.adam_step), which was only ever compared with other library paths."""
    from pda_amd import ops
    nU, nI, d, B, regs, lr, U, I, batches = _small_case()
    ref = _three_steps_oracle(U, I, batches, regs, B, lr)
    Ut, It = to(dev, U, I)
    st = _adam_state(Ut, It)
    tagU, tagI = ops.adam_row_tags(nU, nI, dev)
    losses = []
    for t, b in enumerate(batches, 1):
        ut, pt, nt, ppt, pnt = to(dev, *b)
        loss = torch.zeros(3, device=dev)
        common = dict(regs=regs, reg_div=B, step=t, lr_t=ops.adam_lr_t(lr, t), loss_acc=loss)
        if path == "adam_step_plan":
            ops.adam_step_plan(Ut, st["mU"], st["vU"], st["gU"], tagU, It, st["mI"], st["vI"], st["gI"], tagI, ut, pt, nt, ppt, pnt,
                               plan=ops.triplet_plan(ut, pt, nt)[0], **common)
        else:
            ops.adam_step(Ut, st["mU"], st["vU"], st["gU"], tagU, It, st["mI"], st["vI"], st["gI"], tagI, ut, pt, nt, ppt, pnt, **common)
        losses.append(loss.cpu().numpy())
        assert float(st["gU"].abs().max()) == 0.0 and float(st["gI"].abs().max()) == 0.0   # accumulators reset by the sweep
        if t == 1:
            _check_first_step(st, U, I, b, regs)
    _check_against_oracle((Ut, It, st), ref[:3], losses, ref[3])


def _model(dev, nU, nI, d, B, regs, lr, U, I, extra=()):
    from pda_amd import model_api
    from pda_amd.parse import parse_args
    a = parse_args(["--deterministic", "1", "--batch_size", str(B), "--embed_size", str(d), "--regs", str(regs), "--lr", str(lr), "--verbose", "0"]
                   + list(extra))
    m = model_api.ConditionalBPRMF(a, {"n_users": nU, "n_items": nI}, device=dev)
    m.weights["user_embedding"].copy_(torch.from_numpy(U))
    m.weights["item_embedding"].copy_(torch.from_numpy(I))
    return m


@pytest.mark.parametrize("optimizer", ["adam", "lazy_adam"])
def test_three_model_steps_with_the_flag_match_the_oracle(dev, optimizer):
    """adam: the three steps against the oracle's.  lazy_adam (the planned gradient + pda_adam_rows_f32 on the batch's rows) is the oracle's Adam
    step on the rows a batch touches and nothing elsewhere: every step is compared with ONE oracle step from the model's own state before it --
    the touched rows of tables and moments at test_lazy_adam_rows_matches_dense_on_touched_rows' tolerance, every other row bit for bit."""
    nU, nI, d, B, regs, lr, U, I, batches = _small_case()
    m = _model(dev, nU, nI, d, B, regs, lr, U, I, ("--optimizer", optimizer))
    assert m.deterministic and not m.adam_exact_lazy
    if optimizer == "adam":
        ref = _three_steps_oracle(U, I, batches, regs, B, lr)
        losses = []
        for t, b in enumerate(batches, 1):
            losses.append(m.train_step(*to(dev, *b)).cpu().numpy().copy())             # (no plan given: train_step makes it)
            if t == 1:
                _check_first_step(m._state, U, I, b, regs)
        _check_against_oracle((m.weights["user_embedding"], m.weights["item_embedding"], m._state), ref[:3], losses, ref[3])
        return

    def snapshot():
        st = m._opt_state()
        return {"U": m.weights["user_embedding"].cpu().numpy().copy(), "I": m.weights["item_embedding"].cpu().numpy().copy(),
                **{k: st[k].cpu().numpy().copy() for k in ("mU", "vU", "mI", "vI")}}

    for t, b in enumerate(batches, 1):
        before = snapshot()
        state = {k: before[k].astype(np.float64) for k in ("mU", "vU", "mI", "vI")}
        Ur, Ir, state, ref_loss = po.train_step(before["U"].astype(np.float64), before["I"].astype(np.float64), *b, regs, B, lr, "adam", state, t)
        loss = m.train_step(*to(dev, *b)).cpu().numpy().copy()
        print("step", t, "loss err", np.abs(loss - np.asarray(ref_loss)).max())
        np.testing.assert_allclose(loss, ref_loss, atol=TOL, rtol=TOL)
        after = snapshot()
        ru, ri = np.unique(b[0]), np.unique(np.concatenate([b[1], b[2]]))
        for keys, rows, n in ((("U", "mU", "vU"), ru, nU), (("I", "mI", "vI"), ri, nI)):
            idle = np.setdiff1d(np.arange(n), rows)
            assert len(rows) > 0 and len(idle) > 0
            for k, r in zip(keys, (Ur if keys[0] == "U" else Ir, state[keys[1]], state[keys[2]])):
                print("step", t, k, "err on the touched rows", np.abs(after[k][rows] - r[rows]).max())
                np.testing.assert_allclose(after[k][rows], r[rows], atol=TOL)
                np.testing.assert_array_equal(after[k][idle], before[k][idle])
    assert float(m._state["gU"].abs().max()) == 0.0 and float(m._state["gI"].abs().max()) == 0.0     # accumulators cleared behind the update


# ---- 5. bit identity -----------------------------------------------------------------------------------------------------------------
def _big_case(dev, B):
    (nU, nI), d, regs, lr = BIG, 64, 1e-2, 1e-2
    U, I = tables(5 + B, nU, nI, d, 0.1)
    batches = []
    for seed in (31, 32, 33):
        users, pos, neg = zipf_batch(seed, nU, nI, B)
        check_batch(users, pos, neg, nI, B)
        batches.append(to(dev, users, pos, neg, *pops(seed, B)))
    return nU, nI, d, regs, lr, U, I, batches


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("B", [2048, 32768])
def test_the_same_steps_give_the_same_bits(dev, B):
    """Five repetitions of a healthy computation, three cache policies, and the composite step against its two halves."""
    from pda_amd import ops
    nU, nI, d, regs, lr, U, I, batches = _big_case(dev, B)
    plans = [ops.triplet_plan(b[0], b[1], b[2])[0].clone() for b in batches]

    def run(policy=ops.ADAM_CACHE_AUTO, split=False):
        Ut, It = to(dev, U, I)
        st = _adam_state(Ut, It)
        tagU, tagI = ops.adam_row_tags(nU, nI, dev)
        losses = []
        for t, (b, plan) in enumerate(zip(batches, plans), 1):
            loss = torch.zeros(3, device=dev)
            lr_t = ops.adam_lr_t(lr, t)
            if split:
                ops.bpr_grad_plan(Ut, It, *b, regs=regs, reg_div=B, plan=plan, gU=st["gU"], gI=st["gI"], tagU=tagU, tagI=tagI, step=t, loss_acc=loss)
                ops.adam_dense_sweep4(Ut, st["mU"], st["vU"], st["gU"], tagU, It, st["mI"], st["vI"], st["gI"], tagI, t, lr_t, cache_policy=policy)
            else:
                ops.adam_step_plan(Ut, st["mU"], st["vU"], st["gU"], tagU, It, st["mI"], st["vI"], st["gI"], tagI, *b, regs=regs, reg_div=B, step=t,
                                   lr_t=lr_t, plan=plan, cache_policy=policy, loss_acc=loss)
            losses.append(loss.view(torch.int32).clone())
        torch.cuda.synchronize()
        return [Ut, It, st["mU"], st["vU"], st["mI"], st["vI"]] + losses

    first = run()
    assert not torch.equal(first[0], torch.from_numpy(U).to(dev)) and all(torch.isfinite(x.view(torch.float32)).all() for x in first[6:])
    for rep in range(4):
        assert _same(run(), first), "repetition %d differs" % (rep + 2)
    assert _same(run(ops.ADAM_CACHE_RESIDENT), first), "PDA_ADAM_CACHE_RESIDENT"
    assert _same(run(ops.ADAM_CACHE_STREAM), first), "PDA_ADAM_CACHE_STREAM"
    assert _same(run(split=True), first), "adam_step_plan != bpr_grad_plan + adam_dense_sweep4"


@pytest.mark.parametrize("B", [2048, 32768])
def test_sweep_and_replay_give_the_same_bits_with_the_flag(dev, B):
    """--adam_sweep sweep and replay (after sync_optimizer): without the flag they agree to a tolerance only, because their gradients are summed
    by atomics in whatever order they land."""
    nU, nI, d, regs, lr, U, I, batches = _big_case(dev, B)
    out = {}
    for mode in ("sweep", "replay"):
        m = _model(dev, nU, nI, d, B, regs, lr, U, I, ("--adam_sweep", mode))
        assert m.adam_exact_lazy == (mode == "replay")
        losses = [m.train_step(*b).view(torch.int32).clone() for b in batches]
        m.sync_optimizer()
        torch.cuda.synchronize()
        st = m._state
        out[mode] = [m.weights["user_embedding"], m.weights["item_embedding"], st["mU"], st["vU"], st["mI"], st["vI"]] + losses
    assert _same(out["sweep"], out["replay"])


# ---- 6. the rejected batch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2048, 32768])
@pytest.mark.parametrize("call", ["bpr_grad_plan", "adam_step_plan"])
def test_a_batch_with_a_user_twice_is_rejected_and_nothing_moves(dev, B, call):
    from pda_amd import ops
    (nU, nI), d, regs, seed = BIG, 64, 1e-2, 32
    users, pos, neg = zipf_batch(seed, nU, nI, B)
    check_batch(users, pos, neg, nI, B)
    users[B // 2] = users[3]
    assert len(np.unique(users)) == B - 1
    U, I = tables(9, nU, nI, d, 0.1)
    rng = np.random.default_rng(10)
    Ut, It, ut, pt, nt, ppt, pnt = to(dev, U, I, users, pos, neg, *pops(seed, B))
    st = _adam_state(Ut, It)
    for k in ("mU", "vU", "mI", "vI"):          # moments a decay would move
        st[k].copy_(torch.from_numpy(rng.uniform(0.1, 1.0, tuple(st[k].shape)).astype(np.float32)))
    tagU, tagI = ops.adam_row_tags(nU, nI, dev)
    tagU.fill_(2)
    tagI.fill_(2)
    bufs = [Ut, It, st["mU"], st["vU"], st["gU"], st["mI"], st["vI"], st["gI"], tagU, tagI, ut, pt, nt, ppt, pnt]
    before = [x.clone() for x in bufs]
    plan = ops.triplet_plan(ut, pt, nt)[0]
    assert ops.plan_header(plan)[1] == 1
    plan_before = plan.clone()
    loss = torch.zeros(3, device=dev)
    if call == "bpr_grad_plan":
        ops.bpr_grad_plan(Ut, It, ut, pt, nt, ppt, pnt, regs=regs, reg_div=B, plan=plan, gU=st["gU"], gI=st["gI"], tagU=tagU, tagI=tagI, step=3,
                          loss_acc=loss)
    else:
        ops.adam_step_plan(Ut, st["mU"], st["vU"], st["gU"], tagU, It, st["mI"], st["vI"], st["gI"], tagI, ut, pt, nt, ppt, pnt, regs=regs, reg_div=B,
                           step=3, lr_t=ops.adam_lr_t(1e-2, 3), plan=plan, loss_acc=loss)
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss).all()), loss
    assert _same(bufs, before) and torch.equal(plan, plan_before)


# ---- 7. metrics ----------------------------------------------------------------------------------------------------------------------
def test_ordered_metrics_meet_the_reference_vectors(dev):
    from pda_amd import ops
    cases = json.load(open(os.path.join(G, "metrics.json")))
    assert len(cases) >= 11
    groups = sorted({(len(c["r"]), tuple(c["Ks"])) for c in cases})           # every list length: one call per (length, cut-offs)
    assert {(50, (20, 50)), (50, (1, 5, 10, 50))} < set(groups)
    done = 0
    for k_cols, Ks in groups:
        sub = [c for c in cases if len(c["r"]) == k_cols and tuple(c["Ks"]) == Ks]
        done += len(sub)
        topk = torch.tensor([c["r"] for c in sub], dtype=torch.int32, device=dev)
        indptr = np.zeros(len(sub) + 1, np.int64)
        indptr[1:] = np.cumsum([len(c["target"]) for c in sub])
        flat = np.concatenate([np.asarray(c["target"], np.int32) for c in sub])
        reduce = ops.metrics_route(k_cols, ordered=True)                      # (lists beyond 64 columns: the deep kernel's ordered sums)
        assert reduce is (ops.metrics_sums_ordered if k_cols <= 64 else ops.metrics_sums_deep_ordered)
        sums = reduce(topk, torch.from_numpy(indptr).to(dev), torch.from_numpy(flat).to(dev),
                      torch.tensor(Ks, dtype=torch.int32, device=dev)).cpu().numpy()
        for row, k in enumerate(("precision", "recall", "ndcg", "hit_ratio")):
            ref = np.sum([c["out"][k] for c in sub], axis=0)
            np.testing.assert_allclose(sums[row], ref, rtol=1e-12, err_msg=k)
    assert done == len(cases)


def test_ordered_metrics_equal_the_atomic_ones_and_repeat_bit_for_bit(dev):
    from pda_amd import ops
    rng = np.random.default_rng(4)
    n, K, nI = 100000, 50, 1000
    topk = torch.from_numpy(np.argsort(rng.random((n, 64)), axis=1)[:, :K].astype(np.int32) * 15 + rng.integers(0, 15, (n, 1)).astype(np.int32)).to(dev)
    lens = rng.integers(0, 11, n)                                   # (users without targets add zero: tests/metrics_ref.py; the reference's recall there is 0/0)
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum(lens)
    flat = rng.integers(0, nI, int(indptr[-1])).astype(np.int32)
    ip, fl = torch.from_numpy(indptr).to(dev), torch.from_numpy(flat).to(dev)
    ks = torch.tensor([1, 20, 50], dtype=torch.int32, device=dev)
    ref = ops.metrics_sums(topk, ip, fl, ks)
    got = ops.metrics_sums_ordered(topk, ip, fl, ks)
    assert float(ref[1].min()) > 0
    rel = ((got - ref).abs() / ref.abs()).max()
    print("ordered vs atomic, max relative difference", float(rel))
    assert float(rel) <= 1e-12
    for _ in range(4):
        assert torch.equal(ops.metrics_sums_ordered(topk, ip, fl, ks).view(torch.int64), got.view(torch.int64))
    twice = ops.metrics_sums_ordered(topk, ip, fl, ks, got.clone())     # `sums` is added to
    assert torch.equal(twice, got + got)


# ---- 8. end to end -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from pda_amd import synthetic
    root = tmp_path_factory.mktemp("data")
    synthetic.write_dataset(str(root / "toy"), n_users=400, n_items=300, mean_hist=20)
    return str(root) + "/"


def _masked(out):
    """The wall-clock fields of the log: `Epoch %d [%.1fs]` and the `time:` of an evaluation."""
    out = re.sub(r"\[\d+\.\d+s\]", "[T]", out)
    return re.sub(r"time: ?\s*[0-9.e+-]+", "time: T", out).splitlines()


@pytest.mark.parametrize("train, extra", [("s_condition", ()), ("normal", ()), ("s_condition", ("--adam_sweep", "replay")),
                                          ("s_condition", ("--optimizer", "sgd", "--lr", "0.05"))])
def test_two_runs_print_the_same_log_and_keep_the_same_checkpoint(dev, toy, tmp_path, capsys, train, extra):
    from pda_amd import train_new_api as t
    save = str(tmp_path) + "/"
    argv = ["--data_path", toy, "--dataset", "toy", "--train", train, "--test", train, "--epoch", "5", "--log_interval", "2", "--batch_size", "256",
            "--lr", "1e-2", "--regs", "1e-2", "--valid_set", "valid", "--pop_exp", "0.22", "--save_dir", save, "--Ks", "[20,50]", "--save_flag", "0",
            "--saveID", "t", "--cuda", "0", "--eval_block", "128", "--deterministic", "1"] + list(extra)
    logs, ckpts = [], []
    for _ in range(2):
        capsys.readouterr()
        t.main(argv)
        logs.append(_masked(capsys.readouterr().out))
        found = sorted(os.path.join(r, f) for r, _, fs in os.walk(tmp_path) for f in fs if f.endswith(".ckpt"))
        assert any(f.endswith("best_ckpt.ckpt") for f in found)
        ckpts.append({os.path.basename(f): torch.load(f, map_location="cpu") for f in found})
    a, b = logs
    assert sum("recall=[" in l for l in a) >= 2 and any(l.startswith("Epoch 4 [T]") for l in a)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x == y, "line %d differs:\n%s\n%s" % (i, x, y)
    assert ckpts[0].keys() == ckpts[1].keys()
    for name in ckpts[0]:
        s0, s1 = ckpts[0][name], ckpts[1][name]
        assert s0.keys() == s1.keys()
        for k in s0:
            if torch.is_tensor(s0[k]):
                assert torch.equal(s0[k], s1[k]), (name, k)
            else:
                assert s0[k] == s1[k], (name, k)
