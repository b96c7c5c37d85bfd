"""GPU: MACR (`--train macr`, include/pda_hip_macr.h) -- the three-branch gradient step against the float64 restatement of tests/macr_ref.py,
its flags, tags, saturation and id skip, the whole Adam step over the tables and the branch vectors, graph replay, the item prep, the lists
against the fp32 contract and against the float64 model, and the CLI.

Tolerances: 1e-5 absolute on every loss term and gradient element (macr_ref.tolerance; tests/test_macr_host.py shows that the restatement in
float32 stays inside a quarter of it on the same inputs, gW included), 1e-5 on tables, branch vectors and moments after three Adam steps, 1e-6
on sig and J, 1e-4 on the saturated loss terms.  The lists are bit-equal to the contract; against the float64 model every returned item lies
within 2 E of the K-th value, E the rounding bound derived in macr_ref.rounding_bound."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from macr_ref import (BATCHES, DIMS, KINDS, LIST_CS, LIST_DIMS, LIST_KS, LIST_SHAPES, NI, NU, REGS, TOL, WEIGHTS, batch, branches, contract_lists, list_case,
                      macr_adam, macr_grads, model_values, parity_case, rounding_bound, tables, tolerance)

pytestmark = pytest.mark.gpu
LOG1E10 = -np.log(1e-10)


def to(dev, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


def run_grads(dev, U, I, wi, wu, b, alpha, beta, reg_div, step=1, **kw):
    from pda_amd import ops
    Ut, It, wit, wut, ut, pt, nt = to(dev, U, I, wi, wu, *b)
    st = ops.MacrState(Ut, It)
    loss = torch.zeros(5, device=dev)
    ops.macr_grads(Ut, It, wit, wut, ut, pt, nt, st, alpha=alpha, beta=beta, regs=REGS, reg_div=reg_div, step=step, loss_acc=loss, **kw)
    return (loss.cpu().numpy(), st.gU.cpu().numpy(), st.gI.cpu().numpy(), st.gW.cpu().numpy()), st


@functools.lru_cache(maxsize=None)
def reference(d, B, kind, alpha, beta):
    U, I, wi, wu, b = parity_case(d, B, kind)
    return macr_grads(U, I, wi, wu, *b, alpha=alpha, beta=beta, regs=REGS, reg_div=B)


def check(got, ref, what, alpha=None, beta=None):
    names = ("loss", "gU", "gI", "gW")
    print("macr %s: " % what + "  ".join("max |%s err| %.3g" % (n, np.abs(g - r).max()) for n, g, r in zip(names, got, ref)) + "  (bound %.3g)" % TOL)
    for n, g, r in zip(names, got, ref):
        np.testing.assert_allclose(g, r, atol=tolerance(n), rtol=0, err_msg=n)
    if alpha is not None:
        t = got[0]
        assert abs(t[0] - (t[1] + alpha * t[2] + beta * t[3] + t[4])) <= TOL


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("d", DIMS)
def test_loss_and_gradients_against_the_float64_restatement(dev, d, B, kind):
    """All five loss terms and all four gradients, for the three (alpha, beta) pairs.  64 users and 40 items: at B = 2 048 every row sums dozens
    of occurrences and gW sums 2 048 terms across many workgroups.  The tags: exactly the batch's distinct rows, with the step's tag."""
    U, I, wi, wu, b = parity_case(d, B, kind)
    for alpha, beta in WEIGHTS:
        got, st = run_grads(dev, U, I, wi, wu, b, alpha, beta, B, step=5)
        check(got, reference(d, B, kind, alpha, beta), "%s d=%d B=%d alpha=%g beta=%g" % (kind, d, B, alpha, beta), alpha, beta)
        S_u, S_i = np.unique(b[0]), np.unique(np.concatenate([b[1], b[2]]))
        tagU, tagI = st.tagU.cpu().numpy(), st.tagI.cpu().numpy()
        assert (np.nonzero(tagU)[0] == S_u).all() and (np.nonzero(tagI)[0] == S_i).all() and set(tagU[S_u]) == {5} and set(tagI[S_i]) == {5}
    if B == 2048:
        assert len(S_u) == NU and len(S_i) == NI
    if B == 2048 and kind == "spread":          # the branch gradients are far above the bound, and not equal to each other
        gW = got[3]
        assert np.abs(gW[0]).max() > 100 * TOL and np.abs(gW[1]).max() > 100 * TOL and not np.allclose(gW[0], gW[1], atol=10 * TOL)


@pytest.mark.parametrize("d", [32, 256])
def test_a_grouped_batch_and_distinct_users_take_the_other_paths(dev, d):
    """The two flags of pda_adam_step_f32: a batch grouped by positive without PDA_UPD_ANY_ORDER (runs of equal positives are combined), and
    PDA_UPD_USERS_DISTINCT (the user rows take plain stores).  Same gradients."""
    rng = np.random.default_rng(7 * d)
    U, I = tables(rng, d)
    wi, wu = (3 * w for w in branches(rng, d))
    users, pos, neg = batch(rng, 300)
    order = np.argsort(pos, kind="stable")
    b = (users[order], pos[order], neg[order])
    ref = macr_grads(U, I, wi, wu, *b, alpha=0.5, beta=0.25, regs=REGS, reg_div=300)
    check(run_grads(dev, U, I, wi, wu, b, 0.5, 0.25, 300, grouped=True)[0], ref, "grouped d=%d" % d)
    b = (rng.permutation(NU).astype(np.int32),) + batch(rng, NU)[1:]
    ref = macr_grads(U, I, wi, wu, *b, alpha=0.5, beta=0.25, regs=REGS, reg_div=NU)
    for grouped in (False, True):       # (an ungrouped batch under the grouped rule: equal positives apart are separate atomics, still the same sum)
        check(run_grads(dev, U, I, wi, wu, b, 0.5, 0.25, NU, users_distinct=True, grouped=grouped)[0], ref, "distinct users d=%d" % d)


@pytest.mark.parametrize("d", [32, 128])
def test_saturated_sigmoids_stay_finite(dev, d):
    """a_p = -100 and a_n = +40 on a triplet, branch dots of +-40: 1 - sigmoid(x) + 1e-10 is computed as written, so a saturated term is
    -log(1e-10), never inf, and every gradient is finite.  Coordinates 0, 1, 2 carry y, the item branch and the user branch."""
    rng = np.random.default_rng(d)
    U, I = tables(rng, d, 8, 8)
    wi, wu = np.zeros(d, np.float32), np.zeros(d, np.float32)
    wi[1], wu[2] = 40.0, 40.0
    U[:, 1:3], I[:, 1:3] = 0.0, 0.0
    U[0, :3] = (10.0, 0.0, 1.0)          # s_u = sigmoid(40) = 1
    U[1, :3] = (10.0, 0.0, -1.0)         # s_u = sigmoid(-40) = 4e-18
    I[0, :3] = (-10.0, 1.0, 0.0)         # s = 1; with user 0: y = -100 + small, a_p = -100
    I[1, :3] = (4.0, 1.0, 0.0)           # s = 1; with user 0: y = +40, a_n = +40
    I[2, :3] = (1.0, -1.0, 0.0)          # s = 4e-18
    U[0, 3:], I[0, 3:], I[1, 3:] = 0.0, 0.0, 0.0
    one = lambda u, p, n: tuple(np.int32([x]) for x in (u, p, n))      # noqa: E731
    # (user 0, positive 0, negative 1): L_O = 2 x -log(1e-10); L_I: s_p = 1 -> 0, s_n = 1 -> -log(1e-10); L_U: s_u = 1 -> -log(1e-10)
    got, _ = run_grads(dev, U, I, wi, wu, one(0, 0, 1), 0.5, 0.25, 1)
    print("macr saturated d=%d: terms %s" % (d, got[0]))
    np.testing.assert_allclose(got[0][1:4], [2 * LOG1E10, LOG1E10, LOG1E10], atol=1e-4, rtol=0)
    # (user 1, positive 2, negative 2): a = 0 (both s vanish): L_O = 2 log 2; L_I: s_p = 4e-18 -> -log(1e-10), s_n -> 0; L_U: -log(1e-10)
    got2, _ = run_grads(dev, U, I, wi, wu, one(1, 2, 2), 0.5, 0.25, 1)
    np.testing.assert_allclose(got2[0][1:4], [2 * np.log(2.0), LOG1E10, LOG1E10], atol=1e-4, rtol=0)
    # a batch that mixes them with ordinary triplets: finite everywhere, and the terms of the float64 restatement
    b = (np.int32([0, 1, 3, 0, 5, 1]), np.int32([0, 2, 4, 1, 0, 5]), np.int32([1, 2, 5, 0, 2, 1]))
    got3, _ = run_grads(dev, U, I, wi, wu, b, 0.5, 0.25, 6)
    for g in got + got2 + got3:
        assert np.isfinite(g).all()
    ref = macr_grads(U, I, wi, wu, *b, alpha=0.5, beta=0.25, regs=REGS, reg_div=6)
    np.testing.assert_allclose(got3[0], ref[0], atol=1e-4, rtol=0)


def test_ops_checks_ids_and_the_kernel_skips_a_triplet_outside_the_tables(dev):
    """Ids outside the tables are read by the bounds check and never dereferenced: the batch equals the batch without those triplets (the means
    still divide by B)."""
    from pda_amd import ops
    U, I, wi, wu, _ = parity_case(32, 7, "spread")
    rng = np.random.default_rng(1)
    b = batch(rng, 9)
    Ut, It, wit, wut, ut, pt, nt = to(dev, U, I, wi, wu, *b)
    kw = dict(alpha=0.5, beta=0.25, regs=REGS, reg_div=9, step=1)
    bad_p, bad_u, bad_n = pt.clone(), ut.clone(), nt.clone()
    bad_p[4], bad_u[6], bad_n[0] = NI, -1, 2 ** 31 - 1
    st = ops.MacrState(Ut, It)
    with pytest.raises(ValueError, match="outside the tables"):
        ops.macr_grads(Ut, It, wit, wut, ut, bad_p, nt, st, **kw)
    with pytest.raises(TypeError, match="w_item"):
        ops.macr_grads(Ut, It, wit.double(), wut, ut, pt, nt, st, **kw)
    with pytest.raises(ValueError, match="d float32 each"):
        ops.macr_grads(Ut, It, wit[:-1].contiguous(), wut, ut, pt, nt, st, **kw)
    with pytest.raises(ValueError, match="embedding width"):
        ops.macr_grads(Ut[:, :24].contiguous(), It[:, :24].contiguous(), wit[:24].contiguous(), wut[:24].contiguous(), ut, pt, nt,
                       ops.MacrState(Ut[:, :24].contiguous(), It[:, :24].contiguous()), **kw)
    assert float(st.gU.abs().max()) == 0.0 and float(st.gW.abs().max()) == 0.0 and int(st.tagU.abs().max()) == 0          # nothing was launched
    keep = ~np.isin(np.arange(9), [4, 6, 0])
    b6 = [x[keep] for x in b]
    loss = torch.zeros(5, device=dev)
    ops.macr_grads(Ut, It, wit, wut, bad_u, bad_p, bad_n, st, loss_acc=loss, check_ids=False, **kw)
    ref = macr_grads(U, I, wi, wu, *b6, alpha=0.5, beta=0.25, regs=REGS, reg_div=9, B=9)
    check((loss.cpu().numpy(), st.gU.cpu().numpy(), st.gI.cpu().numpy(), st.gW.cpu().numpy()), ref, "three skipped")
    assert set(np.nonzero(st.tagU.cpu().numpy())[0]) == set(b6[0]) and set(np.nonzero(st.tagI.cpu().numpy())[0]) == set(b6[1]) | set(b6[2])
    st = ops.MacrState(Ut, It)          # every triplet skipped: nothing moves
    loss = torch.zeros(5, device=dev)
    ops.macr_grads(Ut, It, wit, wut, torch.full_like(ut, -1), pt, nt, st, loss_acc=loss, check_ids=False, **kw)
    assert float(loss.abs().max()) == 0.0 and float(st.gU.abs().max()) == 0.0 and float(st.gI.abs().max()) == 0.0 and float(st.gW.abs().max()) == 0.0


@pytest.mark.parametrize("d", [32, 256])
def test_a_refused_triplet_inside_a_run_of_equal_positives(dev, d):
    """The contract of the shared scatter of the positives' gradients (pos_scatter_any / pos_run_head / pos_scatter_run, pda_train_common.h) where
    its callers differ: a workgroup holds TPB = 512 / (d / 4) triplets, the batch TPB + 3 (the run crosses a workgroup boundary, the last workgroup
    is mostly empty), every positive is the same item, and two triplets are refused by the kernel -- triplet 2 (pos = n_items) inside the run of
    the first workgroup, triplet TPB (users = -1) at the head of the second.  Under either rule the batch equals the kept triplets with the
    means over the whole B, and the tags are set on exactly the kept triplets' rows."""
    TPB = 512 // (d // 4)
    B = TPB + 3
    rng = np.random.default_rng(11 * d)
    U, I = tables(rng, d)
    wi, wu = (3 * w for w in branches(rng, d))
    users, pos, neg = batch(rng, B)
    pos[:] = 7
    pos[2], users[TPB] = NI, -1
    keep = ~np.isin(np.arange(B), [2, TPB])
    kept = [x[keep] for x in (users, pos, neg)]
    ref = macr_grads(U, I, wi, wu, *kept, alpha=0.5, beta=0.25, regs=REGS, reg_div=B, B=B)
    for grouped in (False, True):
        got, st = run_grads(dev, U, I, wi, wu, (users, pos, neg), 0.5, 0.25, B, step=5, grouped=grouped, check_ids=False)
        check(got, ref, "refused inside a run d=%d grouped=%d" % (d, grouped), 0.5, 0.25)
        S_u, S_i = np.unique(kept[0]), np.unique(np.concatenate(kept[1:]))
        tagU, tagI = st.tagU.cpu().numpy(), st.tagI.cpu().numpy()
        assert (np.nonzero(tagU)[0] == S_u).all() and (np.nonzero(tagI)[0] == S_i).all() and set(tagU[S_u]) == {5} and set(tagI[S_i]) == {5}


@pytest.mark.parametrize("d", [32, 128])
def test_three_whole_steps_against_the_restatement(dev, d):
    """Tables, branch vectors and all moments after three steps, within 1e-5; the gradient accumulators are zero behind every step."""
    from pda_amd import ops
    B, lr = 64, 1e-2
    rng = np.random.default_rng(33 + d)
    U, I = tables(rng, d)
    W = np.stack([3 * w for w in branches(rng, d)])
    Ut, It, wit, wut = to(dev, U, I, W[0], W[1])
    st = ops.MacrState(Ut, It)
    Ur, Ir, Wr, state = U.astype(np.float64), I.astype(np.float64), W.astype(np.float64), None
    for t in (1, 2, 3):
        b = batch(rng, B)
        Ur, Ir, Wr, state, terms = macr_adam(Ur, Ir, Wr, state, t, lr, *b, alpha=0.5, beta=0.25, regs=REGS, reg_div=B)
        loss = torch.zeros(5, device=dev)
        ops.macr_adam_step(Ut, It, wit, wut, *to(dev, *b), st, alpha=0.5, beta=0.25, regs=REGS, reg_div=B, step=t, lr_t=ops.adam_lr_t(lr, t),
                           loss_acc=loss, check_ids=True)
        np.testing.assert_allclose(loss.cpu().numpy(), terms, atol=TOL, rtol=0)
        assert float(st.gU.abs().max()) == 0.0 and float(st.gI.abs().max()) == 0.0 and float(st.gW.abs().max()) == 0.0
    got = dict(U=Ut, I=It, W=torch.stack([wit, wut]), mU=st.mU, vU=st.vU, mI=st.mI, vI=st.vI, mW=st.mW, vW=st.vW)
    ref = dict(U=Ur, I=Ir, W=Wr, **state)
    for k in got:
        print("macr three steps d=%d: max |%s err| %.3g" % (d, k, np.abs(got[k].cpu().numpy() - ref[k]).max()))
    for k in got:
        np.testing.assert_allclose(got[k].cpu().numpy(), ref[k], atol=TOL, rtol=0, err_msg=k)
    assert np.abs(Wr - W).max() > 100 * TOL             # (the branch vectors did move)


def test_untouched_rows_take_the_dense_decay_of_the_bpr_step(dev):
    """After one pda_macr_adam_step_f32 the rows outside the batch equal, bit for bit, the idle rows of pda_adam_step_f32 on the same tables (the
    same sweep kernel, g = 0), and the gradient tables are zero again."""
    from pda_amd import ops
    d, B, lr_t = 64, 16, 3e-3
    rng = np.random.default_rng(21)
    U, I = tables(rng, d, 300, 200)
    wi, wu = branches(rng, d)
    mom = [np.abs(rng.standard_normal(x.shape)).astype(np.float32) * 1e-3 for x in (U, U, I, I)]
    b = batch(rng, B, 300, 200)
    Ut, It, wit, wut, ut, pt, nt = to(dev, U, I, wi, wu, *b)
    st = ops.MacrState(Ut, It)
    for t, m in zip((st.mU, st.vU, st.mI, st.vI), mom):
        t.copy_(torch.from_numpy(m))
    ops.macr_adam_step(Ut, It, wit, wut, ut, pt, nt, st, alpha=1e-3, beta=1e-3, regs=REGS, reg_div=B, step=1, lr_t=lr_t)
    U2, I2, mU, vU, mI, vI = to(dev, U, I, *mom)
    gU, gI = torch.zeros_like(U2), torch.zeros_like(I2)
    tagU, tagI = ops.adam_row_tags(300, 200, dev)
    ops.adam_step(U2, mU, vU, gU, tagU, I2, mI, vI, gI, tagI, ut, pt, nt, regs=REGS, reg_div=B, step=1, lr_t=lr_t)
    idleU = np.setdiff1d(np.arange(300), b[0])
    idleI = np.setdiff1d(np.arange(200), np.concatenate([b[1], b[2]]))
    assert len(idleU) >= 280 and len(idleI) >= 160
    for got, ref, rows in ((Ut, U2, idleU), (st.mU, mU, idleU), (st.vU, vU, idleU), (It, I2, idleI), (st.mI, mI, idleI), (st.vI, vI, idleI)):
        r = torch.from_numpy(rows).to(dev)
        assert torch.equal(got[r], ref[r])
    assert not torch.equal(Ut[int(b[0][0])], U2[int(b[0][0])])        # (the batch's rows do differ: another loss)
    assert float(st.gU.abs().max()) == 0.0 and float(st.gI.abs().max()) == 0.0 and float(st.gW.abs().max()) == 0.0
    assert torch.equal(st.tagU, tagU) and torch.equal(st.tagI, tagI)
    assert not torch.equal(wit.cpu(), torch.from_numpy(wi)) and not torch.equal(wut.cpu(), torch.from_numpy(wu))


def test_the_step_replays_from_a_captured_graph(dev):
    """pda_macr_adam_step_f32 reads nothing back on the host: two steps (tags 1 and 2) captured once and replayed give the parameters of the
    same two steps launched directly."""
    from pda_amd import ops
    d, B = 64, 200
    rng = np.random.default_rng(5)
    U, I = tables(rng, d)
    wi, wu = branches(rng, d)
    bt = to(dev, *batch(rng, B))

    def two_steps(P, st, loss):
        for t in (1, 2):
            ops.macr_adam_step(*P, *bt, st, alpha=0.5, beta=0.25, regs=REGS, reg_div=B, step=t, lr_t=ops.adam_lr_t(1e-2, t), loss_acc=loss)
    Pa = to(dev, U, I, wi, wu)
    sa, la = ops.MacrState(Pa[0], Pa[1]), torch.zeros(5, device=dev)
    two_steps(Pa, sa, la)
    Pb = to(dev, U, I, wi, wu)
    sb, lb = ops.MacrState(Pb[0], Pb[1]), torch.zeros(5, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            two_steps(Pb, sb, lb)
    torch.cuda.synchronize()
    assert torch.equal(Pb[0].cpu(), torch.from_numpy(U)) and torch.equal(Pb[2].cpu(), torch.from_numpy(wi))        # capturing runs nothing
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(Pb, Pa):
        torch.testing.assert_close(x, y, atol=2e-6, rtol=0)
    torch.testing.assert_close(lb, la, atol=1e-5, rtol=0)
    assert not torch.equal(Pb[2].cpu(), torch.from_numpy(wi))


@pytest.mark.parametrize("d", DIMS)
def test_item_prep_against_float64_and_bit_stable(dev, d):
    from pda_amd import ops
    rng = np.random.default_rng(d)
    n = 1037                                                           # not a multiple of the rows of a workgroup
    I = (rng.standard_normal((n, d)) * 0.3).astype(np.float32)
    w = (rng.standard_normal(d) * 4.0 / np.sqrt(d)).astype(np.float32)
    It, wt = to(dev, I, w)
    one, two = ops.macr_item_prep(It, wt), ops.macr_item_prep(It, wt)
    assert torch.equal(one.sig.view(torch.int32), two.sig.view(torch.int32)) and torch.equal(one.J.view(torch.int32), two.J.view(torch.int32))
    s64 = 1.0 / (1.0 + np.exp(-(I.astype(np.float64) @ w.astype(np.float64))))
    sig, J = one.sig.cpu().numpy(), one.J.cpu().numpy()
    print("macr item prep d=%d: max |sig err| %.3g  max |J err| %.3g  sig in %.3f .. %.3f" % (d, np.abs(sig - s64).max(),
                                                                                           np.abs(J - s64[:, None] * I).max(), sig.min(), sig.max()))
    assert s64.min() < 0.1 and s64.max() > 0.9
    np.testing.assert_allclose(sig, s64, atol=1e-6, rtol=0)
    np.testing.assert_allclose(J, s64[:, None] * I.astype(np.float64), atol=1e-6, rtol=0)
    np.testing.assert_array_equal(J, sig[:, None] * I)                 # J = fl(sig_i I_i), element for element
    for c in (-1.0, 0.37):
        np.testing.assert_array_equal(ops.macr_item_bias(one.sig, c).cpu().numpy(), np.float32(-c) * sig)
    assert one.bias(0.37) is one.bias(0.37)


@functools.lru_cache(maxsize=None)
def list_inputs(shape, d):
    return list_case(*shape, d)


@pytest.mark.parametrize("K", LIST_KS)
@pytest.mark.parametrize("d", LIST_DIMS)
@pytest.mark.parametrize("shape", LIST_SHAPES)
def test_lists_equal_the_contract_and_respect_the_float64_model(dev, monkeypatch, shape, d, K):
    """200 users x 4 096 items through the pre-filtered bias kernel (the library's choice wherever an item prep exists) and 200 x 300 through
    the exact one (PDA_TEMP_POP_KERNEL=exact: the kernel a call without a usable prep falls back to), c in -1, 0, 0.37, 1, user 0 with 40
    unlisted items.  Ids and values: bit-equal to the contract top_k(fl(chain(u . J_i) + fl(-c sig_i)) + mask) restated in numpy
    on ops.score_dense(U, J).  Against the float64 (y - c) s_i: every returned unlisted item's value is at least the row's K-th value minus
    2 max_i E (macr_ref.rounding_bound: E bounds |contract - model| per pair from d, |y| (A), |c| and s_i, so an item more than 2 E below the
    K-th value has K items above it in the contract, too).  tests/test_macr_host.py checks that these inputs' own float64 lists are separated
    by more than that bound."""
    from pda_amd import ops
    U, I, w, users, hist = list_inputs(shape, d)
    nI = shape[1]
    generation = 3 if nI >= 4096 else 1
    if generation == 1:
        monkeypatch.setenv("PDA_TEMP_POP_KERNEL", "exact")
    else:
        monkeypatch.delenv("PDA_TEMP_POP_KERNEL", raising=False)
    Ut, It, wt, ut = to(dev, U, I, w, users)
    indptr = np.zeros(len(hist) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(h) for h in hist])
    h = ops.HistoryCSR(*to(dev, indptr, np.concatenate(hist).astype(np.int32)), by_user=True)
    prep = ops.macr_item_prep(It, wt)
    s = ops.score_dense(Ut, prep.J, ut, ops.HEAD_RAW).cpu().numpy()
    sig = prep.sig.cpu().numpy()
    for c in LIST_CS:
        stats = {}
        idx, val = ops.recommend_topk_macr(Ut, It, wt, ut, c, K, h, prep=prep, stats=stats)
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        assert ops.bias_kernel_identity(stats["kernel_id"].cpu().numpy()[0]) == {"generation": generation, "bias_head": True, "d": d}
        want, hc = contract_lists(s, sig, c, K, hist)
        np.testing.assert_array_equal(idx, want)
        np.testing.assert_array_equal(val, np.take_along_axis(hc, want.astype(np.int64), 1))
        v, E = model_values(U, I, w, users, c), rounding_bound(U, I, w, users, c)
        worst = 0.0
        for r, items in enumerate(hist):
            free = np.ones(nI, bool)
            free[items] = False
            kth = np.sort(v[r, free])[::-1][min(K, int(free.sum())) - 1]
            got = idx[r][free[idx[r]]]
            assert len(got) == min(K, int(free.sum())) and len(set(got)) == len(got)
            slack = 2 * E[r, free].max()
            worst = max(worst, float((kth - v[r, got]).max() / slack))
            assert (v[r, got] >= kth - slack).all(), (c, r)
        print("macr lists %s d=%d K=%d c=%g: largest (K-th - value) / bound %.3g" % (shape, d, K, c, worst))
    # without a prep the call builds one: the same lists
    idx2, val2 = ops.recommend_topk_macr(Ut, It, wt, ut, LIST_CS[-1], K, h)
    assert torch.equal(idx2.cpu(), torch.from_numpy(idx)) and torch.equal(val2.cpu(), torch.from_numpy(val))


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------------
def test_cli_trains_macr_and_the_checkpoint_restores(dev, tmp_path):
    """python -m pda_amd.train_new_api --train macr --test macr in a child process, two epochs on the smallest synthetic dataset, --step 5: it
    ends, the losses are finite and decrease, c = 0 is evaluated first, a best c from the grid or 0 is printed, best_ckpt.ckpt restores into a
    MACRBPRMF with the same lists, and a BPRMF refuses it."""
    from pda_amd import synthetic
    from pda_amd import train_new_api as t
    from pda_amd.model_api import BPRMF, MACRBPRMF
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    synthetic.write_dataset(str(tmp_path / "data" / "toy"), n_users=200, n_items=150, mean_hist=12)
    argv = ["--data_path", str(tmp_path / "data") + "/", "--dataset", "toy", "--train", "macr", "--test", "macr", "--epoch", "2", "--embed_size", "64",
            "--log_interval", "1", "--batch_size", "128", "--lr", "1e-2", "--regs", "1e-3", "--valid_set", "valid", "--pop_exp", "0.22",
            "--save_dir", str(tmp_path / "ckpt") + "/", "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t", "--cuda", "0", "--eval_block", "128",
            "--step", "5", "--alpha", "1e-2", "--beta", "1e-2"]
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "pda_amd.train_new_api"] + argv, cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert "running MACR" in out and "recall=[" in out and "---- MACR without c:" in out and "training and testing end!!!!" in out
    assert out.count("MACR without c\n") == 2 and "best expo" not in out
    losses = [[float(x) for x in m.groups()] for m in re.finditer(r"Epoch \d+ \[[^\]]*\]: train==\[([-\d.]+)=([-\d.]+) \+ ([-\d.]+)\]", out)]
    assert len(losses) == 2 and np.isfinite(losses).all() and losses[1][0] < losses[0][0] and losses[1][1] < losses[0][1], losses
    assert losses[0][1] < 2 * np.log(2.0) * 1.05                      # L_O starts at 2 log 2, the branch terms weigh 1e-2
    grid = [0.0] + [float(c) for c in np.linspace(-1, 1, 5)]
    tried = [float(m.group(1)) for m in re.finditer(r"^c: ([-\d.]+) best c: [-\d.]+$", out, re.M)]
    assert tried == grid[1:] * 2
    best = [float(m.group(1)) for m in re.finditer(r"MACR best c: ([-\d.]+)", out)]
    assert len(best) == 2 and all(min(abs(b - g) for g in grid) < 1e-6 for b in best)
    ck = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path / "ckpt") for f in fs if f == "best_ckpt.ckpt"]
    assert len(ck) == 1 and "macr_train_macr" in ck[0]
    sd = torch.load(ck[0], map_location=dev)
    assert sd["model"] == "macr" and sd["format"] == "pda_amd/2" and sd["embed_size"] == 64 and sd["w_item"].shape == (64, 1) and "mW" in sd
    assert min(abs(sd["macr_c"] - g) for g in grid) < 1e-6
    # the final report ranks with the stored c
    assert "(c = %.6f)" % sd["macr_c"] in out

    t.configure(argv)
    data = t.data
    cfg = {"n_users": data.n_users, "n_items": data.n_items}
    with pytest.raises(ValueError, match="checkpoint of a macr model cannot be loaded into BPRMF"):
        BPRMF(t.args, cfg, device=dev).load_state_dict(sd)
    from pda_amd.sampler import DeviceSampler
    model = t.DatasetApi_Model(t.args, cfg, 128, DeviceSampler(data, dev, False), dev)
    rec = model.Recommender
    assert isinstance(rec, MACRBPRMF)
    rec.load_state_dict(sd)
    assert rec.c == rec.best_c == sd["macr_c"] and rec._t == sd["adam_t"]
    users = np.asarray(list(data.valid_user_list.keys())[:100], dtype=np.int32)
    ev = t.evaluation(data, [20, 50], dev, block=128)
    ev.set_evaluate_obj_pre("valid")
    idx, val = model.recommend_device(users, None, "macr", mask=ev._hist)
    # the same lists from the saved parameters through ops alone, and values that are (y - c) s_i up to rounding
    idx2, val2 = ops_lists(dev, sd, users, ev._hist)
    assert torch.equal(idx, idx2) and torch.equal(val, val2)
    dense = model.testing(None, users, list(range(data.n_items)), "macr")
    U, I = sd["user_embedding"].cpu().numpy().astype(np.float64), sd["item_embedding"].cpu().numpy().astype(np.float64)
    sg = lambda x: 1 / (1 + np.exp(-x))                                # noqa: E731
    want = (U[users] @ I.T - sd["macr_c"]) * sg(I @ sd["w_item"].cpu().numpy().astype(np.float64)).T * sg(U[users] @ sd["w_user"].cpu().numpy().astype(np.float64))
    np.testing.assert_allclose(dense, want, atol=1e-5, rtol=0)
    np.testing.assert_allclose(model.predict(users, None), dense, atol=0, rtol=0)
    np.testing.assert_allclose(np.take_along_axis(want / sg(U[users] @ sd["w_user"].cpu().numpy().astype(np.float64)), idx.cpu().numpy().astype(np.int64), 1),
                               val.cpu().numpy(), atol=1e-5, rtol=0)


def ops_lists(dev, sd, users, hist):
    from pda_amd import ops
    ut = torch.from_numpy(users).to(dev)
    return ops.recommend_topk_macr(sd["user_embedding"], sd["item_embedding"], sd["w_item"], ut, sd["macr_c"], 50, hist)
