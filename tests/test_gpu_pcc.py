"""GPU: the popularity-correlation regulariser (`--train pcc`, include/pda_hip_pcc.h) -- the gradient step against the float64 restatement of
tests/pcc_ref.py, the batch statistic against the float64 moments of the kernel's own scores, the degenerate batches against the plain BPR step,
triplets outside the tables, the other scatter paths, the whole Adam step, graph replay, and the CLI.

Tolerances (pcc_ref.tolerance): 1e-5 max(1, 4 gamma / sqrt(Szz)) absolute on every loss term and gradient element, Szz from the float64
restatement: |d pen / d z_t| <= 4 gamma / sqrt(Szz), and every gradient entry is that coefficient times a quantity the BPR tests hold to 1e-5;
1e-5 where r = 0 by rule.  tests/test_pcc_host.py shows that the restatement in float32 stays inside a quarter of these bounds on the same
inputs.  1e-5 on tables and moments after three Adam steps; 1e-12 relative on the statistic against float64 moments of the same float32 scores."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pcc_ref import COUNTS, DIMS, NI, NU, ONS, TOL, batch, parity_case, pcc_adam, pcc_grads, pcc_pop, tables, tolerance

pytestmark = pytest.mark.gpu
REGS = 1e-2
GAMMA = 10.0


def to(dev, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


class State:
    """What ops.pcc_grads / ops.pcc_adam_step write besides the tables."""

    def __init__(self, Ut, It, B):
        from pda_amd import ops
        z = torch.zeros_like
        self.mU, self.vU, self.gU, self.mI, self.vI, self.gI = z(Ut), z(Ut), z(Ut), z(It), z(It), z(It)
        self.tagU, self.tagI = ops.adam_row_tags(Ut.shape[0], It.shape[0], Ut.device)
        self.z_ws, self.stat = ops.pcc_workspace(B, Ut.device)
        self.pcc = torch.zeros(2, dtype=torch.float32, device=Ut.device)

    def adam(self, Ut, It):
        return (Ut, self.mU, self.vU, self.gU, self.tagU, It, self.mI, self.vI, self.gI, self.tagI)


def run_grads(dev, U, I, b, pop, reg_div, *, gamma=GAMMA, on="pos", step=1, **kw):
    from pda_amd import ops
    Ut, It, ut, pt, nt, qt = to(dev, U, I, *b, pop)
    st = State(Ut, It, len(b[0]))
    loss = torch.zeros(3, device=dev)
    ops.pcc_grads(Ut, It, ut, pt, nt, qt, st.gU, st.gI, st.tagU, st.tagI, gamma=gamma, on=on, regs=REGS, reg_div=reg_div, step=step,
                  z_ws=st.z_ws, stat=st.stat, loss_acc=loss, pcc_acc=st.pcc, **kw)
    return loss.cpu().numpy(), st.gU.cpu().numpy(), st.gI.cpu().numpy(), st


@functools.lru_cache(maxsize=None)
def reference(d, B, on):
    U, I, b, pop = parity_case(d, B)
    return pcc_grads(U, I, *b, pop, gamma=GAMMA, on=on, regs=REGS, reg_div=B)


def check(got, ref, tol, what):
    loss, gU, gI = got
    terms, rU, rI = ref[:3]
    print("pcc %s: max |loss err| %.3g  max |gU err| %.3g  max |gI err| %.3g  (bound %.3g)" % (what, np.abs(loss - terms).max(), np.abs(gU - rU).max(),
                                                                                           np.abs(gI - rI).max(), tol))
    assert np.isfinite(loss).all() and np.isfinite(gU).all() and np.isfinite(gI).all()
    np.testing.assert_allclose(loss, terms, atol=tol, rtol=0)
    np.testing.assert_allclose(gU, rU, atol=tol, rtol=0)
    np.testing.assert_allclose(gI, rI, atol=tol, rtol=0)
    assert abs(loss[0] - (loss[1] + loss[2])) <= tol


def check_tags(st, b, tag):
    S_u, S_i = np.unique(b[0]), np.unique(np.concatenate([b[1], b[2]]))
    tagU, tagI = st.tagU.cpu().numpy(), st.tagI.cpu().numpy()
    assert (np.nonzero(tagU)[0] == S_u).all() and (np.nonzero(tagI)[0] == S_i).all() and set(tagU[S_u]) == {tag} and set(tagI[S_i]) == {tag}


def moments64(z, q):
    """float64 [8] the way the kernel lays it out, from float32 scores and popularities (numpy, centred)."""
    z, q = z.astype(np.float64), q.astype(np.float64)
    n = len(z)
    if n == 0:
        return np.zeros(8)
    zb, qb = z.sum() / n, q.sum() / n
    Szz, Sqq, Szq = ((z - zb) ** 2).sum(), ((q - qb) ** 2).sum(), ((z - zb) * (q - qb)).sum()
    r = Szq / np.sqrt(Szz * Sqq) if n >= 2 and Szz > 0 and Sqq > 0 else 0.0
    return np.array([n, zb, qb, Szz, Sqq, Szq, r, 0.0])


def check_stat(stat, z, q, what):
    """1e-12 relative, each entry against the size of the terms it is summed from."""
    want = moments64(z, q)
    za, qa = np.abs(z.astype(np.float64)).max(initial=0.0), np.abs(q.astype(np.float64)).max(initial=0.0)
    scale = np.array([1.0, za, qa, want[3], want[4], np.sqrt(want[3] * want[4]), 1.0, 1.0])
    err = np.abs(stat - want)
    print("pcc stat %s: max relative error %.3g (bound 1e-12), r = %.6f" % (what, (err / np.maximum(scale, 1e-300)).max(), stat[6]))
    assert stat[0] == want[0] and stat[7] == 0.0
    assert (err <= 1e-12 * scale).all(), (stat, want)


# ---- 1. gradients and loss -------------------------------------------------------------------------------------------------------------------
def cases():
    out = [(d, B) for d in DIMS for B in (1, 2, 3, 7, 2048)]
    return out + [(32, 512 // (32 // 4) + 3), (256, 512 // (256 // 4) + 3)]      # TPB + 3: a batch crosses a workgroup boundary, the last one is partial


@pytest.mark.parametrize("on", ONS)
@pytest.mark.parametrize("d, B", cases())
def test_gradients_and_loss_against_the_float64_restatement(dev, d, B, on):
    assert cases()[-2:] == [(32, 67), (256, 11)]
    U, I, b, pop = parity_case(d, B)
    ref = reference(d, B, on)
    loss, gU, gI, st = run_grads(dev, U, I, b, pop, B, on=on, step=5)
    check((loss, gU, gI), ref, tolerance(GAMMA, ref[3]), "%s d=%d B=%d" % (on, d, B))
    check_tags(st, b, 5)
    stat = st.stat.cpu().numpy()
    np.testing.assert_allclose(stat[[0, 1, 2]], ref[3][[0, 1, 2]], atol=1e-5, rtol=0)
    np.testing.assert_allclose(st.pcc.cpu().numpy(), [stat[6], stat[6] ** 2], atol=1e-6, rtol=0)     # once per step, whatever the grid
    if B == 2048:       # every item is hot: about a hundred summed occurrences per row
        assert len(np.unique(b[1])) == NI


# ---- 2. the statistic ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", ONS)
@pytest.mark.parametrize("d, B", [(32, 2048), (64, 7), (128, 1025), (256, 2048), (32, 5125)])      # (5 125: five rounds of the one-workgroup loop, the last one partial)
def test_the_statistic_is_the_float64_moments_of_its_own_scores_and_keeps_its_bits(dev, d, B, on):
    from pda_amd import ops
    rng = np.random.default_rng(13 * d + B)
    U, I = tables(rng, d)
    b = batch(rng, B)
    pop = pcc_pop(rng.integers(0, 1000, NI), "log")                      # arbitrary float32 popularities: their float32 sums do round
    Ut, It, ut, pt, nt, qt = to(dev, U, I, *b, pop)
    z1, s1 = ops.pcc_stats(Ut, It, ut, pt, nt, qt, on=on)
    z2, s2 = ops.pcc_stats(Ut, It, ut, pt, nt, qt, on=on)
    assert torch.equal(z1.view(torch.int32), z2.view(torch.int32)) and torch.equal(s1.view(torch.int64), s2.view(torch.int64))
    z, stat = z1.cpu().numpy(), s1.cpu().numpy()
    U64, I64 = U.astype(np.float64), I.astype(np.float64)
    sp, sn = (U64[b[0]] * I64[b[1]]).sum(1), (U64[b[0]] * I64[b[2]]).sum(1)
    want = sp if on == "pos" else sp - sn
    print("pcc z_ws %s d=%d B=%d: max |err| %.3g (bound 1e-5)" % (on, d, B, np.abs(z - want).max()))
    np.testing.assert_allclose(z, want, atol=1e-5, rtol=0)
    check_stat(stat, z, pop[b[1]], "%s d=%d B=%d" % (on, d, B))
    assert stat[0] == B and stat[6] != 0.0


# ---- 3. degenerate batches are the BPR step --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", ONS)
@pytest.mark.parametrize("B", [7, 2048])
@pytest.mark.parametrize("d", DIMS)
def test_gamma_zero_is_the_plain_bpr_step(dev, d, B, on):
    from pda_amd import ops
    U, I, b, pop = parity_case(d, B)
    loss, gU, gI, st = run_grads(dev, U, I, b, pop, B, gamma=0.0, on=on)
    Ut, It, ut, pt, nt = to(dev, U, I, *b)
    hU, hI, hl = torch.zeros_like(Ut), torch.zeros_like(It), torch.zeros(3, device=dev)
    ops.bpr_step(Ut, It, ut, pt, nt, regs=REGS, reg_div=B, mode=ops.UPD_DENSE_GRAD, gU=hU, gI=hI, loss_acc=hl)
    check((loss, gU, gI), (hl.cpu().numpy(), hU.cpu().numpy(), hI.cpu().numpy()), TOL, "gamma = 0 against pda_bpr_step_f32, %s d=%d B=%d" % (on, d, B))
    stat = st.stat.cpu().numpy()
    assert stat[6] != 0.0 and float(st.pcc[0]) == np.float32(stat[6])                # r is still reported


@pytest.mark.parametrize("on", ONS)
@pytest.mark.parametrize("case", ["constant_pop", "one_triplet", "one_positive"])
def test_degenerate_batches_are_the_bpr_step(dev, case, on):
    """r = 0 by rule, exactly: every positive equally popular (Sqq = 0 exactly, by centring), one triplet (Szz = 0 exactly).  gamma = 10: the
    loss and the gradients are those of the BPR loss, and nothing is NaN."""
    d = 64
    rng = np.random.default_rng(77)
    U, I = tables(rng, d)
    pop, b = pcc_pop(COUNTS), batch(rng, 67)
    if case == "constant_pop":
        pop = np.full(NI, np.float32(3.7))
    elif case == "one_triplet":
        b = tuple(x[:1] for x in b)
    else:
        b[1][:] = 11
    B = len(b[0])
    loss, gU, gI, st = run_grads(dev, U, I, b, pop, B, on=on)
    ref = pcc_grads(U, I, *b, pop, gamma=0.0, on=on, regs=REGS, reg_div=B)           # the BPR objective
    assert tolerance(GAMMA, pcc_grads(U, I, *b, pop, gamma=GAMMA, on=on, regs=REGS, reg_div=B)[3]) == TOL
    check((loss, gU, gI), ref, TOL, "%s %s" % (case, on))
    stat = st.stat.cpu().numpy()
    assert np.isfinite(stat).all() and stat[0] == B and stat[6] == 0.0 and (stat[3] if case == "one_triplet" else stat[4]) == 0.0
    assert st.pcc.cpu().numpy().tolist() == [0.0, 0.0] and np.isfinite(st.z_ws.cpu().numpy()).all()


# ---- 4. triplets outside the tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", ONS)
@pytest.mark.parametrize("grouped", [False, True])
def test_ops_checks_ids_and_the_kernels_skip_triplets_outside_the_tables(dev, grouped, on):
    from pda_amd import ops
    d, B = 32, 40
    rng = np.random.default_rng(1)
    U, I = tables(rng, d)
    pop = pcc_pop(COUNTS)
    b = batch(rng, B)
    order = np.argsort(b[1], kind="stable")
    b = tuple(x[order] for x in b)
    bad = tuple(x.copy() for x in b)
    bad[0][4], bad[1][17], bad[2][30] = NU, -3, NI                     # a user, a positive, a negative
    keep = ~np.isin(np.arange(B), [4, 17, 30])
    kept = [x[keep] for x in b]
    Ut, It, ut, pt, nt, qt = to(dev, U, I, *bad, pop)
    st = State(Ut, It, B)
    with pytest.raises(ValueError, match="outside the tables"):
        ops.pcc_grads(Ut, It, ut, pt, nt, qt, st.gU, st.gI, st.tagU, st.tagI, gamma=GAMMA, on=on, regs=REGS, reg_div=B, step=1)
    with pytest.raises(TypeError, match="pop"):
        ops.pcc_grads(Ut, It, ut, pt, nt, qt.double(), st.gU, st.gI, st.tagU, st.tagI, gamma=GAMMA, on=on, regs=REGS, reg_div=B, step=1, check_ids=False)
    with pytest.raises(ValueError, match="--pcc_gamma"):
        ops.pcc_grads(Ut, It, ut, pt, nt, qt, st.gU, st.gI, st.tagU, st.tagI, gamma=-1.0, on=on, regs=REGS, reg_div=B, step=1, check_ids=False)
    assert float(st.gU.abs().max()) == 0.0 and int(st.tagU.abs().max()) == 0           # nothing was launched
    loss, gU, gI, st = run_grads(dev, U, I, bad, pop, B, on=on, step=5, grouped=grouped, check_ids=False)
    ref = pcc_grads(U, I, *kept, pop, gamma=GAMMA, on=on, regs=REGS, reg_div=B, B=B)   # 1 / B still counts the three
    check((loss, gU, gI), ref, tolerance(GAMMA, ref[3]), "three skipped, %s grouped=%d" % (on, grouped))
    check_tags(st, kept, 5)
    z, stat = st.z_ws.cpu().numpy(), st.stat.cpu().numpy()
    check_stat(stat, z[keep], pop[kept[1]], "three skipped")
    assert stat[0] == B - 3 and (z[~keep] == 0).all()
    # every triplet skipped: n_v = 0, nothing moves
    loss, gU, gI, st = run_grads(dev, U, I, (np.full(B, -1, np.int32), b[1], b[2]), pop, B, on=on, grouped=grouped, check_ids=False)
    assert np.abs(loss).max() == 0.0 and np.abs(gU).max() == 0.0 and np.abs(gI).max() == 0.0 and (st.stat.cpu().numpy() == 0).all()


@pytest.mark.parametrize("on", ONS)
@pytest.mark.parametrize("d", [32, 256])
def test_a_refused_triplet_inside_a_run_of_equal_positives(dev, d, on):
    """A workgroup holds TPB = 512 / (d / 4) triplets, the batch TPB + 3; the positives are two items of different popularity in two runs, the
    first crossing the workgroup boundary; two triplets are refused by the kernel -- triplet 2 (pos = n_items) inside the run of the first
    workgroup, triplet TPB (users = -1) at the head of the second.  Under either rule the batch equals the kept triplets with 1 / B over the
    whole B and the statistic over the kept ones, and the tags are set on exactly the kept triplets' rows."""
    TPB = 512 // (d // 4)
    B = TPB + 3
    rng = np.random.default_rng(11 * d)
    U, I = tables(rng, d)
    pop = pcc_pop(COUNTS)
    users, pos, neg = batch(rng, B)
    pos[:TPB + 1], pos[TPB + 1:] = 7, 9
    assert pop[7] != pop[9]
    pos[2], users[TPB] = NI, -1
    keep = ~np.isin(np.arange(B), [2, TPB])
    kept = [x[keep] for x in (users, pos, neg)]
    ref = pcc_grads(U, I, *kept, pop, gamma=GAMMA, on=on, regs=REGS, reg_div=B, B=B)
    assert ref[3][6] != 0.0
    for grouped in (False, True):
        loss, gU, gI, st = run_grads(dev, U, I, (users, pos, neg), pop, B, on=on, step=5, grouped=grouped, check_ids=False)
        check((loss, gU, gI), ref, tolerance(GAMMA, ref[3]), "refused inside a run d=%d %s grouped=%d" % (d, on, grouped))
        check_tags(st, kept, 5)
        assert float(st.stat[0]) == B - 2


# ---- 5. the other scatter paths --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", ONS)
@pytest.mark.parametrize("d", [32, 256])
def test_a_grouped_batch_and_distinct_users_take_the_other_paths(dev, d, on):
    rng = np.random.default_rng(7 * d)
    U, I = tables(rng, d)
    pop = pcc_pop(COUNTS)
    users, pos, neg = batch(rng, 300)
    order = np.argsort(pos, kind="stable")
    b = (users[order], pos[order], neg[order])
    ref = pcc_grads(U, I, *b, pop, gamma=GAMMA, on=on, regs=REGS, reg_div=300)
    check(run_grads(dev, U, I, b, pop, 300, on=on, grouped=True)[:3], ref, tolerance(GAMMA, ref[3]), "grouped d=%d %s" % (d, on))
    b = (rng.permutation(NU).astype(np.int32),) + batch(rng, NU)[1:]
    ref = pcc_grads(U, I, *b, pop, gamma=GAMMA, on=on, regs=REGS, reg_div=NU)
    for grouped in (False, True):       # (an ungrouped batch under the grouped rule: equal positives apart are separate atomics, still the same sum)
        check(run_grads(dev, U, I, b, pop, NU, on=on, users_distinct=True, grouped=grouped)[:3], ref, tolerance(GAMMA, ref[3]),
              "distinct users d=%d %s" % (d, on))


# ---- 6. whole steps --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", ONS)
def test_three_whole_steps_against_the_restatement(dev, on):
    from pda_amd import ops
    d, B, lr, gamma = 32, 64, 1e-2, 2.0
    rng = np.random.default_rng(33)
    U, I = tables(rng, d)
    pop = pcc_pop(COUNTS, "log")
    Ut, It, qt = to(dev, U, I, pop)
    st = State(Ut, It, B)
    Ur, Ir, state = U.astype(np.float64), I.astype(np.float64), None
    for t in (1, 2, 3):
        b = batch(rng, B)
        Ur, Ir, state, terms, stat = pcc_adam(Ur, Ir, state, t, lr, *b, pop, gamma=gamma, on=on, regs=REGS, reg_div=B)
        loss = torch.zeros(3, device=dev)
        ops.pcc_adam_step(*st.adam(Ut, It), *to(dev, *b), qt, st.z_ws, st.stat, gamma=gamma, on=on, regs=REGS, reg_div=B, step=t,
                          lr_t=ops.adam_lr_t(lr, t), loss_acc=loss, pcc_acc=st.pcc, check_ids=True)
        print("pcc three steps (%s) step %d: max |loss err| %.3g (bound %.3g)" % (on, t, np.abs(loss.cpu().numpy() - terms).max(), tolerance(gamma, stat)))
        np.testing.assert_allclose(loss.cpu().numpy(), terms, atol=tolerance(gamma, stat), rtol=0)
        assert float(st.gU.abs().max()) == 0.0 and float(st.gI.abs().max()) == 0.0
    got = dict(U=Ut, I=It, mU=st.mU, vU=st.vU, mI=st.mI, vI=st.vI)
    ref = dict(U=Ur, I=Ir, **state)
    for k in got:
        print("pcc three steps (%s): max |%s err| %.3g" % (on, k, np.abs(got[k].cpu().numpy() - ref[k]).max()))
    for k in got:
        np.testing.assert_allclose(got[k].cpu().numpy(), ref[k], atol=TOL, rtol=0, err_msg=k)


@pytest.mark.parametrize("on", ONS)
def test_untouched_rows_take_the_dense_decay_of_the_bpr_step(dev, on):
    """After one pda_pcc_adam_step_f32 the rows outside the batch equal, bit for bit, the idle rows of pda_adam_step_f32 on the same tables (the
    same sweep kernel, g = 0), and both gradient tables are zero again."""
    from pda_amd import ops
    d, B, lr_t = 32, 16, 3e-3
    rng = np.random.default_rng(21)
    U, I = tables(rng, d, 300, 200)
    mom = [np.abs(rng.standard_normal(x.shape)).astype(np.float32) * 1e-3 for x in (U, U, I, I)]
    b = batch(rng, B, 300, 200)
    pop = pcc_pop(rng.integers(0, 50, 200))
    Ut, It, ut, pt, nt, qt = to(dev, U, I, *b, pop)
    st = State(Ut, It, B)
    for t, m in zip((st.mU, st.vU, st.mI, st.vI), mom):
        t.copy_(torch.from_numpy(m))
    ops.pcc_adam_step(*st.adam(Ut, It), ut, pt, nt, qt, st.z_ws, st.stat, gamma=GAMMA, on=on, regs=REGS, reg_div=B, step=1, lr_t=lr_t)
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
    assert float(st.stat[6]) != 0.0 and not torch.equal(Ut[int(b[0][0])], U2[int(b[0][0])])        # (the batch's rows do differ: another loss)
    assert float(st.gU.abs().max()) == 0.0 and float(st.gI.abs().max()) == 0.0
    assert torch.equal(st.tagU, tagU) and torch.equal(st.tagI, tagI)


# ---- 7. graph replay -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", ONS)
def test_the_step_replays_from_a_captured_graph(dev, on):
    """pda_pcc_adam_step_f32 reads nothing back on the host -- the scores and the statistic stay in device memory: two steps (tags 1 and 2)
    captured once and replayed give the tables of the same two steps launched directly.  d = 64, B = 200: seven workgroups, and pcc_acc grows by
    (r, r^2) of each step once -- as the penalty does in loss_acc."""
    from pda_amd import ops
    d, B = 64, 200
    rng = np.random.default_rng(5)
    U, I = tables(rng, d)
    bt = to(dev, *batch(rng, B), pcc_pop(COUNTS))
    rs = []

    def two_steps(Ut, It, st, loss, record=False):
        for t in (1, 2):
            ops.pcc_adam_step(*st.adam(Ut, It), *bt, st.z_ws, st.stat, gamma=GAMMA, on=on, regs=REGS, reg_div=B, step=t,
                              lr_t=ops.adam_lr_t(1e-2, t), loss_acc=loss, pcc_acc=st.pcc)
            if record:
                rs.append(float(st.stat[6]))
    Ua, Ia = to(dev, U, I)
    sa, la = State(Ua, Ia, B), torch.zeros(3, device=dev)
    two_steps(Ua, Ia, sa, la, record=True)
    Ub, Ib = to(dev, U, I)
    sb, lb = State(Ub, Ib, B), torch.zeros(3, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            two_steps(Ub, Ib, sb, lb)
    torch.cuda.synchronize()
    assert torch.equal(Ub.cpu(), torch.from_numpy(U)) and float(sb.pcc.abs().max()) == 0.0      # capturing runs nothing
    g.replay()
    torch.cuda.synchronize()
    torch.testing.assert_close(Ub, Ua, atol=2e-6, rtol=0)
    torch.testing.assert_close(Ib, Ia, atol=2e-6, rtol=0)
    torch.testing.assert_close(lb, la, atol=1e-5, rtol=0)
    want = np.array([rs[0] + rs[1], rs[0] ** 2 + rs[1] ** 2])
    assert abs(rs[0]) > 1e-3 and abs(rs[1]) > 1e-3
    np.testing.assert_allclose(sa.pcc.cpu().numpy(), want, atol=1e-6, rtol=0)
    np.testing.assert_allclose(sb.pcc.cpu().numpy(), want, atol=1e-5, rtol=0)
    # the penalty is in loss_acc once per step: mf - bpr = gamma r^2, with bpr from the restatement of the first step
    ref = pcc_grads(U, I, *(x.cpu().numpy() for x in bt[:3]), pcc_pop(COUNTS), gamma=GAMMA, on=on, regs=REGS, reg_div=B)
    assert abs(ref[3][6] - rs[0]) <= 1e-5


# ---- 8. the CLI ------------------------------------------------------------------------------------------------------------------------------
def test_cli_trains_pcc_and_export_topk_restores_it(dev, tmp_path, capsys):
    """python -m pda_amd.train_new_api --train pcc --test normal in a child process, two epochs on the smallest synthetic dataset: it ends, prints
    the result lines and one `||--- pcc` line per epoch, writes a BPRMF-format best_ckpt.ckpt, and export_topk restores the checkpoint.  Then, in
    this process, --pcc_gamma 0 against --train normal on the same flags: r is still printed, and the losses are those of the BPR objective."""
    import re
    from pda_amd import export_topk, synthetic
    from pda_amd import train_new_api as t
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    synthetic.write_dataset(str(tmp_path / "data" / "toy"), n_users=200, n_items=150, mean_hist=12)

    def flags(train, test, save, *more):
        return ["--data_path", str(tmp_path / "data") + "/", "--dataset", "toy", "--train", train, "--test", test, "--epoch", "2", "--embed_size",
                "32", "--log_interval", "1", "--batch_size", "128", "--lr", "1e-2", "--regs", "1e-3", "--valid_set", "valid", "--pop_exp", "0.22",
                "--save_dir", str(tmp_path / save) + "/", "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t", "--cuda", "0", "--eval_block",
                "128"] + list(more)

    def lines(out):
        loss = [tuple(float(x) for x in m.groups()) for m in re.finditer(r"Epoch \d+ \[[^\]]*\]: train==\[([-\d.]+)=([-\d.]+) \+ ([-\d.]+)\]", out)]
        pcc = [tuple(float(x) for x in m.groups()) for m in re.finditer(r"^\|\|--- pcc r=([-\d.]+) r2=([-\d.]+) \(gamma=", out, flags=re.M)]
        return loss, pcc

    argv = flags("pcc", "normal", "ckpt", "--pcc_gamma", "2", "--pcc_on", "pos", "--pcc_pop", "log")
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "pda_amd.train_new_api"] + argv, cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert "running PCC" in out and "recall=[" in out and "best expo" in out and "training and testing end!!!!" in out
    loss, pcc = lines(out)
    assert len(loss) == 2 and len(pcc) == 2, out[-3000:]
    for (r1, r2) in pcc:
        assert -1.0 <= r1 <= 1.0 and r1 * r1 - 1e-4 <= r2 <= 1.0        # mean of r^2 >= (mean of r)^2
    ck = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path / "ckpt") for f in fs]
    best = [f for f in ck if f.endswith("best_ckpt.ckpt")]
    assert len(best) == 1 and "pcc_train_pcc" in best[0]
    sd = torch.load(best[0], map_location="cpu")
    assert "model" not in sd and sd["format"] == "pda_amd/2" and sd["embed_size"] == 32 and sd["user_embedding"].shape == (200, 32) and "mU" in sd
    assert (sd["pcc_gamma"], sd["pcc_on"], sd["pcc_pop"]) == (2.0, "pos", "log")
    res = export_topk.main(argv + ["--export_out", str(tmp_path / "lists.npz")])
    assert res["idx"].shape[1] == 50 and res["idx"].shape[0] == len(res["users"]) > 0 and np.isfinite(res["val"]).all()
    # gamma = 0: the BPR objective (the same sampler, the same seeds), r still reported
    capsys.readouterr()
    t.main(flags("pcc", "pcc", "ckpt0", "--pcc_gamma", "0"))
    loss0, pcc0 = lines(capsys.readouterr().out)
    t.main(flags("normal", "normal", "ckptn"))
    lossn, pccn = lines(capsys.readouterr().out)
    print("pcc cli: gamma = 0 losses", loss0, "--train normal losses", lossn, "r", pcc0)
    assert len(loss0) == 2 and len(lossn) == 2 and len(pcc0) == 2 and pccn == [] and all(abs(r1) > 0 for r1, _ in pcc0)
    # (printed to five decimals; the two runs take the same batches through two step kernels that agree to 1e-5 per step)
    np.testing.assert_allclose(np.array(loss0), np.array(lossn), atol=1e-3, rtol=0)
    assert loss[0][1] > loss0[0][1]                                      # and gamma = 2 did add its penalty to mf_loss
