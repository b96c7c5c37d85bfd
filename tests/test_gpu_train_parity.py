"""GPU: the reference's own train step (pda_bpr_step_f32 / _bf16 / _shard_f32, pda_sgd_apply_f32, pda_bpr_step_plan_f32, pda_bpr_grad_plan_f32,
pda_adam_step_f32) against the float64 oracle, element for element, within tests/train_ref.py's a-priori rounding bound -- a bound that scales
with 1 / B like the quantities it is applied to.  tests/test_train_parity_host.py shows on the CPU that an fp32 emulation of the kernels lies
inside this bound on every case used here, and that fifteen single-defect mutants of the reference leave it by more than 10x.

Every test prints its largest err / bound per quantity.  Observed on an MI355X (recorded, not thresholds):
    UPD_NONE                 loss 0.09, due 0.46, dpe 0.47, dne 0.44 (the largest at d = 256 with the popularity head; 0.22 .. 0.36 below that)
    UPD_DENSE_GRAD/adam_step loss 0.09, gU 0.06, gI 0.28, mU 0.23, mI 0.31, vU 0.21, vI 0.22
    UPD_SGD_FUSED            loss 0.07, U_sgd 0.96, I_sgd 0.98 (the bound of an updated row is little more than the half ulp of the final sum)
    sgd_step_exact / plan    loss 0.08, U_sgd 0.99, I_sgd 0.97
    bpr_grad_plan            loss 0.08, gU 0.08, gI 0.34
    bpr_step_bf16            loss 0.09, due 0.07, dpe 0.29, dne 0.31, U_sgd 0.98, I_sgd 0.98
    bpr_step_shard           loss 0.05, due 0.05, gI 0.16, U_sgd 0.96, I_sgd 0.98
    saturated                loss 0.06, due 0.27, dpe 0.30, dne 0.26, gU 0.27, gI 0.30, the mf of the x = -100 triplet 0.03
"""
import numpy as np
import pytest
import torch

import train_ref as tr

pytestmark = pytest.mark.gpu
F = np.float32
LRS = (0.05, 1.0)


def to(dev, *xs):
    return [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


def dev_case(dev, c, pop):
    """-> (U, I, users, pos, neg, pos_pop, neg_pop) on the device (fresh copies of the tables)."""
    return to(dev, c.U, c.I, c.users, c.pos, c.neg, *c.heads(pop))


class Worst:
    """The largest err / bound per quantity of one test; check() asserts element for element."""

    def __init__(self, title):
        self.title, self.w = title, {}

    def check(self, q, got, ref, bnd, where=""):
        got = np.asarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
        assert got.shape == np.shape(ref) and np.isfinite(got).all(), (q, where)
        err = np.abs(got - ref)
        assert ((bnd > 0) | (err == 0)).all(), (q, where, "error where the bound is exactly 0")
        ratio = float((err / np.where(bnd > 0, bnd, 1.0)).max())
        self.w[q] = max(self.w.get(q, 0.0), ratio)
        assert ratio <= 1.0, "%s %s: err / bound = %.3f (largest err %.3e)" % (q, where, ratio, err.max())

    def report(self):
        print("%s largest err / bound: %s" % (self.title, " ".join("%s %.3f" % kv for kv in sorted(self.w.items()))))


def cases_of(d, kinds):
    return [(B, kind) for dd, B, kind in tr.gpu_cases() if dd == d and kind in kinds]


def grads_out(dev, B, d):
    return tuple(torch.empty(B, d, device=dev) for _ in range(3))


# ---- ops.bpr_step(mode=UPD_NONE, grads_out=...) --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pop", [False, True])
@pytest.mark.parametrize("d", tr.DIMS)
def test_loss_terms_and_per_occurrence_gradients(dev, d, pop):
    """All B (1, TPB - 1, TPB + 1, 3 TPB + 5; d = 64 also 2048), all kinds: the three loss terms and the three per-occurrence gradients; the tables
    are bit-unchanged."""
    from pda_amd import ops
    w = Worst("UPD_NONE d=%d pop=%d" % (d, pop))
    for B, kind in cases_of(d, tr.KINDS):
        c, ref, bnd = tr.shared(d, B, kind, pop)
        Ut, It, ut, pt, nt, ppt, pnt = dev_case(dev, c, pop)
        g = grads_out(dev, B, d)
        loss = torch.zeros(3, device=dev)
        ops.bpr_step(Ut, It, ut, pt, nt, ppt, pnt, regs=c.regs, reg_div=c.reg_div, mode=ops.UPD_NONE, grads_out=g, loss_acc=loss)
        where = "B=%d %s" % (B, kind)
        w.check("loss", loss, ref["loss"], bnd["loss"], where)
        for q, t in zip(("due", "dpe", "dne"), g):
            w.check(q, t, ref[q], bnd[q], where)
        assert torch.equal(Ut.cpu(), torch.from_numpy(c.U)) and torch.equal(It.cpu(), torch.from_numpy(c.I)), where
    w.report()


# ---- ops.bpr_step(mode=UPD_DENSE_GRAD) and ops.adam_step ---------------------------------------------------------------------------------------
def _adam_tables(dev, c):
    Ut, It = to(dev, c.U, c.I)
    st = {k: torch.zeros_like(t) for k, t in (("mU", Ut), ("vU", Ut), ("gU", Ut), ("mI", It), ("vI", It), ("gI", It))}
    return Ut, It, st


def _check_first_adam_step(w, c, ref, bnd, st, tagU, tagI, where):
    """The tags are exactly the batch's distinct rows; the four moment tables lie within their propagated bound on the batch's rows and are
    exactly 0 on idle rows (the bound is 0 there, and check() allows no error where it is)."""
    occ_u, occ_i = tr.occurrences(c)
    np.testing.assert_array_equal(tagU.cpu().numpy(), np.where(occ_u > 0, 1, 0), err_msg=where)
    np.testing.assert_array_equal(tagI.cpu().numpy(), np.where(occ_i > 0, 1, 0), err_msg=where)
    for q, occ in (("mU", occ_u), ("vU", occ_u), ("mI", occ_i), ("vI", occ_i)):
        w.check(q, st[q], ref[q], bnd[q], where)
        assert not st[q].cpu().numpy()[occ == 0].any(), (q, where, "idle rows are exactly 0")
        assert not bnd[q][occ == 0].any()
    assert float(st["gU"].abs().max()) == 0.0 and float(st["gI"].abs().max()) == 0.0, "the sweep clears the accumulators"


@pytest.mark.parametrize("pop", [False, True])
@pytest.mark.parametrize("d", tr.DIMS)
def test_summed_gradients_and_the_first_adam_step(dev, d, pop):
    """`hot` and `spread`: gU / gI of the ungrouped step and of the grouped one on the batch stably sorted by positive; through ops.adam_step (both
    variants, and users_distinct on a distinct-user batch) the tags and the moments after the first step from zero moments."""
    from pda_amd import ops
    w = Worst("UPD_DENSE_GRAD / adam_step d=%d pop=%d" % (d, pop))
    lr_t = ops.adam_lr_t(1e-2, 1)
    for B, kind in cases_of(d, ("hot", "spread")):
        for variant in ("any_order", "grouped", "users_distinct"):
            c, ref, bnd = tr.shared(d, B, kind, pop, distinct_users=True) if variant == "users_distinct" else tr.shared(d, B, kind, pop)
            if variant == "grouped":
                c = c.take(np.argsort(c.pos, kind="stable"))       # (the sums are those of the same reference)
                assert (np.diff(c.pos) >= 0).all()
            where = "B=%d %s %s" % (B, kind, variant)
            kw = dict(regs=c.regs, reg_div=c.reg_div)
            if variant != "users_distinct":
                Ut, It, ut, pt, nt, ppt, pnt = dev_case(dev, c, pop)
                gU, gI = torch.zeros_like(Ut), torch.zeros_like(It)
                loss = torch.zeros(3, device=dev)
                ops.bpr_step(Ut, It, ut, pt, nt, ppt, pnt, mode=ops.UPD_DENSE_GRAD, gU=gU, gI=gI, loss_acc=loss, grouped=variant == "grouped", **kw)
                w.check("loss", loss, ref["loss"], bnd["loss"], where)
                w.check("gU", gU, ref["gU"], bnd["gU"], where)
                w.check("gI", gI, ref["gI"], bnd["gI"], where)
                assert torch.equal(Ut.cpu(), torch.from_numpy(c.U)) and torch.equal(It.cpu(), torch.from_numpy(c.I)), where
            Ut, It, st = _adam_tables(dev, c)
            _, _, ut, pt, nt, ppt, pnt = dev_case(dev, c, pop)
            tagU, tagI = ops.adam_row_tags(c.U.shape[0], c.I.shape[0], dev)
            loss = torch.zeros(3, device=dev)
            ops.adam_step(Ut, st["mU"], st["vU"], st["gU"], tagU, It, st["mI"], st["vI"], st["gI"], tagI, ut, pt, nt, ppt, pnt, step=1, lr_t=lr_t,
                          grouped=variant == "grouped", users_distinct=variant == "users_distinct", loss_acc=loss, **kw)
            w.check("loss", loss, ref["loss"], bnd["loss"], where)
            _check_first_adam_step(w, c, ref, bnd, st, tagU, tagI, where)
    w.report()


# ---- ops.bpr_step(mode=UPD_SGD_FUSED) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lr", LRS)
@pytest.mark.parametrize("d", tr.DIMS)
def test_fused_sgd_step_on_unshared_rows(dev, d, lr):
    """`unshared` only: no row is read while another triplet writes it, so the one-launch step is the exact step there.  Both heads, with and
    without users_distinct."""
    from pda_amd import ops
    w = Worst("UPD_SGD_FUSED d=%d lr=%g" % (d, lr))
    for B, kind in cases_of(d, ("unshared",)):
        for pop in (False, True):
            c, ref, bnd = tr.shared(d, B, kind, pop, lr)
            for distinct in (False, True):
                Ut, It, ut, pt, nt, ppt, pnt = dev_case(dev, c, pop)
                loss = torch.zeros(3, device=dev)
                ops.bpr_step(Ut, It, ut, pt, nt, ppt, pnt, regs=c.regs, reg_div=c.reg_div, lr=lr, mode=ops.UPD_SGD_FUSED, loss_acc=loss,
                             users_distinct=distinct)
                where = "B=%d pop=%d users_distinct=%d" % (B, pop, distinct)
                w.check("loss", loss, ref["loss"], bnd["loss"], where)
                w.check("U_sgd", Ut, ref["U_sgd"], bnd["U_sgd"], where)
                w.check("I_sgd", It, ref["I_sgd"], bnd["I_sgd"], where)
    w.report()


# ---- ops.sgd_step_exact and ops.bpr_step_plan ---------------------------------------------------------------------------------------------------
def _untouched_rows_identical(c, Ut, It, where):
    occ_u, occ_i = tr.occurrences(c)
    assert np.array_equal(Ut.cpu().numpy()[occ_u == 0], c.U[occ_u == 0]) and np.array_equal(It.cpu().numpy()[occ_i == 0], c.I[occ_i == 0]), where


@pytest.mark.parametrize("lr", LRS)
@pytest.mark.parametrize("d", tr.DIMS)
def test_exact_sgd_steps_on_a_hot_batch(dev, d, lr):
    """`hot`: the two-launch exact step (repeated users) and the planned step (distinct users, as its contract says): tables within bound,
    untouched rows bit-identical."""
    from pda_amd import ops
    w = Worst("sgd_step_exact / bpr_step_plan d=%d lr=%g" % (d, lr))
    for B, kind in cases_of(d, ("hot",)):
        for pop in (False, True):
            for path in ("sgd_step_exact", "bpr_step_plan"):
                c, ref, bnd = tr.shared(d, B, kind, pop, lr, distinct_users=True) if path == "bpr_step_plan" else tr.shared(d, B, kind, pop, lr)
                Ut, It, ut, pt, nt, ppt, pnt = dev_case(dev, c, pop)
                loss = torch.zeros(3, device=dev)
                kw = dict(regs=c.regs, reg_div=c.reg_div, lr=lr, loss_acc=loss)
                if path == "sgd_step_exact":
                    ops.sgd_step_exact(Ut, It, ut, pt, nt, ppt, pnt, **kw)
                else:
                    plan = ops.triplet_plan(ut, pt, nt)[0]
                    assert ops.plan_header(plan)[1] == 0
                    ops.bpr_step_plan(Ut, It, ut, pt, nt, ppt, pnt, plan=plan, **kw)
                where = "B=%d pop=%d %s" % (B, pop, path)
                w.check("loss", loss, ref["loss"], bnd["loss"], where)
                w.check("U_sgd", Ut, ref["U_sgd"], bnd["U_sgd"], where)
                w.check("I_sgd", It, ref["I_sgd"], bnd["I_sgd"], where)
                _untouched_rows_identical(c, Ut, It, where)
    w.report()


# ---- ops.bpr_grad_plan -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pop", [False, True])
@pytest.mark.parametrize("d", tr.DIMS)
def test_planned_gradient(dev, d, pop):
    """`hot` and `spread`, both with distinct users (a planned batch with a repeated user is rejected)."""
    from pda_amd import ops
    w = Worst("bpr_grad_plan d=%d pop=%d" % (d, pop))
    for B, kind in cases_of(d, ("hot", "spread")):
        c, ref, bnd = tr.shared(d, B, kind, pop, distinct_users=True)
        Ut, It, ut, pt, nt, ppt, pnt = dev_case(dev, c, pop)
        gU, gI = torch.zeros_like(Ut), torch.zeros_like(It)
        loss = torch.zeros(3, device=dev)
        plan = ops.triplet_plan(ut, pt, nt)[0]
        ops.bpr_grad_plan(Ut, It, ut, pt, nt, ppt, pnt, regs=c.regs, reg_div=c.reg_div, plan=plan, gU=gU, gI=gI, loss_acc=loss)
        where = "B=%d %s" % (B, kind)
        w.check("loss", loss, ref["loss"], bnd["loss"], where)
        w.check("gU", gU, ref["gU"], bnd["gU"], where)
        w.check("gI", gI, ref["gI"], bnd["gI"], where)
    w.report()


# ---- ops.bpr_step_bf16 -----------------------------------------------------------------------------------------------------------------------------
def _bf16_case(dev, d, B, kind):
    """The case with its tables as fp32 masters; the forward pass reads their bf16 roundings, so reference and bound are taken on the widened
    bf16 tables, the update on the masters."""
    m = tr.case(d, B, kind)
    Ub, Ib = (torch.from_numpy(x).to(dev).bfloat16() for x in (m.U, m.I))
    return m.with_tables(Ub.float().cpu().numpy(), Ib.float().cpu().numpy(), Um=m.U, Im=m.I), Ub, Ib


@pytest.mark.parametrize("d", tr.DIMS)
def test_bf16_tables_step(dev, d):
    """The per-occurrence gradients on `spread` and `unshared`; on `unshared` the fp32 masters after a fused step, and the touched bf16 rows equal
    to the RNE of the masters bit for bit."""
    from pda_amd import ops
    lr = 0.05
    w = Worst("bpr_step_bf16 d=%d" % d)
    for B, kind in cases_of(d, ("spread", "unshared")):
        c, Ub, Ib = _bf16_case(dev, d, B, kind)
        for pop in (False, True):
            ref, bnd = tr.reference(c, pop, lr), tr.bound(c, pop, lr)
            _, _, ut, pt, nt, ppt, pnt = dev_case(dev, c, pop)
            where = "B=%d %s pop=%d" % (B, kind, pop)
            g = grads_out(dev, B, d)
            loss = torch.zeros(3, device=dev)
            ops.bpr_step_bf16(Ub, Ib, ut, pt, nt, ppt, pnt, regs=c.regs, reg_div=c.reg_div, mode=ops.UPD_NONE, grads_out=g, loss_acc=loss)
            w.check("loss", loss, ref["loss"], bnd["loss"], where)
            for q, t in zip(("due", "dpe", "dne"), g):
                w.check(q, t, ref[q], bnd[q], where)
            if kind != "unshared":
                continue
            Um, Im = to(dev, c.Um, c.Im)
            Ub1, Ib1 = Ub.clone(), Ib.clone()
            loss.zero_()
            ops.bpr_step_bf16(Ub1, Ib1, ut, pt, nt, ppt, pnt, regs=c.regs, reg_div=c.reg_div, lr=lr, mode=ops.UPD_SGD_FUSED, U_master=Um, I_master=Im,
                              loss_acc=loss)
            w.check("loss", loss, ref["loss"], bnd["loss"], where)
            w.check("U_sgd", Um, ref["U_sgd"], bnd["U_sgd"], where)
            w.check("I_sgd", Im, ref["I_sgd"], bnd["I_sgd"], where)
            occ_u, occ_i = (torch.from_numpy(o > 0) for o in tr.occurrences(c))
            Ub1, Ib1, Um, Im = Ub1.cpu(), Ib1.cpu(), Um.cpu(), Im.cpu()
            assert torch.equal(Ub1[occ_u], Um[occ_u].bfloat16()) and torch.equal(Ib1[occ_i], Im[occ_i].bfloat16()), where
            assert torch.equal(Ub1[~occ_u], Ub.cpu()[~occ_u]) and torch.equal(Ib1[~occ_i], Ib.cpu()[~occ_i]), where
    w.report()


# ---- ops.bpr_step_shard and ops.apply_user_grads -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pop", [False, True])
@pytest.mark.parametrize("d", tr.DIMS)
def test_item_shards_equal_the_one_table_step(dev, d, pop):
    """A batch split over two item shards (the second with item_offset > 0): the shards' loss shares, user gradients and item rows together are
    the one-table reference.  The gradient mode (gI_shard) on `hot`; the SGD mode, which moves the shard's rows inside the launch, on `unshared`."""
    from pda_amd import ops
    lr = 0.05
    w = Worst("bpr_step_shard d=%d pop=%d" % (d, pop))
    for B in tr.batches(d)[2:]:
        for kind in ("hot", "unshared"):
            c, ref, bnd = tr.shared(d, B, kind, pop, lr, shards=2)
            per = c.I.shape[0] // 2
            Ut, It, ut, pt, nt, ppt, pnt = dev_case(dev, c, pop)
            shards = [It[:per].clone(), It[per:].clone()]
            g_sh = [torch.zeros_like(s) for s in shards]
            g_user = torch.zeros(B, d, device=dev)
            loss = torch.zeros(3, device=dev)
            cut = int(np.searchsorted(c.pos >= per, True))
            assert 0 < cut < B and (c.neg[:cut] < per).all() and (c.neg[cut:] >= per).all() and (c.pos[cut:] >= per).all()
            for s, sl in enumerate((slice(0, cut), slice(cut, B))):
                ops.bpr_step_shard(Ut, shards[s], s * per, ut[sl], pt[sl], nt[sl], None if ppt is None else ppt[sl], None if pnt is None else pnt[sl],
                                   regs=c.regs, reg_div=c.reg_div, mean_div=B, lr=lr, g_user=g_user[sl], loss_acc=loss,
                                   gI_shard=g_sh[s] if kind == "hot" else None)
            where = "B=%d %s" % (B, kind)
            assert torch.equal(Ut.cpu(), torch.from_numpy(c.U)), "U waits for the exchange"
            w.check("loss", loss, ref["loss"], bnd["loss"], where)
            w.check("due", g_user, ref["due"], bnd["due"], where)
            if kind == "hot":
                w.check("gI", torch.cat(g_sh), ref["gI"], bnd["gI"], where)
                assert torch.equal(torch.cat(shards).cpu(), torch.from_numpy(c.I))
            else:
                w.check("I_sgd", torch.cat(shards), ref["I_sgd"], bnd["I_sgd"], where)
            ops.apply_user_grads(Ut, ut, g_user, lr)
            w.check("U_sgd", Ut, ref["U_sgd"], bnd["U_sgd"], where)
    w.report()


# ---- saturated sigmoids ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pop", [False, True])
@pytest.mark.parametrize("d", tr.DIMS)
def test_saturated_sigmoids(dev, d, pop):
    """x = -30 (the + 1e-10 decides the gradient: the case that rejects a denominator without it), x = -100 (fp32 expf overflows: the loss term is
    -log(1e-10) / B, the gradient exactly the L2 term), x = +40 (1 - s vanishes), alone and among ordinary triplets, through UPD_NONE and
    UPD_DENSE_GRAD: every output finite and within bound."""
    from pda_amd import ops
    w = Worst("saturated d=%d pop=%d" % (d, pop))
    singles = [(tr.saturated_single(d, j), "single x=%g" % tr.SAT_X[j]) for j in range(3)]
    mixed = [(tr.shared(d, B, "saturated", pop)[0], "B=%d" % B) for B in tr.batches(d)[2:]]
    for c, where in singles + mixed:
        ref, bnd = tr.reference(c, pop), tr.bound(c, pop)
        B = c.B
        Ut, It, ut, pt, nt, ppt, pnt = dev_case(dev, c, pop)
        g = grads_out(dev, B, d)
        gU, gI = torch.zeros_like(Ut), torch.zeros_like(It)
        loss, loss2 = torch.zeros(3, device=dev), torch.zeros(3, device=dev)
        kw = dict(regs=c.regs, reg_div=c.reg_div)
        ops.bpr_step(Ut, It, ut, pt, nt, ppt, pnt, mode=ops.UPD_NONE, grads_out=g, loss_acc=loss, **kw)
        ops.bpr_step(Ut, It, ut, pt, nt, ppt, pnt, mode=ops.UPD_DENSE_GRAD, gU=gU, gI=gI, loss_acc=loss2, **kw)
        w.check("loss", loss, ref["loss"], bnd["loss"], where)
        w.check("loss", loss2, ref["loss"], bnd["loss"], where)
        for q, t in zip(("due", "dpe", "dne", "gU", "gI"), g + (gU, gI)):
            w.check(q, t, ref[q], bnd[q], where)                      # (finite, and the x = -30 triplet's gradient within bound)
        if len(c.sat) > 1 and c.sat[1] is not None:
            # the x = -100 triplet: d loss / dx is exactly 0, what is left is fl(c row) with c = fl(regs / reg_div)
            t = c.sat[1]
            cc = F(c.regs) / F(c.reg_div)
            for got, row in zip(g, (c.U[c.users[t]], c.I[c.pos[t]], c.I[c.neg[t]])):
                assert np.array_equal(got[t].cpu().numpy(), cc * row), where
            if B == 1:
                w.check("mf of x=-100", loss[1:2], np.array([-np.log(1e-10)]), bnd["loss"][1:2], where)
    w.report()
