"""GPU: the sampled-softmax loss (`--train ssm`, include/pda_hip_ssm.h) -- the gradient step against the float64 restatement of tests/ssm_ref.py
on its 24 cases (every d with every N, norm, tau, batch size, batch order and user rule), the skipped rows, a saturated batch, zero rows under
the normalisation, the BPR step at N = 1, the whole Adam step, graph replay, the sampler bit for bit, the row normalisation, the refusals, and
the CLI.

Tolerances (ssm_ref.tolerance): 1e-5 max(1, 1 / tau) absolute on every loss term and gradient element.  tests/test_ssm_host.py shows that the
restatement in float32 stays inside a quarter of it on the same inputs, and that a restatement with one clause of the contract broken does
not stay inside it.  1e-5 on tables and moments after three Adam steps."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from ssm_ref import (ADAM_STEPS, CASES, DIMS, NI, NU, REGS, TOL, adam_steps_case, adam_steps_reference, batch, parity_case, ssm_grads, ssm_sample,
                     tables, tolerance, tpb)

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = -1, -2


def to(dev, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


class State:
    """What ops.ssm_step / ops.ssm_adam_step write besides the tables."""

    def __init__(self, Ut, It):
        from pda_amd import ops
        z = torch.zeros_like
        self.mU, self.vU, self.gU, self.mI, self.vI, self.gI = z(Ut), z(Ut), z(Ut), z(It), z(It), z(It)
        self.tagU, self.tagI = ops.adam_row_tags(Ut.shape[0], It.shape[0], Ut.device)

    def adam(self, Ut, It):
        return (Ut, self.mU, self.vU, self.gU, self.tagU, It, self.mI, self.vI, self.gI, self.tagI)


def run_step(dev, U, I, b, *, tau, norm, reg_div, step=1, **kw):
    from pda_amd import ops
    Ut, It, ut, pt, nt = to(dev, U, I, *b)
    st = State(Ut, It)
    loss = torch.zeros(3, device=dev)
    ops.ssm_step(Ut, It, ut, pt, nt, st.gU, st.gI, st.tagU, st.tagI, tau=tau, norm=norm, regs=REGS, reg_div=reg_div, step=step, loss_acc=loss, **kw)
    return loss.cpu().numpy(), st.gU.cpu().numpy(), st.gI.cpu().numpy(), st


def check(got, ref, tol, what):
    loss, gU, gI = got
    terms, rU, rI = ref
    print("ssm %s: max |loss err| %.3g  max |gU err| %.3g  max |gI err| %.3g  (bound %.3g)" % (what, np.abs(loss - terms).max(), np.abs(gU - rU).max(),
                                                                                           np.abs(gI - rI).max(), tol))
    assert np.isfinite(loss).all() and np.isfinite(gU).all() and np.isfinite(gI).all()
    np.testing.assert_allclose(loss, terms, atol=tol, rtol=0)
    np.testing.assert_allclose(gU, rU, atol=tol, rtol=0)
    np.testing.assert_allclose(gI, rI, atol=tol, rtol=0)
    assert abs(loss[0] - (loss[1] + loss[2])) <= tol


def check_tags(st, b, tag):
    """Exactly the batch's distinct rows carry the tag, as pda_adam_step_f32 leaves them."""
    S_u, S_i = np.unique(b[0]), np.unique(np.concatenate([b[1], np.asarray(b[2]).ravel()]))
    tagU, tagI = st.tagU.cpu().numpy(), st.tagI.cpu().numpy()
    assert (np.nonzero(tagU)[0] == S_u).all() and (np.nonzero(tagI)[0] == S_i).all() and set(tagU[S_u]) == {tag} and set(tagI[S_i]) == {tag}


@functools.lru_cache(maxsize=None)
def reference(case):
    d, N, norm, tau, one_row, grouped, distinct = case
    U, I, b, B = parity_case(*case)
    return ssm_grads(U, I, *b, tau=tau, norm=norm, regs=REGS, reg_div=B)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "d%d-N%d-norm%d-tau%g-B%s-%s-%s" % (c[0], c[1], c[2], c[3], "1" if c[4] else "T+3",
                                                                                          "grouped" if c[5] else "any", "distinct" if c[6] else "rep"))
def test_gradients_and_loss_against_the_float64_restatement(dev, case):
    """24 cases: with every d, every N in {1, 2, 7, 64, 256}, both norms, both taus, B = 1 and B = TPB + 3 (a run of the hot positive crosses the
    workgroup boundary of the grouped batches, the last workgroup is partial), PDA_UPD_ANY_ORDER on a shuffled batch and the grouped rule on a
    sorted one, with and without PDA_UPD_USERS_DISTINCT."""
    d, N, norm, tau, one_row, grouped, distinct = case
    U, I, b, B = parity_case(*case)
    loss, gU, gI, st = run_step(dev, U, I, b, tau=tau, norm=norm, reg_div=B, step=5, grouped=grouped, users_distinct=distinct)
    check((loss, gU, gI), reference(case), tolerance(tau), "d=%d N=%d norm=%d tau=%g B=%d grouped=%d distinct=%d" % (d, N, norm, tau, B, grouped, distinct))
    check_tags(st, b, 5)


@pytest.mark.parametrize("d, norm", [(32, 0), (256, 1)])
def test_rows_with_an_id_outside_the_tables_are_skipped_whole(dev, d, norm):
    """The kernel's own id test (pda_ssm.hip: users, pos and all N negatives are compared with the table sizes before any row is gathered) skips a
    row with an out-of-range user, one with an out-of-range positive and one with a single out-of-range negative in column N - 1 -- inside the
    run of the hot positive, and across the workgroup boundary: the batch equals the remaining rows with the mean still over B, under either
    batch rule, and the tags are set on exactly the kept rows."""
    from pda_amd import ops
    N, tau = 7, 0.1
    T = tpb(d)
    B = T + 3
    rng = np.random.default_rng(11 * d)
    U, I = tables(rng, d)
    users, pos, negs = batch(rng, B, N, grouped=True)
    assert pos[T - 1] == pos[T] == NI - 1
    with pytest.raises(ValueError, match="outside the tables"):       # ops checks the ids when asked to
        bad = negs.copy()
        bad[0, N - 1] = NI
        Ut, It, ut, pt, nt = to(dev, U, I, users, pos, bad)
        st = State(Ut, It)
        ops.ssm_step(Ut, It, ut, pt, nt, st.gU, st.gI, st.tagU, st.tagI, tau=tau, norm=norm, regs=REGS, reg_div=B, step=1)
    assert float(st.gU.abs().max()) == 0.0 and int(st.tagI.abs().max()) == 0            # nothing was launched
    users[1], pos[2], negs[T, N - 1], negs[B - 2, N - 1] = -1, NI, NI, -7
    keep = ~np.isin(np.arange(B), [1, 2, T, B - 2])
    kept = [x[keep] for x in (users, pos, negs)]
    ref = ssm_grads(U, I, *kept, tau=tau, norm=norm, regs=REGS, reg_div=B, B=B)
    for grouped in (False, True):
        loss, gU, gI, st = run_step(dev, U, I, (users, pos, negs), tau=tau, norm=norm, reg_div=B, step=3, grouped=grouped, check_ids=False)
        check((loss, gU, gI), ref, tolerance(tau), "four rows skipped d=%d norm=%d grouped=%d" % (d, norm, grouped))
        check_tags(st, kept, 3)
    users[:], pos[0] = NU, 0                                            # every row skipped: nothing moves
    loss, gU, gI, st = run_step(dev, U, I, (users, pos, negs), tau=tau, norm=norm, reg_div=B, check_ids=False)
    assert np.abs(loss).max() == 0.0 and np.abs(gU).max() == 0.0 and np.abs(gI).max() == 0.0 and int(st.tagU.abs().max()) == 0 == int(st.tagI.abs().max())


@pytest.mark.parametrize("d", [32, 128])
def test_a_saturated_batch_stays_finite_and_keeps_its_loss(dev, d):
    """tau = 0.1, norm = 0, hand-built rows on one axis (so that every logit is exact in float32): u = 8 e_0, items +10 e_0, -10 e_0 and 0 give the
    logits +800, -800 and 0 = +-80 / tau.  Row 0: the positive at +800 against -800 and zeros (loss 0); row 1: the positive at -800 against +800
    (loss 1 600: exp overflows without the max subtraction, and underflows with it); row 2: all four logits +800 (loss log 4); row 3: all
    four logits 0 (a user orthogonal to the items).  The gU comparison implies sum_k p_k = 1."""
    tau, N, B = 0.1, 3, 4
    U, I = np.zeros((NU, d), np.float32), np.zeros((NI, d), np.float32)
    U[0, 0], U[1, 1] = 8.0, 8.0
    I[0, 0], I[1, 0] = 10.0, -10.0                                      # item 2: the zero row
    users = np.array([0, 0, 0, 1], np.int32)
    pos = np.array([0, 1, 0, 0], np.int32)
    negs = np.array([[1, 2, 2], [0, 2, 2], [0, 0, 0], [1, 2, 0]], np.int32)
    ref = ssm_grads(U, I, users, pos, negs, tau=tau, norm=0, regs=REGS, reg_div=B)
    assert abs(ref[0][1] - (0.0 + 1600.0 + 2 * np.log(4.0)) / 4) < 1e-9
    for grouped in (False, True):
        loss, gU, gI, _ = run_step(dev, U, I, (users, pos, negs), tau=tau, norm=0, reg_div=B, grouped=grouped)
        check((loss, gU, gI), ref, tolerance(tau), "saturated d=%d grouped=%d" % (d, grouped))


@pytest.mark.parametrize("d", DIMS)
def test_zero_rows_under_the_normalisation_give_finite_numbers(dev, d):
    rng = np.random.default_rng(d)
    U, I = tables(rng, d)
    U[3], I[5], I[6] = 0.0, 0.0, 1e-30                                 # |x| below 1e-12: the derivative of x / 1e-12
    users = np.array([3, 3, 4, 3], np.int32)
    pos = np.array([5, 7, 5, 6], np.int32)
    negs = np.array([[5, 8, 6], [5, 5, 9], [6, 5, 5], [5, 6, 6]], np.int32)
    for tau in (1.0, 0.1):
        loss, gU, gI, _ = run_step(dev, U, I, (users, pos, negs), tau=tau, norm=1, reg_div=4)
        assert np.isfinite(loss).all() and np.isfinite(gU).all() and np.isfinite(gI).all() and loss[1] > 0


@pytest.mark.parametrize("d", DIMS)
def test_one_negative_at_tau_one_is_the_dense_gradient_bpr_step(dev, d):
    """N = 1, tau = 1, norm = 0, |x| <= 10: gU and gI of pda_bpr_step_f32(PDA_UPD_DENSE_GRAD) on the same triplets within 1e-5 -- a kernel the
    project already trusts (the 1e-10 inside BPR's log is far below that)."""
    from pda_amd import ops
    B = tpb(d) + 3
    rng = np.random.default_rng(3 * d)
    U, I = tables(rng, d)
    users, pos, negs = batch(rng, B, 1)
    x = np.einsum("bd,bd->b", U[users], I[pos]) - np.einsum("bd,bd->b", U[users], I[negs[:, 0]])
    assert np.abs(x).max() <= 10
    loss, gU, gI, _ = run_step(dev, U, I, (users, pos, negs), tau=1.0, norm=0, reg_div=B)
    Ut, It, ut, pt, nt = to(dev, U, I, users, pos, negs[:, 0])
    hU, hI, hl = torch.zeros_like(Ut), torch.zeros_like(It), torch.zeros(3, device=dev)
    ops.bpr_step(Ut, It, ut, pt, nt, regs=REGS, reg_div=B, mode=ops.UPD_DENSE_GRAD, gU=hU, gI=hI, loss_acc=hl)
    check((loss, gU, gI), (hl.cpu().numpy(), hU.cpu().numpy(), hI.cpu().numpy()), TOL, "N = 1 against pda_bpr_step_f32, d=%d" % d)


@functools.lru_cache(maxsize=None)
def adam_reference(norm):
    return adam_steps_reference(norm)


@pytest.mark.parametrize("policy", [1, 2], ids=["resident", "stream"])
@pytest.mark.parametrize("norm", [0, 1])
def test_three_whole_steps_against_the_restatement(dev, norm, policy):
    """ssm_ref.ADAM_STEPS says why these steps run at the trainer's default learning rate."""
    from pda_amd import ops
    c = ADAM_STEPS
    U, I, batches = adam_steps_case()
    ref, terms = adam_reference(norm)
    Ut, It = to(dev, U, I)
    st = State(Ut, It)
    for t, b in enumerate(batches, 1):
        loss = torch.zeros(3, device=dev)
        ops.ssm_adam_step(*st.adam(Ut, It), *to(dev, *b), tau=c["tau"], norm=norm, regs=REGS, reg_div=c["B"], step=t,
                          lr_t=ops.adam_lr_t(c["lr"], t), cache_policy=policy, loss_acc=loss, check_ids=True)
        np.testing.assert_allclose(loss.cpu().numpy(), terms[t - 1], atol=tolerance(c["tau"]), rtol=0)
        # g is zero again and the tags are consumed: the batch's rows carry this step's tag, and a sweep under the NEXT tag would read no g
        assert float(st.gU.abs().max()) == 0.0 and float(st.gI.abs().max()) == 0.0
        tagI = st.tagI.cpu().numpy()
        assert set(tagI[np.unique(np.concatenate([b[1], b[2].ravel()]))]) == {t} and tagI.max() == t
    got = dict(U=Ut, I=It, mU=st.mU, vU=st.vU, mI=st.mI, vI=st.vI)
    for k in got:
        print("ssm three steps (norm=%d policy=%d): max |%s err| %.3g" % (norm, policy, k, np.abs(got[k].cpu().numpy() - ref[k]).max()))
    for k in got:
        np.testing.assert_allclose(got[k].cpu().numpy(), ref[k], atol=TOL, rtol=0, err_msg=k)


@pytest.mark.parametrize("norm", [0, 1])
def test_the_step_replays_from_a_captured_graph(dev, norm):
    """pda_ssm_adam_step_f32 reads nothing back on the host: two steps (tags 1 and 2) captured once on one stream and replayed give the tables
    of the same two steps launched directly."""
    from pda_amd import ops
    d, B, N = 64, 200, 16
    rng = np.random.default_rng(5)
    U, I = tables(rng, d)
    bt = to(dev, *batch(rng, B, N))

    def two_steps(Ut, It, st, loss):
        for t in (1, 2):
            ops.ssm_adam_step(*st.adam(Ut, It), *bt, tau=0.1, norm=norm, regs=REGS, reg_div=B, step=t, lr_t=ops.adam_lr_t(1e-2, t), loss_acc=loss)
    Ua, Ia = to(dev, U, I)
    sa, la = State(Ua, Ia), torch.zeros(3, device=dev)
    two_steps(Ua, Ia, sa, la)
    Ub, Ib = to(dev, U, I)
    sb, lb = State(Ub, Ib), torch.zeros(3, device=dev)
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


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------------------
def toy_csr(n_users, n_items, seed, max_len):
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.permutation(n_items)[:rng.integers(0, max_len + 1)]) for _ in range(n_users)]
    indptr = np.zeros(n_users + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.concatenate(rows).astype(np.int32)


@pytest.mark.parametrize("N", [1, 5, 256])
def test_the_sampler_equals_its_restatement_bit_for_bit(dev, N):
    """pda_ssm_sample and pda_ssm_sample_dev against tests/ssm_ref.ssm_sample: users drawn by the kernel from a pool larger than B (distinct) and
    smaller than B (with replacement) and users given, the whole catalogue and a narrowed neg_lo / neg_hi; column 0 is pda_sample_triplets on the
    device for the same seed and step; step_next is written."""
    from pda_amd import ops
    n_users, n_items = 60, 80
    indptr, indices = toy_csr(n_users, n_items, 5, 30)
    ip, ix = to(dev, indptr, indices)
    pool = np.random.default_rng(2).permutation(n_users)[:40].astype(np.int32)
    pt = to(dev, pool)[0]
    given = np.random.default_rng(3).integers(0, n_users, 24).astype(np.int32)
    seed = 0x9E3779B97F4A7C15
    for B, users, rng_ in ((24, None, (0, n_items)), (64, None, (10, 50)), (24, given, (0, n_items))):
        step = 7 + B
        ref = ssm_sample(seed, step, B, N, indptr, indices, user_pool=pool, n_pool=len(pool), users=users, neg_range=rng_)
        ut = None if users is None else to(dev, users)[0]
        u, p, n = ops.ssm_sample(ip, ix, B, N, seed=seed, step=step, neg_range=rng_, users=ut, user_pool=pt, n_pool=len(pool))
        np.testing.assert_array_equal(u.cpu().numpy(), ref["users"])
        np.testing.assert_array_equal(p.cpu().numpy(), ref["pos"])
        np.testing.assert_array_equal(n.cpu().numpy(), ref["negs"])
        assert n.shape == (B, N) and n.dtype == torch.int32
        if users is None:
            assert (len(np.unique(ref["users"])) == B) == (B <= len(pool))
        tu, tp, tn, _, _ = ops.sample_triplets(ip, ix, B, seed=seed, step=step, users=None if ut is None else ut.clone(), user_pool=pt,
                                               n_pool=len(pool), neg_range=rng_)
        assert torch.equal(tu, u) and torch.equal(tp, p) and torch.equal(tn, n[:, 0])
        if users is None:       # the _dev form: the step from device memory, step + 1 into the other slot
            out = (torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev),
                   torch.zeros((B, N), dtype=torch.int32, device=dev))
            ctr = torch.tensor([step, -1], dtype=torch.int64, device=dev)
            ops.ssm_sample_into(out, ip, ix, seed=seed, step_dev=ctr, neg_range=rng_, parity=0, user_pool=pt, n_pool=len(pool))
            assert torch.equal(out[0], u) and torch.equal(out[1], p) and torch.equal(out[2], n) and ctr.tolist() == [step, step + 1]
            ops.ssm_sample_into(out, ip, ix, seed=seed, step_dev=ctr, neg_range=rng_, parity=1, user_pool=pt, n_pool=len(pool))
            nxt = ssm_sample(seed, step + 1, B, N, indptr, indices, user_pool=pool, n_pool=len(pool), neg_range=rng_)
            np.testing.assert_array_equal(out[2].cpu().numpy(), nxt["negs"])
            assert ctr.tolist() == [step + 2, step + 1]
            ops.ssm_sample_into(out, ip, ix, seed=seed, step_dev=ctr[1:], neg_range=rng_, user_pool=pt, n_pool=len(pool))      # read only
            np.testing.assert_array_equal(out[2].cpu().numpy(), nxt["negs"])
            assert ctr.tolist() == [step + 2, step + 1]


def test_the_device_sampler_hands_out_the_stream_of_the_restatement(dev, tmp_path):
    """DeviceSampler(mode="ssm"): batches 1, 2, .. of ops.ssm_sample, across a refill of its queue, and refused with a plan."""
    from pda_amd import load_data, parse, sampler, synthetic
    synthetic.write_dataset(str(tmp_path / "data" / "toy"), n_users=200, n_items=150, mean_hist=12)
    args = parse.parse_args(["--data_path", str(tmp_path / "data") + "/", "--dataset", "toy", "--batch_size", "64"])
    data = load_data.Data(args)
    s = sampler.DeviceSampler(data, dev, False, mode="ssm", n_negs=5, ahead=3)
    indptr, indices, _ = (t.numpy() for t in data.train_csr("cpu"))
    pool = np.fromiter(data.train_user_list.keys(), dtype=np.int32)
    for step in range(1, 8):
        u, p, n = (t.cpu().numpy() for t in s.batch())
        ref = ssm_sample(2020, step, 64, 5, indptr, indices, user_pool=pool, n_pool=len(pool), neg_range=(0, data.n_items))
        np.testing.assert_array_equal(u, ref["users"])
        np.testing.assert_array_equal(p, ref["pos"])
        np.testing.assert_array_equal(n, ref["negs"])
    s.with_plan = True
    with pytest.raises(ValueError, match="with_plan"):
        s.batch()


# ---- the row normalisation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
def test_normalised_rows_are_within_two_ulp_and_keep_their_bits(dev, d):
    from pda_amd import ops
    rng = np.random.default_rng(d)
    n = 531                                                            # not a multiple of the rows of a workgroup
    X = rng.standard_normal((n, d))
    X *= (10.0 ** rng.uniform(-20, 3, n) / np.sqrt((X ** 2).sum(1)))[:, None]       # row norms 1e-20 .. 1e3
    X = X.astype(np.float32)
    X[17] = 0.0
    Xt = to(dev, X)[0]
    Y, Y2 = ops.ssm_normalize_rows(Xt), ops.ssm_normalize_rows(Xt)
    assert torch.equal(Y.view(torch.int32), Y2.view(torch.int32))
    x64 = X.astype(np.float64)
    want = x64 / np.maximum(np.sqrt((x64 ** 2).sum(1)), 1e-12)[:, None]
    got = Y.cpu().numpy()
    ulp = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print("ssm normalise d=%d: worst %.3g ulp" % (d, ulp.max()))
    assert ulp.max() <= 2.0 and np.abs(got[17]).max() == 0.0
    nrm = np.sqrt((got.astype(np.float64) ** 2).sum(1))
    big = np.sqrt((x64 ** 2).sum(1)) >= 1e-12
    assert big.sum() > 100 and (~big).sum() > 100 and np.abs(nrm[big] - 1).max() < 1e-6 and nrm[~big].max() < 1.0
    ops.ssm_normalize_rows(Xt, out=Xt)                                 # in place
    assert torch.equal(Xt, Y)


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_refuse_before_they_launch(dev):
    from pda_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(1)
    U, I = tables(rng, 32)
    b = batch(rng, 9, 4)
    Ut, It, ut, pt, nt = to(dev, U, I, *b)
    st = State(Ut, It)
    p, null = _lib.ptr, C.c_void_p(None)

    def step(U=p(Ut), negs=p(nt), gI=p(st.gI), N=4, d=32, tau=0.1, norm=1):
        return lib.pda_ssm_step_f32(U, p(It), NU, NI, p(ut), p(pt), negs, 9, N, d, tau, norm, REGS, 9.0, p(st.gU), gI, p(st.tagU), p(st.tagI), 1, 0x100,
                                    null, _lib.stream_ptr())

    assert step(N=0) == ERR_ARG and step(N=257) == ERR_ARG and step(tau=0.0) == ERR_ARG and step(tau=float("nan")) == ERR_ARG and step(norm=2) == ERR_ARG
    assert step(d=48) == ERR_UNSUPPORTED and step(U=null) == ERR_ARG and step(negs=null) == ERR_ARG and step(gI=null) == ERR_ARG
    torch.cuda.synchronize()
    assert float(st.gU.abs().max()) == 0.0 and float(st.gI.abs().max()) == 0.0 and int(st.tagU.abs().max()) == 0 == int(st.tagI.abs().max())
    assert step() == 0                                                 # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert float(st.gU.abs().max()) > 0.0


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [0, 1])
def test_cli_trains_ssm_and_export_topk_ranks_by_the_tables_the_loss_trained(dev, tmp_path, norm):
    """python -m pda_amd.train_new_api --train ssm --test normal --ssm_negs 8 --epoch 3 --bias_report 1 in a child process on the smallest
    synthetic dataset: it ends, prints the metrics line and its bias lines, the loss of epoch 3 is below that of epoch 1, the checkpoint holds the
    RAW tables and the flags, and export_topk restores it into a fresh model whose lists are the top-K of U I^T (--ssm_norm 1: of the
    row-normalised tables) with the history masked, computed here with torch.topk in float64.
    Ties: no two items share a score to the last bit (every item row keeps its own Xavier draw or its own gradient history), and where two
    reference scores of a user's first K + 1 lie within 1e-5 of each other -- closer than the float32 scores can be trusted to order -- the
    user's list is compared by value only; the test asks that at least three users in four are compared item for item."""
    from pda_amd import ops, synthetic
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    synthetic.write_dataset(str(tmp_path / "data" / "toy"), n_users=200, n_items=150, mean_hist=12)
    argv = ["--data_path", str(tmp_path / "data") + "/", "--dataset", "toy", "--train", "ssm", "--test", "normal", "--epoch", "3", "--embed_size", "32",
            "--log_interval", "1", "--batch_size", "128", "--lr", "1e-2", "--regs", "1e-3", "--valid_set", "valid", "--pop_exp", "0.22",
            "--save_dir", str(tmp_path / "ckpt") + "/", "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t", "--cuda", "0", "--eval_block", "128",
            "--ssm_negs", "8", "--ssm_norm", str(norm), "--bias_report", "1", "--bias_groups", "4"]
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "pda_amd.train_new_api"] + argv, cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert "running SSM" in out and "recall=[" in out and "||--- bias@" in out and "best expo" in out and "training and testing end!!!!" in out
    losses = [float(m.group(1)) for m in re.finditer(r"Epoch \d+ \[[^\]]*\]: train==\[([-\d.]+)=[-\d.]+ \+ [-\d.]+\]", out)]
    assert len(losses) == 3 and losses[2] < losses[0] and np.isfinite(losses).all(), losses
    best = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path / "ckpt") for f in fs if f == "best_ckpt.ckpt"]
    assert len(best) == 1 and "ssm_train_ssm" in best[0]
    sd = torch.load(best[0], map_location="cpu")
    assert sd["format"] == "pda_amd/2" and sd["embed_size"] == 32 and sd["user_embedding"].shape == (200, 32) and "mU" in sd
    assert (sd["ssm_negs"], sd["ssm_tau"], sd["ssm_norm"]) == (8, 0.1, norm)
    assert float((sd["item_embedding"].double().norm(dim=1) - 1).abs().min()) > 1e-3           # the raw tables, not the normalised ones
    from pda_amd import export_topk
    from pda_amd import train_new_api as t
    res = export_topk.main(argv + ["--export_out", str(tmp_path / "lists.npz")])
    K = 50
    assert res["idx"].shape == (len(res["users"]), K) and len(res["users"]) > 0 and np.isfinite(res["val"]).all()
    # a second fresh model restored from the same file ranks identically
    res2 = export_topk.main(argv + ["--export_out", str(tmp_path / "lists2.npz")])
    np.testing.assert_array_equal(res["idx"], res2["idx"])
    np.testing.assert_array_equal(res["val"], res2["val"])
    U, I = sd["user_embedding"].to(dev), sd["item_embedding"].to(dev)
    if norm:
        U, I = ops.ssm_normalize_rows(U.contiguous()), ops.ssm_normalize_rows(I.contiguous())
    S = (U.double()[torch.from_numpy(res["users"]).long().to(dev)] @ I.double().T).cpu()
    for row, u in enumerate(res["users"]):
        S[row, torch.as_tensor(list(t.data.train_user_list.get(int(u), [])), dtype=torch.long)] = -np.inf
    val, idx = torch.topk(S, K + 1, dim=1)
    np.testing.assert_allclose(res["val"], val[:, :K].numpy(), atol=2e-6, rtol=0)
    gapped = ((val[:, :-1] - val[:, 1:]).min(dim=1).values > 1e-5).numpy()
    assert gapped.mean() >= 0.75, gapped.mean()
    np.testing.assert_array_equal(res["idx"][gapped], idx[:, :K].numpy()[gapped])
    if norm:
        assert np.abs(res["val"]).max() <= 1.0 + 1e-6                  # cosines
