"""GPU: the in-batch softmax with logQ correction (`--train ssm --ssm_source batch`, include/pda_hip_inbatch.h) -- the gradient step against the
float64 restatement of tests/inbatch_ref.py on its 24 cases (every d with every batch size, norm, tau, logq, mask, batch order and user rule),
whole column tiles excluded, skipped ids, a saturated batch, zero rows, the sampled-softmax kernel fed the same negatives, the train mask bit
for bit, the whole Adam step, graph replay, the operating point, and the CLI.

Tolerance (ssm_ref.tolerance): 1e-5 max(1, 1 / tau) absolute on every loss term and gradient element.  tests/test_inbatch_host.py shows that
the restatement in float32 stays inside a quarter of it on the same inputs, and that a restatement with one clause of the contract broken does
not stay inside it.  1e-5 on tables and moments after three Adam steps."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import inbatch_ref as ir
from inbatch_ref import ADAM, CASES, DIMS, NI, NU, REGS, T, case_reference, parity_case, tables, tolerance

pytestmark = pytest.mark.gpu


def to(dev, *xs):
    return [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


class State:
    """What ops.inbatch_step / ops.inbatch_adam_step write besides the tables."""

    def __init__(self, Ut, It):
        from pda_amd import ops
        z = torch.zeros_like
        self.mU, self.vU, self.gU, self.mI, self.vI, self.gI = z(Ut), z(Ut), z(Ut), z(It), z(It), z(It)
        self.tagU, self.tagI = ops.adam_row_tags(Ut.shape[0], It.shape[0], Ut.device)

    def adam(self, Ut, It):
        return (Ut, self.mU, self.vU, self.gU, self.tagU, It, self.mI, self.vI, self.gI, self.tagI)


def run_step(dev, U, I, users, pos, *, tau, norm, reg_div, logq=None, excl=None, step=1, **kw):
    from pda_amd import ops
    Ut, It, ut, pt, lq = to(dev, U, I, users, pos, logq)
    mask = None if excl is None else to(dev, ir.pack_mask(excl))[0]
    st = State(Ut, It)
    loss = torch.zeros(3, device=dev)
    ws = ops.inbatch_workspace(len(users), U.shape[1], dev)
    ws.fill_(0xFF)                                                      # (NaN patterns: the step relies on nothing it has not written)
    ops.inbatch_step(Ut, It, ut, pt, st.gU, st.gI, st.tagU, st.tagI, ws, tau=tau, norm=norm, regs=REGS, reg_div=reg_div, step=step, logq=lq,
                     mask=mask, loss_acc=loss, **kw)
    return loss.cpu().numpy(), st.gU.cpu().numpy(), st.gI.cpu().numpy(), st


def check(got, ref, tol, what):
    loss, gU, gI = got[:3]
    terms, rU, rI = ref[:3]
    print("in-batch %s: max |loss err| %.3g  max |gU err| %.3g  max |gI err| %.3g  (bound %.3g)" % (what, np.abs(loss - terms).max(),
                                                                                                np.abs(gU - rU).max(), np.abs(gI - rI).max(), tol))
    assert np.isfinite(loss).all() and np.isfinite(gU).all() and np.isfinite(gI).all()
    np.testing.assert_allclose(loss, terms, atol=tol, rtol=0)
    np.testing.assert_allclose(gU, rU, atol=tol, rtol=0)
    np.testing.assert_allclose(gI, rI, atol=tol, rtol=0)
    assert abs(loss[0] - (loss[1] + loss[2])) <= tol


def check_tags(st, users, pos, tag):
    """Exactly the batch's distinct rows carry the tag, as pda_adam_step_f32 leaves them."""
    S_u, S_i = np.unique(users), np.unique(pos)
    tagU, tagI = st.tagU.cpu().numpy(), st.tagI.cpu().numpy()
    assert (np.nonzero(tagU)[0] == S_u).all() and (np.nonzero(tagI)[0] == S_i).all() and set(tagU[S_u]) == {tag} and set(tagI[S_i]) == {tag}


@functools.lru_cache(maxsize=None)
def reference(case):
    return case_reference(case)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "d%d-B%d-norm%d-tau%g-logq%d-mask%d-%s-%s" % (c[0], c[1], c[2], c[3], c[4], c[5],
                                                                                                   "grouped" if c[6] else "any",
                                                                                                   "distinct" if c[7] else "rep"))
def test_gradients_and_loss_against_the_float64_restatement(dev, case):
    """24 cases: with every d, B in {1, 2, T + 3, 2 T + 5} (partial row and column tiles, more than one column split from T + 3 on), both norms,
    both taus, logq on and off, the mask given and null, PDA_UPD_ANY_ORDER on a shuffled batch and the grouped rule on a sorted one, with and
    without PDA_UPD_USERS_DISTINCT."""
    from pda_amd import ops
    d, B, norm, tau, use_logq, use_mask, grouped, distinct = case
    c, logq, excl = parity_case(*case)
    assert ops.inbatch_col_splits(B) > 1 or B <= T
    loss, gU, gI, st = run_step(dev, c["U"], c["I"], c["users"], c["pos"], tau=tau, norm=norm, reg_div=B, logq=logq, excl=excl, step=5,
                                grouped=grouped, users_distinct=distinct)
    check((loss, gU, gI), reference(case), tolerance(tau), "d=%d B=%d norm=%d tau=%g logq=%d mask=%d grouped=%d distinct=%d" % case)
    check_tags(st, c["users"], c["pos"], 5)


@pytest.mark.parametrize("d, norm", [(32, 1), (128, 0)])
def test_a_whole_column_tile_excluded_and_a_row_alone_with_its_diagonal(dev, d, norm):
    """Row 1's user holds every item of columns [T, 2 T) in its train set: one split of that row has no admitted column (m = -inf, se = 0) and
    the merge must give finite numbers.  Row 3 is excluded everywhere but its diagonal: l_3 = 0 and it takes only the regulariser."""
    from pda_amd import ops
    B, tau = 2 * T + 5, 0.1
    c = ir.make_case(900 + d, d, B, distinct=True)
    users, pos, train = c["users"], c["pos"], c["train"]
    assert ops.inbatch_col_splits(B) == 3                                # one column tile per split: columns [T, 2 T) are a split of their own
    train[int(users[1])] |= {int(p) for p in pos[T:2 * T]}
    train[int(users[3])] |= {int(p) for p in pos}
    excl = ir.exclusion(users, pos, train, c["nU"], c["nI"])
    assert excl[1, T:2 * T].all() and excl[3, np.arange(B) != 3].all() and not excl[3, 3]
    logq = ir.logq_ref(train, c["nI"], range(c["nU"]))
    ref = ir.reference(c["U"], c["I"], users, pos, excl=excl, logq=logq, tau=tau, norm=norm, regs=0.0, reg_div=B)
    assert ref[3][3] == 0.0
    # regs = 0: row 3's user gradient is exactly zero
    Ut, It, ut, pt, lq = to(dev, c["U"], c["I"], users, pos, logq)
    st, loss = State(Ut, It), torch.zeros(3, device=dev)
    ops.inbatch_step(Ut, It, ut, pt, st.gU, st.gI, st.tagU, st.tagI, ops.inbatch_workspace(B, d, dev), tau=tau, norm=norm, regs=0.0, reg_div=B,
                      step=1, logq=lq, mask=to(dev, ir.pack_mask(excl))[0], users_distinct=True, loss_acc=loss)
    got = (loss.cpu().numpy(), st.gU.cpu().numpy(), st.gI.cpu().numpy())
    check(got, ref, tolerance(tau), "column tile excluded d=%d norm=%d" % (d, norm))
    assert np.abs(got[1][users[3]]).max() <= 1e-9                       # p_33 = 1: C_33 = 0


@pytest.mark.parametrize("d, norm", [(32, 0), (256, 1)])
def test_rows_with_an_id_outside_the_tables_are_dropped_as_rows_and_as_columns(dev, d, norm):
    """A user and a positive outside the tables, inside a tile and across the tile boundary: the batch equals the remaining rows with the
    mean still over B, under either batch rule, and the tags are set on exactly the kept rows."""
    from pda_amd import ops
    B, tau = 2 * T + 5, 0.1
    c = ir.make_case(1300 + d, d, B)
    users, pos = c["users"].copy(), c["pos"].copy()
    with pytest.raises(ValueError, match="outside the tables"):         # ops checks the ids when asked to
        bad = pos.copy()
        bad[0] = c["nI"]
        Ut, It, ut, pt = to(dev, c["U"], c["I"], users, bad)
        st = State(Ut, It)
        ops.inbatch_step(Ut, It, ut, pt, st.gU, st.gI, st.tagU, st.tagI, ops.inbatch_workspace(B, d, dev), tau=tau, norm=norm, regs=REGS, reg_div=B,
                         step=1)
    assert float(st.gU.abs().max()) == 0.0 and int(st.tagI.abs().max()) == 0            # nothing was launched
    users[1], pos[5], users[T - 1], pos[T], users[2 * T + 4] = -1, c["nI"], c["nU"], -7, c["nU"] + 9
    keep = ir.valid_rows(users, pos, c["nU"], c["nI"])
    assert (~keep).sum() == 5
    excl = ir.exclusion(users, pos, c["train"], c["nU"], c["nI"])
    logq = ir.logq_ref(c["train"], c["nI"], range(c["nU"]))
    ref = ir.reference(c["U"], c["I"], users, pos, excl=excl, logq=logq, tau=tau, norm=norm, regs=REGS, reg_div=B)
    for grouped in (False, True):
        if grouped:
            order = np.argsort(np.where(keep, pos, -1), kind="stable")
            users, pos, excl, keep = users[order], pos[order], excl[np.ix_(order, order)], keep[order]
        loss, gU, gI, st = run_step(dev, c["U"], c["I"], users, pos, tau=tau, norm=norm, reg_div=B, logq=logq, excl=excl, step=3, grouped=grouped,
                                    check_ids=False)
        check((loss, gU, gI), ref, tolerance(tau), "five rows dropped d=%d norm=%d grouped=%d" % (d, norm, grouped))
        check_tags(st, users[keep], pos[keep], 3)
    users[:] = c["nU"]                                                   # every row dropped: nothing moves
    loss, gU, gI, st = run_step(dev, c["U"], c["I"], users, pos, tau=tau, norm=norm, reg_div=B, check_ids=False)
    assert np.abs(loss).max() == 0.0 and np.abs(gU).max() == 0.0 and np.abs(gI).max() == 0.0 and int(st.tagU.abs().max()) == 0 == int(st.tagI.abs().max())


@pytest.mark.parametrize("d", [32, 128])
def test_a_saturated_batch_stays_finite_and_keeps_its_loss(dev, d):
    """tau = 0.1, norm = 0, hand-built rows on one axis (every logit exact in float32): u = 8 e_0 against items +10 e_0, -10 e_0 and 0 gives
    the logits +800, -800 and 0.  Row 0: the positive at +800 (loss log 2: column 3 is at +800 too); row 1: the positive at -800 against +800
    (loss 1 600 + log 2); row 2: the positive at 0; row 3 (a user orthogonal to the items): all logits 0, loss log 4."""
    tau, B = 0.1, 4
    U, I = np.zeros((NU, d), np.float32), np.zeros((NI, d), np.float32)
    U[0, 0], U[1, 1] = 8.0, 8.0
    I[0, 0], I[1, 0], I[3, 0] = 10.0, -10.0, 10.0                       # item 2: the zero row
    users, pos = np.array([0, 0, 0, 1], np.int32), np.array([0, 1, 2, 3], np.int32)
    ref = ir.reference(U, I, users, pos, tau=tau, norm=0, regs=REGS, reg_div=B)
    assert abs(ref[3][1] - (1600.0 + np.log(2.0))) < 1e-9 and abs(ref[3][3] - np.log(4.0)) < 1e-12
    for grouped in (False, True):
        loss, gU, gI, _ = run_step(dev, U, I, users, pos, tau=tau, norm=0, reg_div=B, grouped=grouped)
        check((loss, gU, gI), ref, 1e-4, "saturated d=%d grouped=%d" % (d, grouped))


@pytest.mark.parametrize("d", DIMS)
def test_zero_rows_under_the_normalisation_give_finite_numbers(dev, d):
    rng = np.random.default_rng(d)
    U, I = tables(rng, d)
    U[3], I[5], I[6] = 0.0, 0.0, 1e-30                                 # |x| below 1e-12: the derivative of x / 1e-12
    users, pos = np.array([3, 3, 4, 3], np.int32), np.array([5, 7, 8, 6], np.int32)
    for tau in (1.0, 0.1):
        loss, gU, gI, _ = run_step(dev, U, I, users, pos, tau=tau, norm=1, reg_div=4)
        assert np.isfinite(loss).all() and np.isfinite(gU).all() and np.isfinite(gI).all() and loss[1] > 0


@pytest.mark.parametrize("d, norm, tau", [(32, 1, 0.1), (64, 0, 1.0), (128, 1, 1.0), (256, 0, 0.1)])
def test_the_sampled_softmax_kernel_fed_the_other_positives_agrees(dev, d, norm, tau):
    """logq and mask null, distinct positives, regs = 0: pda_inbatch_step_f32 and pda_ssm_step_f32 with negs[r] = pos[c != r] compute the same
    loss and gradients -- each within the bound of one float64 value, so within twice the bound of each other."""
    from pda_amd import ops
    B = T + 3
    rng = np.random.default_rng(40 + d)
    U, I = tables(rng, d)
    users = rng.integers(0, 20, B).astype(np.int32)
    pos = rng.permutation(NI)[:B].astype(np.int32)
    negs = np.stack([np.delete(pos, r) for r in range(B)]).astype(np.int32)
    assert negs.shape == (B, B - 1) and B - 1 <= 256
    ref = ir.reference(U, I, users, pos, tau=tau, norm=norm, regs=0.0, reg_div=B)
    Ut, It, ut, pt, nt = to(dev, U, I, users, pos, negs)
    got = []
    for which in ("inbatch", "ssm"):
        st, loss = State(Ut, It), torch.zeros(3, device=dev)
        if which == "inbatch":
            ops.inbatch_step(Ut, It, ut, pt, st.gU, st.gI, st.tagU, st.tagI, ops.inbatch_workspace(B, d, dev), tau=tau, norm=norm, regs=0.0,
                             reg_div=B, step=1, loss_acc=loss)
        else:
            ops.ssm_step(Ut, It, ut, pt, nt, st.gU, st.gI, st.tagU, st.tagI, tau=tau, norm=norm, regs=0.0, reg_div=B, step=1, loss_acc=loss)
        got.append((loss.cpu().numpy(), st.gU.cpu().numpy(), st.gI.cpu().numpy()))
        check(got[-1], ref, tolerance(tau), "%s kernel, shared negatives d=%d norm=%d tau=%g" % (which, d, norm, tau))
    w = ir.worst(got[0], got[1])
    print("in-batch against the sampled kernel d=%d: differ by %.3g (bound %.3g)" % (d, w, 2 * tolerance(tau)))
    assert w <= 2 * tolerance(tau)


@pytest.mark.parametrize("B", [1, 33, 2 * T + 5])
def test_the_train_mask_bit_for_bit_against_python_sets(dev, B):
    from pda_amd import ops
    c = ir.make_case(500 + B, 32, B)
    users, pos, train = c["users"].copy(), c["pos"].copy(), c["train"]
    if B > 1:
        train[int(users[0])] = set()                                    # an empty train row
        users[B - 1] = c["nU"]                                          # an invalid id: its row and its column are zero
    if B > 40:
        pos[T + 1] = -3
    indptr, indices = ir.csr(train, c["nU"])
    want = ir.exclusion(users, pos, train, c["nU"], c["nI"])
    ut, pt, ip, ix = to(dev, users, pos, indptr, indices)
    out = torch.full((B, (B + 31) // 32), -1, dtype=torch.int32, device=dev)
    got = ops.inbatch_mask(ut, pt, ip, ix, c["nU"], c["nI"], out=out)
    assert got is out
    np.testing.assert_array_equal(got.cpu().numpy(), ir.pack_mask(want))                 # the bits of c >= B are zero as well
    again = ops.inbatch_mask(ut, pt, ip, ix, c["nU"], c["nI"])
    assert torch.equal(again, got)
    if B > 1:
        assert not want[0].any() and not want[B - 1].any() and not want[:, B - 1].any() and want.any()


@functools.lru_cache(maxsize=None)
def adam_reference(norm):
    return ir.adam_reference(norm)


@pytest.mark.parametrize("policy", [1, 2], ids=["resident", "stream"])
@pytest.mark.parametrize("norm", [0, 1])
def test_three_whole_steps_against_the_restatement(dev, norm, policy):
    """The mask kernel, the step and the sweep, three times, at the d, lr and tau of ssm_ref.ADAM_STEPS (which says why the trainer's default
    learning rate)."""
    from pda_amd import ops
    c, batches, logq = ir.adam_case()
    ref, terms = adam_reference(norm)
    Ut, It, lq, ip, ix = to(dev, c["U"], c["I"], logq, *ir.csr(c["train"], c["nU"]))
    st = State(Ut, It)
    ws = ops.inbatch_workspace(ADAM["B"], ADAM["d"], dev)
    for t, (users, pos) in enumerate(batches, 1):
        ut, pt = to(dev, users, pos)
        loss = torch.zeros(3, device=dev)
        mask = ops.inbatch_mask(ut, pt, ip, ix, c["nU"], c["nI"])
        ops.inbatch_adam_step(*st.adam(Ut, It), ut, pt, ws, tau=ADAM["tau"], norm=norm, regs=REGS, reg_div=ADAM["B"], step=t,
                              lr_t=ops.adam_lr_t(ADAM["lr"], t), logq=lq, mask=mask, cache_policy=policy, loss_acc=loss, check_ids=True)
        np.testing.assert_allclose(loss.cpu().numpy(), terms[t - 1], atol=tolerance(ADAM["tau"]), rtol=0)
        assert float(st.gU.abs().max()) == 0.0 and float(st.gI.abs().max()) == 0.0        # g is zero again
        tagI = st.tagI.cpu().numpy()
        assert set(tagI[np.unique(pos)]) == {t} and tagI.max() == t
    got = dict(U=Ut, I=It, mU=st.mU, vU=st.vU, mI=st.mI, vI=st.vI)
    for k in got:
        print("in-batch three steps (norm=%d policy=%d): max |%s err| %.3g" % (norm, policy, k, np.abs(got[k].cpu().numpy() - ref[k]).max()))
    for k in got:
        np.testing.assert_allclose(got[k].cpu().numpy(), ref[k], atol=1e-5, rtol=0, err_msg=k)


@pytest.mark.parametrize("norm", [0, 1])
def test_the_mask_the_step_and_the_sweep_replay_from_a_captured_graph(dev, norm):
    """Nothing is read back on the host: the mask, the step and the sweep captured once and replayed three times give the tables of three eager
    steps (the tag of the captured step is fixed: the eager steps take the same one)."""
    from pda_amd import ops
    d, B, tau = 64, 200, 0.1
    c = ir.make_case(77, d, B)
    logq = ir.logq_ref(c["train"], c["nI"], range(c["nU"]))
    ut, pt, lq, ip, ix = to(dev, c["users"], c["pos"], logq, *ir.csr(c["train"], c["nU"]))

    def one_step(Ut, It, st, loss, ws, mask):
        ops.inbatch_mask(ut, pt, ip, ix, c["nU"], c["nI"], out=mask)
        ops.inbatch_adam_step(*st.adam(Ut, It), ut, pt, ws, tau=tau, norm=norm, regs=REGS, reg_div=B, step=1, lr_t=ops.adam_lr_t(1e-2, 1), logq=lq,
                              mask=mask, loss_acc=loss)

    def fresh():
        Ut, It = to(dev, c["U"], c["I"])
        return Ut, It, State(Ut, It), torch.zeros(3, device=dev), ops.inbatch_workspace(B, d, dev), torch.zeros((B, (B + 31) // 32), dtype=torch.int32,
                                                                                                                device=dev)
    a = fresh()
    for _ in range(3):
        one_step(*a)
    b = fresh()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            one_step(*b)
    torch.cuda.synchronize()
    assert torch.equal(b[0].cpu(), torch.from_numpy(c["U"]))             # capturing runs nothing
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    tol = tolerance(tau)
    print("in-batch graph replay norm=%d: max |U diff| %.3g  max |I diff| %.3g  loss diff %.3g (bound %.3g)" % (
        norm, float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max()), float((a[3] - b[3]).abs().max()), tol))
    torch.testing.assert_close(b[0], a[0], atol=tol, rtol=0)
    torch.testing.assert_close(b[1], a[1], atol=tol, rtol=0)
    torch.testing.assert_close(b[3], a[3], atol=3 * tol, rtol=0)        # (the sum of three steps' losses)


def test_the_operating_point_against_float64(dev):
    """B = 2 048, d = 64, tau = 0.1, norm 1, logq and mask on: 64 x 64 tiles in 16 column splits."""
    d, B, tau = 64, 2048, 0.1
    c = ir.make_case(2048, d, B, distinct=True)
    logq = ir.logq_ref(c["train"], c["nI"], range(c["nU"]))
    excl = ir.exclusion(c["users"], c["pos"], c["train"], c["nU"], c["nI"])
    share = ir.excluded_share(c["users"], c["pos"], excl)
    assert 0.05 <= share <= 0.5, share
    ref = ir.reference(c["U"], c["I"], c["users"], c["pos"], excl=excl, logq=logq, tau=tau, norm=1, regs=REGS, reg_div=B)
    loss, gU, gI, st = run_step(dev, c["U"], c["I"], c["users"], c["pos"], tau=tau, norm=1, reg_div=B, logq=logq, excl=excl, step=2,
                                users_distinct=True)
    check((loss, gU, gI), ref, tolerance(tau), "operating point B=%d d=%d (%.1f %% excluded)" % (B, d, 100 * share))
    check_tags(st, c["users"], c["pos"], 2)


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------------
def test_cli_trains_in_batch_and_export_topk_ranks_its_checkpoint(dev, tmp_path):
    """python -m pda_amd.train_new_api --train ssm --test normal --ssm_source batch --epoch 3 --bias_report 1 --bias_groups 4 in a child process
    on the smallest synthetic dataset: losses finite and decreasing, the checkpoint written under the same "ssm" directory name with the three
    new keys, and export_topk on it equals torch.topk on the float64 product of the normalised checkpoint tables with the history masked (ties:
    as tests/test_gpu_ssm.py treats them).  The same run with --ssm_source sampled prints what --train ssm prints without the flag."""
    from pda_amd import ops, synthetic
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    synthetic.write_dataset(str(tmp_path / "data" / "toy"), n_users=200, n_items=150, mean_hist=12)
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def argv_for(sub, extra):
        return ["--data_path", str(tmp_path / "data") + "/", "--dataset", "toy", "--train", "ssm", "--test", "normal", "--epoch", "3", "--embed_size",
                "32", "--log_interval", "1", "--batch_size", "128", "--lr", "1e-2", "--regs", "1e-3", "--valid_set", "valid", "--pop_exp", "0.22",
                "--save_dir", str(tmp_path / sub) + "/", "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t", "--cuda", "0", "--eval_block", "128",
                "--bias_report", "1", "--bias_groups", "4"] + extra

    def train(sub, extra):
        r = subprocess.run([sys.executable, "-m", "pda_amd.train_new_api"] + argv_for(sub, extra), cwd=root, env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    argv = argv_for("ckpt", ["--ssm_source", "batch"])
    out = train("ckpt", ["--ssm_source", "batch"])
    assert "running SSM" in out and "recall=[" in out and "||--- bias@" in out and "training and testing end!!!!" in out
    losses = [float(m.group(1)) for m in re.finditer(r"Epoch \d+ \[[^\]]*\]: train==\[([-\d.]+)=[-\d.]+ \+ [-\d.]+\]", out)]
    print("in-batch CLI losses:", losses)
    assert len(losses) == 3 and np.isfinite(losses).all() and losses[0] > losses[1] > losses[2], losses
    best = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path / "ckpt") for f in fs if f == "best_ckpt.ckpt"]
    assert len(best) == 1 and "ssm_train_ssm" in best[0]
    sd = torch.load(best[0], map_location="cpu")
    assert sd["format"] == "pda_amd/2" and sd["user_embedding"].shape == (200, 32) and "mU" in sd
    assert (sd["ssm_source"], sd["ssm_logq"], sd["ssm_mask_train"], sd["ssm_norm"], sd["ssm_tau"]) == ("batch", 1, 1, 1, 0.1)
    assert float((sd["item_embedding"].double().norm(dim=1) - 1).abs().min()) > 1e-3           # the raw tables, not the normalised ones
    from pda_amd import export_topk
    from pda_amd import train_new_api as t
    res = export_topk.main(argv + ["--export_out", str(tmp_path / "lists.npz")])
    K = 50
    assert res["idx"].shape == (len(res["users"]), K) and len(res["users"]) > 0 and np.isfinite(res["val"]).all()
    U, I = ops.ssm_normalize_rows(sd["user_embedding"].to(dev).contiguous()), ops.ssm_normalize_rows(sd["item_embedding"].to(dev).contiguous())
    S = (U.double()[torch.from_numpy(res["users"]).long().to(dev)] @ I.double().T).cpu()
    for row, u in enumerate(res["users"]):
        S[row, torch.as_tensor(list(t.data.train_user_list.get(int(u), [])), dtype=torch.long)] = -np.inf
    val, idx = torch.topk(S, K + 1, dim=1)
    np.testing.assert_allclose(res["val"], val[:, :K].numpy(), atol=2e-6, rtol=0)
    gapped = ((val[:, :-1] - val[:, 1:]).min(dim=1).values > 1e-5).numpy()
    assert gapped.mean() >= 0.75, gapped.mean()
    np.testing.assert_array_equal(res["idx"][gapped], idx[:, :K].numpy()[gapped])


def test_cli_with_the_sampled_source_is_train_ssm_as_it_was(dev, tmp_path):
    """--ssm_source sampled against no --ssm_source at all, one epoch each in a child process: the same lines.  The sampled step sums with float
    atomics, so the losses are compared to 1e-4 and the metric lines by their text with the digits taken out."""
    from pda_amd import synthetic
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    synthetic.write_dataset(str(tmp_path / "data" / "toy"), n_users=200, n_items=150, mean_hist=12)
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    outs = []
    for sub, extra in (("a", []), ("b", ["--ssm_source", "sampled"])):
        argv = ["--data_path", str(tmp_path / "data") + "/", "--dataset", "toy", "--train", "ssm", "--test", "normal", "--epoch", "1", "--embed_size", "32",
                "--log_interval", "1", "--batch_size", "128", "--lr", "1e-2", "--regs", "1e-3", "--valid_set", "valid", "--pop_exp", "0.22",
                "--save_dir", str(tmp_path / sub) + "/", "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t", "--cuda", "0", "--eval_block", "128",
                "--ssm_negs", "8", "--bias_report", "1", "--bias_groups", "4"] + extra
        r = subprocess.run([sys.executable, "-m", "pda_amd.train_new_api"] + argv, cwd=root, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(r.stdout)
    loss = [[float(x) for x in re.search(r"train==\[([-\d.]+)=([-\d.]+) \+ ([-\d.]+)\]", o).groups()] for o in outs]
    np.testing.assert_allclose(loss[0], loss[1], atol=1e-4, rtol=0)
    shape = lambda o: [re.sub(r"[-\d.e+]+", "#", ln) for ln in o.splitlines() if "recall=[" in ln or "||--- bias@" in ln or "running SSM" in ln]      # noqa: E731
    assert len(shape(outs[0])) >= 3 and shape(outs[0]) == shape(outs[1])
    best = [dp for sub in "ab" for dp, _, fs in os.walk(tmp_path / sub) for f in fs if f == "best_ckpt.ckpt"]
    assert len(best) == 2 and all("ssm_train_ssm" in b for b in best)
    sd = torch.load(os.path.join(best[1], "best_ckpt.ckpt"), map_location="cpu")
    assert "ssm_source" not in sd and sd["ssm_negs"] == 8                # the checkpoint of a sampled run keeps the keys it had
