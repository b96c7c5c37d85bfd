"""GPU: the full-catalogue softmax (`--train ssm --ssm_source all`, include/pda_hip_fullsm.h) -- the gradient step against the float64
restatement of tests/fullsm_ref.py on its 24 cases (every d with every batch size, catalogue size, norm, tau, mask, user rule, and a batch
with ids outside the tables), a whole column tile excluded, a row alone with its positive, a saturated batch, zero rows, the sampled-softmax
kernel and the in-batch kernel fed the same columns, bit-reproducibility, the whole Adam step, graph replay and the CLI.

Tolerance (ssm_ref.tolerance): 1e-5 max(1, 1 / tau) absolute on every loss term, gradient element and row statistic.
tests/test_fullsm_host.py shows that the restatement in float32 stays inside it on the same inputs (about a tenth of it at worst), and that a
restatement with one clause of the contract broken is more than twice the bound away.  1e-5 on tables and moments after three Adam steps."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import fullsm_ref as fr
import inbatch_ref as ir
from fullsm_ref import ADAM, CASES, DIMS, NU, REGS, T, case_id, case_reference, parity_case, tables, tolerance

pytestmark = pytest.mark.gpu
NI = 200


def to(dev, *xs):
    return [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


class State:
    """What ops.fullsm_step / ops.fullsm_adam_step write besides the tables."""

    def __init__(self, Ut, It):
        from pda_amd import ops
        z = torch.zeros_like
        self.mU, self.vU, self.gU, self.mI, self.vI, self.gI = z(Ut), z(Ut), z(Ut), z(It), z(It), z(It)
        self.tagU, self.tagI = ops.adam_row_tags(Ut.shape[0], It.shape[0], Ut.device)

    def adam(self, Ut, It):
        return (Ut, self.mU, self.vU, self.gU, self.tagU, It, self.mI, self.vI, self.gI, self.tagI)


def run_step(dev, U, I, users, pos, *, tau, norm, reg_div, train=None, regs=REGS, step=1, **kw):
    """-> (loss [3], gU, gI, row_stats [B, 2], State).  train: {user: set} or None (no mask)."""
    from pda_amd import ops
    Ut, It, ut, pt = to(dev, U, I, users, pos)
    ip, ix = (None, None) if train is None else to(dev, *fr.csr(train, U.shape[0]))
    st = State(Ut, It)
    loss = torch.zeros(3, device=dev)
    stats = torch.full((len(users), 2), float("nan"), device=dev)
    ws = ops.fullsm_workspace(len(users), I.shape[0], U.shape[1], dev)
    ws.fill_(0xFF)                                                      # (NaN patterns: the step relies on nothing it has not written)
    ops.fullsm_step(Ut, It, ut, pt, st.gU, st.gI, st.tagU, st.tagI, ws, tau=tau, norm=norm, regs=regs, reg_div=reg_div, step=step,
                    train_indptr=ip, train_indices=ix, loss_acc=loss, row_stats=stats, **kw)
    return loss.cpu().numpy(), st.gU.cpu().numpy(), st.gI.cpu().numpy(), stats.cpu().numpy(), st


def check(got, ref, tol, what):
    loss, gU, gI = got[:3]
    terms, rU, rI = ref[:3]
    print("full softmax %s: max |loss err| %.3g  max |gU err| %.3g  max |gI err| %.3g  (bound %.3g)" % (
        what, np.abs(loss - terms).max(), np.abs(gU - rU).max(), np.abs(gI - rI).max(), tol))
    assert np.isfinite(loss).all() and np.isfinite(gU).all() and np.isfinite(gI).all()
    np.testing.assert_allclose(loss, terms, atol=tol, rtol=0)
    np.testing.assert_allclose(gU, rU, atol=tol, rtol=0)
    np.testing.assert_allclose(gI, rI, atol=tol, rtol=0)
    assert abs(loss[0] - (loss[1] + loss[2])) <= tol


def check_stats(stats, ref_stats, keep, tol, what):
    """(m_r, log se_r) of the valid rows against float64; (0, 0) on the dropped ones."""
    print("full softmax %s: max |m err| %.3g  max |log se err| %.3g" % (what, np.abs(stats[keep, 0] - ref_stats[:, 0]).max(initial=0),
                                                                        np.abs(stats[keep, 1] - ref_stats[:, 1]).max(initial=0)))
    np.testing.assert_allclose(stats[keep], ref_stats, atol=tol, rtol=0)
    assert (stats[~keep] == 0).all()


def check_tags(st, users, tag):
    """The batch's distinct valid users and EVERY item carry the tag."""
    S_u = np.unique(users)
    tagU, tagI = st.tagU.cpu().numpy(), st.tagI.cpu().numpy()
    assert (np.nonzero(tagU)[0] == S_u).all() and set(tagU[S_u]) <= {tag} and (tagI == tag).all()


@functools.lru_cache(maxsize=None)
def reference(case):
    return case_reference(case)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gradients_loss_and_row_statistics_against_the_float64_restatement(dev, case):
    """24 cases: with every d, B in {1, 33, 69}, n_items in {20, 70, 257, 5 000} (one partial tile; tiles plus a remainder; one item past a tile
    edge; more than one column split), both norms, both taus, the mask on and off, repeated users without PDA_UPD_USERS_DISTINCT and distinct
    users with it, Zipf positives with duplicates, and one batch per d with five ids outside the tables (B still divides the mean)."""
    from pda_amd import ops
    d, B, nI, norm, tau, use_mask, distinct, drop = case
    c, member = parity_case(*case)
    if nI == 5000:
        assert ops.fullsm_col_splits(nI, B) > 1
    loss, gU, gI, stats, st = run_step(dev, c["U"], c["I"], c["users"], c["pos"], tau=tau, norm=norm, reg_div=B, step=5,
                                       train=c["train"] if use_mask else None, users_distinct=distinct, check_ids=not drop)
    ref = reference(case)
    keep = fr.valid_rows(c["users"], c["pos"], c["nU"], nI)
    assert (~keep).sum() == (5 if drop else 0)
    check((loss, gU, gI), ref, tolerance(tau), case_id(case))
    check_stats(stats, ref[4], keep, tolerance(tau), case_id(case))
    check_tags(st, c["users"][keep], 5)


@pytest.mark.parametrize("d, norm", [(32, 1), (128, 0)])
def test_a_whole_column_tile_excluded_and_a_row_alone_with_its_positive(dev, d, norm):
    """Row 1's user holds every item of columns [T, 2 T) in its train set and its positive lies elsewhere: with one column tile per split that
    split of the row has no admitted column (m = -inf, se = 0) and the merge must give finite numbers.  Row 3's user holds EVERY item: only its
    positive is left, l_3 = 0, and with regs = 0 its gradient is exactly zero."""
    from pda_amd import ops
    B, nI, tau = 2 * T + 5, 257, 0.1
    c = fr.make_case(900 + d, d, B, nI, distinct=True)
    users, pos, train = c["users"], c["pos"], c["train"]
    assert ops.fullsm_col_splits(nI, B) == -(-nI // T)                   # one column tile per split
    pos[1] = 3
    train[int(users[1])] |= set(range(T, 2 * T)) | {3}
    train[int(users[3])] = set(range(nI))
    member = fr.membership(users, train, c["nU"], nI)
    ref = fr.reference(c["U"], c["I"], users, pos, member=member, tau=tau, norm=norm, regs=0.0, reg_div=B)
    assert ref[3][3] == 0.0 and ref[4][3, 1] == 0.0
    loss, gU, gI, stats, _ = run_step(dev, c["U"], c["I"], users, pos, tau=tau, norm=norm, reg_div=B, train=train, regs=0.0, users_distinct=True)
    check((loss, gU, gI), ref, tolerance(tau), "column tile excluded d=%d norm=%d" % (d, norm))
    check_stats(stats, ref[4], np.ones(B, dtype=bool), tolerance(tau), "column tile excluded")
    assert np.abs(gU[users[3]]).max() <= 1e-9 and stats[3, 1] == 0.0    # p = 1 on the positive: C = 0


def test_a_batch_of_dropped_rows_moves_nothing(dev):
    d, B, nI = 32, T + 3, 70
    c = fr.make_case(1300, d, B, nI)
    users = np.full(B, c["nU"], np.int32)
    loss, gU, gI, stats, st = run_step(dev, c["U"], c["I"], users, c["pos"], tau=0.1, norm=1, reg_div=B, train=c["train"], check_ids=False)
    assert np.abs(loss).max() == 0.0 and np.abs(gU).max() == 0.0 and np.abs(gI).max() == 0.0 and (stats == 0).all()
    assert int(st.tagU.abs().max()) == 0
    with pytest.raises(ValueError, match="outside the tables"):         # ops checks the ids when asked to
        run_step(dev, c["U"], c["I"], users, c["pos"], tau=0.1, norm=1, reg_div=B)


@pytest.mark.parametrize("d", [32, 128])
def test_a_saturated_batch_stays_finite_and_keeps_its_loss(dev, d):
    """tau = 0.1, norm = 0, hand-built rows on one axis (every logit exact in float32): u = 8 e_0 against items +10 e_0, -10 e_0 and 0 gives
    the logits +800, -800 and 0 (the other 197 items are zero rows).  Row 1: the positive at -800 against two items at +800, l = 1 600 + log 2.
    The gradients are held to the bound; the loss terms, whose size is 400, to 1e-6 of their size (float32 carries 6e-8 of it)."""
    tau, B = 0.1, 4
    U, I = np.zeros((NU, d), np.float32), np.zeros((NI, d), np.float32)
    U[0, 0], U[1, 1] = 8.0, 8.0
    I[0, 0], I[1, 0], I[3, 0] = 10.0, -10.0, 10.0
    users, pos = np.array([0, 0, 0, 1], np.int32), np.array([0, 1, 2, 3], np.int32)
    ref = fr.reference(U, I, users, pos, tau=tau, norm=0, regs=REGS, reg_div=B)
    assert abs(ref[3][1] - (1600.0 + np.log(2.0))) < 1e-9 and abs(ref[3][3] - np.log(float(NI))) < 1e-12
    loss, gU, gI, stats, _ = run_step(dev, U, I, users, pos, tau=tau, norm=0, reg_div=B)
    assert np.isfinite(loss).all() and np.isfinite(gU).all() and np.isfinite(gI).all() and np.isfinite(stats).all()
    np.testing.assert_allclose(loss, ref[0], rtol=1e-6, atol=0)
    np.testing.assert_allclose(gU, ref[1], atol=tolerance(tau), rtol=0)
    np.testing.assert_allclose(gI, ref[2], atol=tolerance(tau), rtol=0)


@pytest.mark.parametrize("d", DIMS)
def test_zero_rows_under_the_normalisation_give_finite_numbers(dev, d):
    rng = np.random.default_rng(d)
    U, I = tables(rng, d)
    U[3], I[5], I[6], I[NI - 1] = 0.0, 0.0, 1e-30, 0.0                 # |x| below 1e-12: the derivative of x / 1e-12
    users, pos = np.array([3, 3, 4, 3], np.int32), np.array([5, 7, 8, 6], np.int32)
    for tau in (1.0, 0.1):
        loss, gU, gI, stats, _ = run_step(dev, U, I, users, pos, tau=tau, norm=1, reg_div=4)
        assert np.isfinite(loss).all() and np.isfinite(gU).all() and np.isfinite(gI).all() and np.isfinite(stats).all() and loss[1] > 0


@pytest.mark.parametrize("d, norm, tau", [(32, 1, 0.1), (64, 0, 1.0), (128, 1, 1.0), (256, 0, 0.1)])
def test_the_sampled_softmax_kernel_fed_every_other_item_agrees(dev, d, norm, tau):
    """200 items, no mask, regs = 0: pda_fullsm_step_f32 and pda_ssm_step_f32 with negs[r] = all 199 other items compute the same loss and
    gradients -- each within the bound of one float64 value, so within twice the bound of each other.  The two kernels share no code."""
    from pda_amd import ops
    B = T + 3
    rng = np.random.default_rng(40 + d)
    U, I = tables(rng, d)
    users = rng.integers(0, 20, B).astype(np.int32)
    pos = ir.zipf(rng, B, NI).astype(np.int32)
    negs = np.stack([np.delete(np.arange(NI), p) for p in pos]).astype(np.int32)
    assert negs.shape == (B, NI - 1) and NI - 1 <= ops.SSM_MAX_NEGS
    ref = fr.reference(U, I, users, pos, tau=tau, norm=norm, regs=0.0, reg_div=B)
    full = run_step(dev, U, I, users, pos, tau=tau, norm=norm, reg_div=B, regs=0.0)[:3]
    check(full, ref, tolerance(tau), "full kernel against float64 d=%d norm=%d tau=%g" % (d, norm, tau))
    Ut, It, ut, pt, nt = to(dev, U, I, users, pos, negs)
    st, loss = State(Ut, It), torch.zeros(3, device=dev)
    ops.ssm_step(Ut, It, ut, pt, nt, st.gU, st.gI, st.tagU, st.tagI, tau=tau, norm=norm, regs=0.0, reg_div=B, step=1, loss_acc=loss)
    sampled = (loss.cpu().numpy(), st.gU.cpu().numpy(), st.gI.cpu().numpy())
    w = fr.worst(full, sampled)
    print("full softmax against the sampled kernel d=%d: differ by %.3g (bound %.3g)" % (d, w, 2 * tolerance(tau)))
    assert w <= 2 * tolerance(tau)


@pytest.mark.parametrize("d, norm, tau", [(32, 0, 0.1), (64, 1, 0.1), (128, 0, 1.0), (256, 1, 1.0)])
def test_the_in_batch_kernel_on_a_permutation_of_all_items_agrees(dev, d, norm, tau):
    """The positives of the batch are a permutation of all 70 items, so the in-batch columns ARE the catalogue: pda_inbatch_step_f32 without logq
    and with its train mask computes the loss and gradients of pda_fullsm_step_f32 with the train graph, within twice the bound."""
    from pda_amd import ops
    B = nI = 70
    c = fr.make_case(70 + d, d, B, nI)
    users, train = c["users"], c["train"]
    pos = np.random.default_rng(d).permutation(nI).astype(np.int32)
    for u, p in zip(users, pos):
        train[int(u)].add(int(p))
    full = run_step(dev, c["U"], c["I"], users, pos, tau=tau, norm=norm, reg_div=B, train=train)[:3]
    excl = ir.exclusion(users, pos, train, c["nU"], nI)
    Ut, It, ut, pt, mask = to(dev, c["U"], c["I"], users, pos, ir.pack_mask(excl))
    st, loss = State(Ut, It), torch.zeros(3, device=dev)
    ops.inbatch_step(Ut, It, ut, pt, st.gU, st.gI, st.tagU, st.tagI, ops.inbatch_workspace(B, d, dev), tau=tau, norm=norm, regs=REGS, reg_div=B,
                     step=1, mask=mask, loss_acc=loss)
    inb = (loss.cpu().numpy(), st.gU.cpu().numpy(), st.gI.cpu().numpy())
    w = fr.worst(full, inb)
    print("full softmax against the in-batch kernel d=%d: differ by %.3g (bound %.3g)" % (d, w, 2 * tolerance(tau)))
    assert 0.1 <= excl.mean() <= 0.5 and np.abs(inb[2]).max() > 100 * tolerance(tau)
    assert w <= 2 * tolerance(tau)


@pytest.mark.parametrize("d, nI", [(64, 5000), (256, 257)])
def test_two_calls_on_distinct_users_give_the_same_bits(dev, d, nI):
    """No float atomic and no sum of varying order under PDA_UPD_USERS_DISTINCT: loss, gU, gI and the row statistics bit for bit, with Zipf
    positives that repeat and more than one workgroup in the tail."""
    B = 69
    c = fr.make_case(31 + d, d, B, nI, distinct=True)
    assert len(np.unique(c["pos"])) < B
    a = run_step(dev, c["U"], c["I"], c["users"], c["pos"], tau=0.1, norm=1, reg_div=B, train=c["train"], users_distinct=True)
    b = run_step(dev, c["U"], c["I"], c["users"], c["pos"], tau=0.1, norm=1, reg_div=B, train=c["train"], users_distinct=True)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    assert np.abs(a[2]).max() > 0


@functools.lru_cache(maxsize=None)
def adam_reference(norm):
    return fr.adam_reference(norm)


@pytest.mark.parametrize("policy", [1, 2], ids=["resident", "stream"])
@pytest.mark.parametrize("norm", [0, 1])
def test_three_whole_steps_against_the_restatement(dev, norm, policy):
    """The step and the sweep, three times, at the d, lr and tau of ssm_ref.ADAM_STEPS (which says why the trainer's default learning rate)."""
    from pda_amd import ops
    c, batches = fr.adam_case()
    ref, terms = adam_reference(norm)
    Ut, It, ip, ix = to(dev, c["U"], c["I"], *fr.csr(c["train"], c["nU"]))
    st = State(Ut, It)
    ws = ops.fullsm_workspace(ADAM["B"], ADAM["nI"], ADAM["d"], dev)
    for t, (users, pos) in enumerate(batches, 1):
        ut, pt = to(dev, users, pos)
        loss = torch.zeros(3, device=dev)
        ops.fullsm_adam_step(*st.adam(Ut, It), ut, pt, ws, tau=ADAM["tau"], norm=norm, regs=REGS, reg_div=ADAM["B"], step=t,
                             lr_t=ops.adam_lr_t(ADAM["lr"], t), train_indptr=ip, train_indices=ix, cache_policy=policy, loss_acc=loss,
                             check_ids=True)
        np.testing.assert_allclose(loss.cpu().numpy(), terms[t - 1], atol=tolerance(ADAM["tau"]), rtol=0)
        assert float(st.gU.abs().max()) == 0.0 and float(st.gI.abs().max()) == 0.0        # g is zero again
        assert (st.tagI.cpu().numpy() == t).all()
    got = dict(U=Ut, I=It, mU=st.mU, vU=st.vU, mI=st.mI, vI=st.vI)
    for k in got:
        print("full softmax three steps (norm=%d policy=%d): max |%s err| %.3g" % (norm, policy, k, np.abs(got[k].cpu().numpy() - ref[k]).max()))
    for k in got:
        np.testing.assert_allclose(got[k].cpu().numpy(), ref[k], atol=1e-5, rtol=0, err_msg=k)


@pytest.mark.parametrize("norm", [0, 1])
def test_the_step_and_the_sweep_replay_from_a_captured_graph(dev, norm):
    """Nothing is read back on the host: the step and the sweep captured once and replayed three times give the tables of three eager steps
    (the tag of the captured step is fixed: the eager steps take the same one).  Users repeat: the bound, not the bits."""
    from pda_amd import ops
    d, B, nI, tau = 64, 200, 1000, 0.1
    c = fr.make_case(77, d, B, nI)
    ut, pt, ip, ix = to(dev, c["users"], c["pos"], *fr.csr(c["train"], c["nU"]))

    def one_step(Ut, It, st, loss, ws):
        ops.fullsm_adam_step(*st.adam(Ut, It), ut, pt, ws, tau=tau, norm=norm, regs=REGS, reg_div=B, step=1, lr_t=ops.adam_lr_t(1e-2, 1),
                             train_indptr=ip, train_indices=ix, loss_acc=loss)

    def fresh():
        Ut, It = to(dev, c["U"], c["I"])
        return Ut, It, State(Ut, It), torch.zeros(3, device=dev), ops.fullsm_workspace(B, nI, d, dev)
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
    print("full softmax graph replay norm=%d: max |U diff| %.3g  max |I diff| %.3g  loss diff %.3g (bound %.3g)" % (
        norm, float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max()), float((a[3] - b[3]).abs().max()), tol))
    assert float((a[1] - torch.from_numpy(c["I"]).to(dev)).abs().max()) > 1e-3          # the steps moved the tables
    torch.testing.assert_close(b[0], a[0], atol=tol, rtol=0)
    torch.testing.assert_close(b[1], a[1], atol=tol, rtol=0)
    torch.testing.assert_close(b[3], a[3], atol=3 * tol, rtol=0)        # (the sum of three steps' losses)


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------------
def test_cli_trains_on_the_whole_catalogue_and_export_topk_ranks_its_checkpoint(dev, tmp_path):
    """python -m pda_amd.train_new_api --train ssm --test normal --ssm_source all --epoch 3 --bias_report 1 --bias_groups 4 in a child process on
    the toy data of the in-batch CLI test: losses finite and decreasing, the checkpoint under the same "ssm" directory name with
    ssm_source == "all", and export_topk on it equals torch.topk on the float64 product of the normalised checkpoint tables (the model's
    score_tables()) with the history masked (ties: as tests/test_gpu_ssm.py treats them).  One epoch with --ssm_source sampled still prints the
    lines of --train ssm and keeps the keys its checkpoint had."""
    from pda_amd import ops, synthetic
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    synthetic.write_dataset(str(tmp_path / "data" / "toy"), n_users=200, n_items=150, mean_hist=12)
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def argv_for(sub, epochs, extra):
        return ["--data_path", str(tmp_path / "data") + "/", "--dataset", "toy", "--train", "ssm", "--test", "normal", "--epoch", str(epochs),
                "--embed_size", "32", "--log_interval", "1", "--batch_size", "128", "--lr", "1e-2", "--regs", "1e-3", "--valid_set", "valid",
                "--pop_exp", "0.22", "--save_dir", str(tmp_path / sub) + "/", "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t", "--cuda", "0",
                "--eval_block", "128", "--bias_report", "1", "--bias_groups", "4"] + extra

    def train(argv):
        r = subprocess.run(["timeout", "-k", "10", "280", sys.executable, "-m", "pda_amd.train_new_api"] + argv, cwd=root, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    argv = argv_for("ckpt", 3, ["--ssm_source", "all"])
    out = train(argv)
    assert "running SSM" in out and "recall=[" in out and "||--- bias@" in out and "training and testing end!!!!" in out
    losses = [float(m.group(1)) for m in re.finditer(r"Epoch \d+ \[[^\]]*\]: train==\[([-\d.]+)=[-\d.]+ \+ [-\d.]+\]", out)]
    print("full softmax CLI losses:", losses)
    assert len(losses) == 3 and np.isfinite(losses).all() and losses[0] > losses[1] > losses[2], losses
    best = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path / "ckpt") for f in fs if f == "best_ckpt.ckpt"]
    assert len(best) == 1 and "ssm_train_ssm" in best[0]
    sd = torch.load(best[0], map_location="cpu")
    assert sd["format"] == "pda_amd/2" and sd["user_embedding"].shape == (200, 32) and "mU" in sd
    assert (sd["ssm_source"], sd["ssm_mask_train"], sd["ssm_norm"], sd["ssm_tau"]) == ("all", 1, 1, 0.1) and "ssm_logq" not in sd
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
    # the sampled source, as it was
    out = train(argv_for("s", 1, ["--ssm_source", "sampled", "--ssm_negs", "8"]))
    assert "running SSM" in out and "recall=[" in out and "||--- bias@" in out and re.search(r"train==\[[-\d.]+=[-\d.]+ \+ [-\d.]+\]", out)
    best = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path / "s") for f in fs if f == "best_ckpt.ckpt"]
    sd = torch.load(best[0], map_location="cpu")
    assert len(best) == 1 and "ssm_source" not in sd and sd["ssm_negs"] == 8
