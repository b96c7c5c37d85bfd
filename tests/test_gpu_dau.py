"""GPU: the DirectAU loss (`--train dau`, include/pda_hip_dau.h) -- the gradient step against the float64 restatement of tests/dau_ref.py on its
24 cases (every d with every batch size, t, gamma, same, batch order and user rule), the degenerate batches, skipped ids, bit-reproducible
loss terms, the whole Adam step, graph replay, the operating point, the argument errors and the CLI.

Tolerance (dau_ref.tolerance): 1e-5 max(1, 2 t gamma) absolute on every loss term and gradient element.  tests/test_dau_host.py shows that the
restatement in float32 stays inside a quarter of it on the same inputs, and that a restatement with one clause of the contract broken does not
stay inside it.  1e-5 on tables and moments after three Adam steps."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import dau_ref as dr
from dau_ref import ADAM, CASES, DIMS, NI, NU, REGS, T, case_id, case_reference, parity_case, tables, tolerance

pytestmark = pytest.mark.gpu


def to(dev, *xs):
    return [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


class State:
    """What ops.dau_step / ops.dau_adam_step write besides the tables."""

    def __init__(self, Ut, It):
        from pda_amd import ops
        z = torch.zeros_like
        self.mU, self.vU, self.gU, self.mI, self.vI, self.gI = z(Ut), z(Ut), z(Ut), z(It), z(It), z(It)
        self.tagU, self.tagI = ops.adam_row_tags(Ut.shape[0], It.shape[0], Ut.device)

    def adam(self, Ut, It):
        return (Ut, self.mU, self.vU, self.gU, self.tagU, It, self.mI, self.vI, self.gI, self.tagI)


def run_step(dev, U, I, users, pos, *, t, gamma, same, reg_div, regs=REGS, step=1, **kw):
    """-> (loss [3], gU, gI, stat [4], State): one ops.dau_step on fresh buffers, the workspace pre-filled with 0xFF."""
    from pda_amd import ops
    Ut, It, ut, pt = to(dev, U, I, users, pos)
    st = State(Ut, It)
    loss, stat = torch.zeros(3, device=dev), torch.zeros(4, device=dev)
    ws = ops.dau_workspace(len(users), U.shape[1], dev)
    ws.fill_(0xFF)                                                      # (NaN patterns: the step relies on nothing it has not written)
    ops.dau_step(Ut, It, ut, pt, st.gU, st.gI, st.tagU, st.tagI, ws, t=t, gamma=gamma, same=same, regs=regs, reg_div=reg_div, step=step, stat=stat,
                 loss_acc=loss, **kw)
    return loss.cpu().numpy(), st.gU.cpu().numpy(), st.gI.cpu().numpy(), stat.cpu().numpy(), st


def check(got, ref, tol, what):
    loss, gU, gI, stat = got[:4]
    terms, rU, rI, rstat = ref[:4]
    print("DirectAU %s: max |loss err| %.3g  max |stat err| %.3g  max |gU err| %.3g  max |gI err| %.3g  (bound %.3g)" % (
        what, np.abs(loss - terms).max(), np.abs(stat[:3] - rstat).max(), np.abs(gU - rU).max(), np.abs(gI - rI).max(), tol))
    assert np.isfinite(loss).all() and np.isfinite(gU).all() and np.isfinite(gI).all() and np.isfinite(stat).all()
    np.testing.assert_allclose(loss, terms, atol=tol, rtol=0)
    np.testing.assert_allclose(stat[:3], rstat, atol=tol, rtol=0)
    np.testing.assert_allclose(gU, rU, atol=tol, rtol=0)
    np.testing.assert_allclose(gI, rI, atol=tol, rtol=0)
    assert loss[0] == np.float32(loss[1]) + np.float32(loss[2]) and stat[3] == 1.0         # loss = mf + reg, one step counted


def check_tags(st, users, pos, tag):
    """Exactly the batch's distinct rows carry the tag, as pda_adam_step_f32 leaves them."""
    S_u, S_i = np.unique(users), np.unique(pos)
    tagU, tagI = st.tagU.cpu().numpy(), st.tagI.cpu().numpy()
    assert (np.nonzero(tagU)[0] == S_u).all() and (np.nonzero(tagI)[0] == S_i).all() and set(tagU[S_u]) == {tag} and set(tagI[S_i]) == {tag}


@functools.lru_cache(maxsize=None)
def reference(case):
    return case_reference(case)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gradients_and_loss_against_the_float64_restatement(dev, case):
    """24 cases: with every d, B in {1, 2, T + 3, 2 T + 5} (partial row and column tiles, more than one column split from T + 3 on), both t, both
    gamma, keep and drop, PDA_UPD_ANY_ORDER on a shuffled batch and the grouped rule on a sorted one, with and without PDA_UPD_USERS_DISTINCT."""
    from pda_amd import ops
    d, B, t, gamma, same, grouped, distinct = case
    c = parity_case(*case)
    assert ops.dau_col_splits(B) > 1 or B <= T
    got = run_step(dev, c["U"], c["I"], c["users"], c["pos"], t=t, gamma=gamma, same=same, reg_div=B, step=5, grouped=grouped, users_distinct=distinct)
    check(got, reference(case), tolerance(t, gamma), case_id(case))
    check_tags(got[4], c["users"], c["pos"], 5)


@pytest.mark.parametrize("d", [32, 256])
def test_a_batch_of_one_row_has_alignment_and_regulariser_only(dev, d):
    c = dr.make_case(11 + d, d, 1)
    got = run_step(dev, c["U"], c["I"], c["users"], c["pos"], t=2.0, gamma=5.0, same="keep", reg_div=1)
    ref = dr.reference(c["U"], c["I"], c["users"], c["pos"], t=2.0, gamma=5.0, same="keep", regs=REGS, reg_div=1)
    check(got, ref, tolerance(2.0, 5.0), "B=1 d=%d" % d)
    assert got[3][1] == 0.0 and got[3][2] == 0.0 and got[0][1] == got[3][0] > 0


@pytest.mark.parametrize("d, B", [(32, T + 3), (128, 2 * T + 5)])
def test_every_row_with_the_same_item(dev, d, B):
    """drop: the item side has no admitted pair -- P = 0, uni_I = 0, no uniformity gradient on the item, finite everywhere.  keep: every pair
    is at distance 0 with e = 1 exactly -- uni_I = log 1 = 0 exactly, and again no uniformity gradient.  regs = 0: the item's gradient is the
    alignment's alone under both."""
    c = dr.make_case(300 + d, d, B, distinct=True)
    pos = np.full(B, 7, np.int32)
    t, gamma = 10.0, 5.0
    tol = tolerance(t, gamma)
    align_only = dr.reference(c["U"], c["I"], c["users"], pos, t=t, gamma=0.0, same="keep", regs=0.0, reg_div=B)
    for same in ("drop", "keep"):
        got = run_step(dev, c["U"], c["I"], c["users"], pos, t=t, gamma=gamma, same=same, reg_div=B, regs=0.0, users_distinct=True)
        ref = dr.reference(c["U"], c["I"], c["users"], pos, t=t, gamma=gamma, same=same, regs=0.0, reg_div=B)
        check(got, ref, tol, "one item, %s, d=%d B=%d" % (same, d, B))
        assert got[3][2] == 0.0, got[3]                                 # uni_I: exactly zero
        assert got[3][1] < 0.0                                          # the users are distinct: their side is alive
        np.testing.assert_allclose(got[2], align_only[2], atol=tol, rtol=0)
        assert np.abs(got[2][np.arange(NI) != 7]).max() == 0.0


@pytest.mark.parametrize("d", DIMS)
def test_zero_rows_under_the_normalisation_give_finite_numbers(dev, d):
    rng = np.random.default_rng(d)
    U, I = tables(rng, d)
    U[3], I[5], I[6] = 0.0, 0.0, 1e-30                                 # |x| below 1e-12: the derivative of x / 1e-12
    users, pos = np.array([3, 3, 4, 3, 9], np.int32), np.array([5, 7, 8, 6, 5], np.int32)
    for same in ("keep", "drop"):
        for t in (2.0, 10.0):
            loss, gU, gI, stat, _ = run_step(dev, U, I, users, pos, t=t, gamma=1.0, same=same, reg_div=5)
            assert np.isfinite(loss).all() and np.isfinite(gU).all() and np.isfinite(gI).all() and np.isfinite(stat).all() and stat[0] > 0


def alignment_only(U, I, users, pos, *, regs, reg_div):
    """The alignment-only restatement, on its own: mean |unit(u) - unit(i)|^2 plus the regulariser, autograd in float64."""
    Ut = torch.tensor(U, dtype=torch.float64, requires_grad=True)
    It = torch.tensor(I, dtype=torch.float64, requires_grad=True)
    u, it = Ut[torch.as_tensor(users, dtype=torch.long)], It[torch.as_tensor(pos, dtype=torch.long)]
    unit = lambda x: x / torch.linalg.vector_norm(x, dim=1, keepdim=True).clamp_min(1e-12)      # noqa: E731
    mf = ((unit(u) - unit(it)) ** 2).sum() / len(users)
    reg = regs * 0.5 * ((u ** 2).sum() + (it ** 2).sum()) / reg_div
    (mf + reg).backward()
    return np.array([float((mf + reg).detach()), float(mf.detach()), float(reg.detach())]), Ut.grad.numpy(), It.grad.numpy()


@pytest.mark.parametrize("d", [64, 128])
def test_gamma_zero_is_the_alignment_term_alone(dev, d):
    B = 2 * T + 5
    c = dr.make_case(500 + d, d, B)
    terms, rU, rI = alignment_only(c["U"], c["I"], c["users"], c["pos"], regs=REGS, reg_div=B)
    loss, gU, gI, stat, _ = run_step(dev, c["U"], c["I"], c["users"], c["pos"], t=10.0, gamma=0.0, same="keep", reg_div=B)
    tol = tolerance(10.0, 0.0)
    assert tol == 1e-5
    np.testing.assert_allclose(loss, terms, atol=tol, rtol=0)
    np.testing.assert_allclose(gU, rU, atol=tol, rtol=0)
    np.testing.assert_allclose(gI, rI, atol=tol, rtol=0)
    assert stat[1] < 0 and stat[2] < 0                                 # the uniformity terms are still reported


@pytest.mark.parametrize("d, same", [(32, "keep"), (256, "drop")])
def test_rows_with_an_id_outside_the_tables_are_dropped_as_rows_and_as_columns(dev, d, same):
    """A user and a positive outside the tables, inside a tile and across the tile boundary: the batch equals the remaining rows with the
    alignment mean still over B, under either batch rule, and the tags are set on exactly the kept rows."""
    from pda_amd import ops
    B, t, gamma = 2 * T + 5, 2.0, 5.0
    c = dr.make_case(1300 + d, d, B)
    users, pos = c["users"].copy(), c["pos"].copy()
    with pytest.raises(ValueError, match="outside the tables"):         # ops checks the ids when asked to
        bad = pos.copy()
        bad[0] = c["nI"]
        Ut, It, ut, pt = to(dev, c["U"], c["I"], users, bad)
        st = State(Ut, It)
        ops.dau_step(Ut, It, ut, pt, st.gU, st.gI, st.tagU, st.tagI, ops.dau_workspace(B, d, dev), t=t, gamma=gamma, same=same, regs=REGS, reg_div=B,
                     step=1)
    assert float(st.gU.abs().max()) == 0.0 and int(st.tagI.abs().max()) == 0            # nothing was launched
    users[1], pos[5], users[T - 1], pos[T], users[2 * T + 4] = -1, c["nI"], c["nU"], -7, c["nU"] + 9
    keep = dr.valid_rows(users, pos, c["nU"], c["nI"])
    assert (~keep).sum() == 5
    ref = dr.reference(c["U"], c["I"], users, pos, t=t, gamma=gamma, same=same, regs=REGS, reg_div=B)
    for grouped in (False, True):
        if grouped:
            order = np.argsort(np.where(keep, pos, -1), kind="stable")
            users, pos, keep = users[order], pos[order], keep[order]
        got = run_step(dev, c["U"], c["I"], users, pos, t=t, gamma=gamma, same=same, reg_div=B, step=3, grouped=grouped, check_ids=False)
        check(got, ref, tolerance(t, gamma), "five rows dropped d=%d %s grouped=%d" % (d, same, grouped))
        check_tags(got[4], users[keep], pos[keep], 3)
    users[:] = c["nU"]                                                   # every row dropped: nothing moves
    loss, gU, gI, stat, st = run_step(dev, c["U"], c["I"], users, pos, t=t, gamma=gamma, same=same, reg_div=B, check_ids=False)
    assert np.abs(loss).max() == 0.0 and np.abs(gU).max() == 0.0 and np.abs(gI).max() == 0.0 and int(st.tagU.abs().max()) == 0 == int(st.tagI.abs().max())
    assert (stat == np.array([0, 0, 0, 1], np.float32)).all()


@pytest.mark.parametrize("d, B", [(64, 2 * T + 5), (128, 700)])
def test_the_same_inputs_give_the_same_bits(dev, d, B):
    """No float atomics in r, n, G, S or P: loss_acc and stat carry the same bits on two calls, and with distinct users under
    PDA_UPD_USERS_DISTINCT (plain stores) so does gU.  gI takes the atomics of repeated items and is held to the bound only."""
    c = dr.make_case(40 + B, d, B, distinct=True)
    a = run_step(dev, c["U"], c["I"], c["users"], c["pos"], t=2.0, gamma=1.0, same="keep", reg_div=B, users_distinct=True)
    b = run_step(dev, c["U"], c["I"], c["users"], c["pos"], t=2.0, gamma=1.0, same="keep", reg_div=B, users_distinct=True)
    assert a[0].tobytes() == b[0].tobytes() and a[3].tobytes() == b[3].tobytes()
    assert a[1].tobytes() == b[1].tobytes() and np.abs(a[1]).max() > 0
    np.testing.assert_allclose(a[2], b[2], atol=tolerance(2.0, 1.0), rtol=0)


@functools.lru_cache(maxsize=None)
def adam_reference():
    return dr.adam_reference()


@pytest.mark.parametrize("policy", [1, 2], ids=["resident", "stream"])
def test_three_whole_steps_against_the_restatement(dev, policy):
    """The step and the sweep, three times, at the d, B and lr of the in-batch test's ADAM."""
    from pda_amd import ops
    c, batches = dr.adam_case()
    ref, terms = adam_reference()
    Ut, It = to(dev, c["U"], c["I"])
    st = State(Ut, It)
    ws = ops.dau_workspace(ADAM["B"], ADAM["d"], dev)
    stat = torch.zeros(4, device=dev)
    for step, (users, pos) in enumerate(batches, 1):
        ut, pt = to(dev, users, pos)
        loss = torch.zeros(3, device=dev)
        ops.dau_adam_step(*st.adam(Ut, It), ut, pt, ws, t=ADAM["t"], gamma=ADAM["gamma"], same=ADAM["same"], regs=REGS, reg_div=ADAM["B"], step=step,
                          lr_t=ops.adam_lr_t(ADAM["lr"], step), cache_policy=policy, stat=stat, loss_acc=loss, check_ids=True)
        np.testing.assert_allclose(loss.cpu().numpy(), terms[step - 1], atol=tolerance(ADAM["t"], ADAM["gamma"]), rtol=0)
        assert float(st.gU.abs().max()) == 0.0 and float(st.gI.abs().max()) == 0.0        # g is zero again
        tagI = st.tagI.cpu().numpy()
        assert set(tagI[np.unique(pos)]) == {step} and tagI.max() == step
    assert float(stat[3]) == 3.0
    got = dict(U=Ut, I=It, mU=st.mU, vU=st.vU, mI=st.mI, vI=st.vI)
    for k in got:
        print("DirectAU three steps (policy=%d): max |%s err| %.3g" % (policy, k, np.abs(got[k].cpu().numpy() - ref[k]).max()))
    for k in got:
        np.testing.assert_allclose(got[k].cpu().numpy(), ref[k], atol=1e-5, rtol=0, err_msg=k)


def test_the_step_and_the_sweep_replay_from_a_captured_graph(dev):
    """Nothing is read back on the host: the step and the sweep captured once and replayed three times give the tables of three eager steps (the
    tag of the captured step is fixed: the eager steps take the same one)."""
    from pda_amd import ops
    d, B, t, gamma = 64, 200, 2.0, 1.0
    c = dr.make_case(77, d, B)
    ut, pt = to(dev, c["users"], c["pos"])

    def one_step(Ut, It, st, loss, stat, ws):
        ops.dau_adam_step(*st.adam(Ut, It), ut, pt, ws, t=t, gamma=gamma, same="keep", regs=REGS, reg_div=B, step=1, lr_t=ops.adam_lr_t(1e-2, 1),
                          stat=stat, loss_acc=loss)

    def fresh():
        Ut, It = to(dev, c["U"], c["I"])
        return Ut, It, State(Ut, It), torch.zeros(3, device=dev), torch.zeros(4, device=dev), ops.dau_workspace(B, d, dev)
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
    tol = tolerance(t, gamma)
    print("DirectAU graph replay: max |U diff| %.3g  max |I diff| %.3g  loss diff %.3g (bound %.3g)" % (
        float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max()), float((a[3] - b[3]).abs().max()), tol))
    torch.testing.assert_close(b[0], a[0], atol=tol, rtol=0)
    torch.testing.assert_close(b[1], a[1], atol=tol, rtol=0)
    torch.testing.assert_close(b[3], a[3], atol=3 * tol, rtol=0)        # (the sum of three steps' losses)
    assert float(b[4][3]) == 3.0


def test_the_operating_point_against_float64(dev):
    """B = 2 048, d = 64, t = 2, gamma = 1, keep: 64 row tiles x 8 column splits x 2 sides."""
    from pda_amd import ops
    d, B, t, gamma = 64, 2048, 2.0, 1.0
    c = dr.make_case(2048, d, B, distinct=True)
    assert ops.dau_col_splits(B) == 8 and len(np.unique(c["pos"])) < B
    ref = dr.reference(c["U"], c["I"], c["users"], c["pos"], t=t, gamma=gamma, same="keep", regs=REGS, reg_div=B)
    got = run_step(dev, c["U"], c["I"], c["users"], c["pos"], t=t, gamma=gamma, same="keep", reg_div=B, step=2, users_distinct=True)
    check(got, ref, tolerance(t, gamma), "operating point B=%d d=%d" % (B, d))
    check_tags(got[4], c["users"], c["pos"], 2)


def test_ops_argument_errors(dev):
    """Each PDA_ERR_ARG clause and an unsupported d, through ops: the wrapper's own ValueError where it checks first, the library's error where
    it does not; nothing is launched either way."""
    from pda_amd import _lib, ops
    d, B = 32, 8
    c = dr.make_case(5, d, B)
    Ut, It, ut, pt = to(dev, c["U"], c["I"], c["users"], c["pos"])
    st = State(Ut, It)
    ws = ops.dau_workspace(B, d, dev)
    good = dict(t=2.0, gamma=1.0, same="keep", regs=REGS, reg_div=B, step=1)

    def step(ut=ut, pt=pt, ws=ws, tagU=None, **over):
        ops.dau_step(Ut, It, ut, pt, st.gU, st.gI, st.tagU if tagU is None else tagU, st.tagI, ws, **dict(good, **over))

    for over, match in (({"t": 0.0}, "t must"), ({"t": 20.5}, "t must"), ({"t": float("nan")}, "t must"), ({"gamma": -1.0}, "gamma"),
                        ({"gamma": float("inf")}, "gamma"), ({"same": "both"}, "same")):
        with pytest.raises(ValueError, match=match):
            step(**over)
    with pytest.raises(ValueError, match="workspace"):
        step(ws=ws[:-16])
    with pytest.raises(ValueError, match="same, non-zero length"):
        step(pt=pt[:-1])
    with pytest.raises(ValueError, match="tagU"):
        step(tagU=st.tagU[:-1])
    with pytest.raises(ValueError, match="width"):              # an unsupported d
        U48, I48 = torch.zeros(NU, 48, device=dev), torch.zeros(NI, 48, device=dev)
        ops.dau_step(U48, I48, ut, pt, torch.zeros_like(U48), torch.zeros_like(I48), st.tagU, st.tagI, ws, **good)
    big = torch.zeros(ops.DAU_MAX_B + 1, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="batch size"):
        step(ut=big, pt=big)
    for over in ({"reg_div": 0.0}, {"step": 0}):                        # (the library's own checks)
        with pytest.raises(_lib.PdaHipError, match="invalid argument"):
            step(**over)
    lib = _lib.load()
    args = lambda **o: [_lib.ptr(Ut), _lib.ptr(It), NU, NI, _lib.ptr(ut), _lib.ptr(pt), o.get("B", B), o.get("d", d), 2.0, 1.0, 0, REGS, float(B),      # noqa: E731
                        _lib.ptr(st.gU), _lib.ptr(st.gI), _lib.ptr(st.tagU), _lib.ptr(st.tagI), 1, o.get("flags", 0x100), _lib.ptr(ws),
                        o.get("wsb", ws.numel()), None, None, _lib.stream_ptr()]
    assert lib.pda_dau_step_f32(*args(flags=0x400)) == -1 and lib.pda_dau_step_f32(*args(wsb=16)) == -1 and lib.pda_dau_step_f32(*args(B=0)) == -1
    assert lib.pda_dau_step_f32(*args(d=48)) == -2
    torch.cuda.synchronize()
    assert float(st.gU.abs().max()) == 0.0 and int(st.tagU.abs().max()) == 0 == int(st.tagI.abs().max())        # nothing was launched


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------------
def test_cli_trains_directau_and_export_topk_ranks_its_checkpoint(dev, tmp_path):
    """python -m pda_amd.train_new_api --train dau --test normal --epoch 2 in a child process on the smallest synthetic dataset: the `||--- dau`
    line, losses finite and decreasing, the checkpoint written under the `dau` directory name with the four new keys, and export_topk with
    --dau_rank cosine equals torch.topk on the float64 product of the normalised checkpoint tables with the history masked."""
    from pda_amd import ops, synthetic
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    synthetic.write_dataset(str(tmp_path / "data" / "toy"), n_users=200, n_items=150, mean_hist=12)
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    argv = ["--data_path", str(tmp_path / "data") + "/", "--dataset", "toy", "--train", "dau", "--test", "normal", "--epoch", "2", "--embed_size",
            "32", "--log_interval", "1", "--batch_size", "128", "--lr", "1e-2", "--regs", "1e-3", "--valid_set", "valid", "--pop_exp", "0.22",
            "--save_dir", str(tmp_path / "ckpt") + "/", "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t", "--cuda", "0", "--eval_block", "128"]
    r = subprocess.run([sys.executable, "-m", "pda_amd.train_new_api"] + argv, cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert "running DirectAU" in out and "recall=[" in out and "training and testing end!!!!" in out
    lines = re.findall(r"\|\|--- dau align=([-\d.]+) uni_u=([-\d.]+) uni_i=([-\d.]+)", out)
    assert len(lines) == 2 and np.isfinite(np.array(lines, dtype=np.float64)).all(), out[-2000:]
    losses = [float(m.group(1)) for m in re.finditer(r"Epoch \d+ \[[^\]]*\]: train==\[([-\d.]+)=[-\d.]+ \+ [-\d.]+\]", out)]
    print("DirectAU CLI losses:", losses, "dau lines:", lines)
    assert len(losses) == 2 and np.isfinite(losses).all() and losses[0] > losses[1], losses
    best = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path / "ckpt") for f in fs if f == "best_ckpt.ckpt"]
    assert len(best) == 1 and "dau_train_dau" in best[0]
    sd = torch.load(best[0], map_location="cpu")
    assert sd["format"] == "pda_amd/2" and sd["user_embedding"].shape == (200, 32) and "mU" in sd
    assert (sd["dau_gamma"], sd["dau_t"], sd["dau_same"], sd["dau_rank"]) == (1.0, 2.0, "keep", "raw")
    from pda_amd import export_topk
    from pda_amd import train_new_api as t
    res = export_topk.main(argv + ["--dau_rank", "cosine", "--export_out", str(tmp_path / "lists.npz")])
    K = 50
    assert res["idx"].shape == (len(res["users"]), K) and len(res["users"]) > 0 and np.isfinite(res["val"]).all()
    U, I = ops.ssm_normalize_rows(sd["user_embedding"].to(dev).contiguous()), ops.ssm_normalize_rows(sd["item_embedding"].to(dev).contiguous())
    S = (U.double()[torch.from_numpy(res["users"]).long().to(dev)] @ I.double().T).cpu()
    for row, u in enumerate(res["users"]):
        S[row, torch.as_tensor(list(t.data.train_user_list.get(int(u), [])), dtype=torch.long)] = -np.inf
    val, idx = torch.topk(S, K + 1, dim=1)
    np.testing.assert_allclose(res["val"], val[:, :K].numpy(), atol=2e-6, rtol=0)
    gapped = ((val[:, :-1] - val[:, 1:]).min(dim=1).values > 1e-5).numpy()
    assert gapped.mean() >= 0.5, gapped.mean()
    np.testing.assert_array_equal(res["idx"][gapped], idx[:, :K].numpy()[gapped])
