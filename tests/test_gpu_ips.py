"""GPU: the IPS baselines (`--train ips`, include/pda_hip_ips.h) -- the weighted gradient step against the float64 restatement of
tests/ips_ref.py, against the plain BPR step when every weight is one, the whole Adam step, the weight sum, graph replay, and the CLI.

Tolerances (ips_ref.tolerance): 1e-5 absolute on every loss term and gradient element for the self-normalised variant, 1e-5 max(1, w_max) for
the two unnormalised ones, w_max the largest weight in the batch -- every term is w_t times a quantity the BPR and DICE tests hold to 1e-5.
tests/test_ips_host.py shows that the restatement in float32 stays inside a quarter of these bounds on the same inputs.  1e-5 on tables and
moments after three Adam steps."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ips_ref import BATCHES, COUNTS, DIMS, NI, NU, TOL, VARIANTS, batch, ips_adam, ips_grads, ips_weights, parity_case, tables, tolerance

pytestmark = pytest.mark.gpu
REGS = 1e-2


def to(dev, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


class State:
    """What ops.ips_grads / ops.ips_adam_step write besides the tables."""

    def __init__(self, Ut, It):
        from pda_amd import ops
        z = torch.zeros_like
        self.mU, self.vU, self.gU, self.mI, self.vI, self.gI = z(Ut), z(Ut), z(Ut), z(It), z(It), z(It)
        self.tagU, self.tagI = ops.adam_row_tags(Ut.shape[0], It.shape[0], Ut.device)
        self.wsum = torch.zeros(1, dtype=torch.float32, device=Ut.device)

    def adam(self, Ut, It):
        return (Ut, self.mU, self.vU, self.gU, self.tagU, It, self.mI, self.vI, self.gI, self.tagI)


def run_grads(dev, U, I, b, ipw, norm, reg_div, step=1, **kw):
    from pda_amd import ops
    Ut, It, ut, pt, nt, wt = to(dev, U, I, *b, ipw)
    st = State(Ut, It)
    loss = torch.zeros(3, device=dev)
    ops.ips_grads(Ut, It, ut, pt, nt, wt, st.gU, st.gI, st.tagU, st.tagI, wsum=st.wsum if norm else None, regs=REGS, reg_div=reg_div, step=step,
                  loss_acc=loss, **kw)
    return loss.cpu().numpy(), st.gU.cpu().numpy(), st.gI.cpu().numpy(), st


@functools.lru_cache(maxsize=None)
def reference(d, B, variant):
    U, I, b, ipw, norm = parity_case(d, B, variant)
    return ips_grads(U, I, *b, ipw, norm=norm, regs=REGS, reg_div=B)


def check(got, ref, tol, what):
    loss, gU, gI = got
    terms, rU, rI = ref
    print("ips %s: max |loss err| %.3g  max |gU err| %.3g  max |gI err| %.3g  (bound %.3g)" % (what, np.abs(loss - terms).max(), np.abs(gU - rU).max(),
                                                                                           np.abs(gI - rI).max(), tol))
    np.testing.assert_allclose(loss, terms, atol=tol, rtol=0)
    np.testing.assert_allclose(gU, rU, atol=tol, rtol=0)
    np.testing.assert_allclose(gI, rI, atol=tol, rtol=0)
    assert abs(loss[0] - (loss[1] + loss[2])) <= tol


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("d", DIMS)
def test_gradients_and_loss_against_the_float64_restatement(dev, d, B):
    for variant in VARIANTS:
        U, I, b, ipw, norm = parity_case(d, B, variant)
        loss, gU, gI, st = run_grads(dev, U, I, b, ipw, norm, B, step=5)
        check((loss, gU, gI), reference(d, B, variant), tolerance(ipw, b[1], norm), "%s d=%d B=%d" % (variant, d, B))
        # the tags: exactly the batch's distinct rows, as pda_adam_step_f32 leaves them
        S_u, S_i = np.unique(b[0]), np.unique(np.concatenate([b[1], b[2]]))
        tagU, tagI = st.tagU.cpu().numpy(), st.tagI.cpu().numpy()
        assert (np.nonzero(tagU)[0] == S_u).all() and (np.nonzero(tagI)[0] == S_i).all() and set(tagU[S_u]) == {5} and set(tagI[S_i]) == {5}
        if B == 2048:       # every item is hot: about a hundred summed occurrences per row
            assert len(S_i) == NI and np.bincount(np.concatenate([b[1], b[2]])).min() >= 60


@pytest.mark.parametrize("d", [32, 256])
def test_a_grouped_batch_and_distinct_users_take_the_other_paths(dev, d):
    """The two flags of pda_adam_step_f32: a batch grouped by positive without PDA_UPD_ANY_ORDER (runs of equal positives are combined), and
    PDA_UPD_USERS_DISTINCT (the user rows take plain stores).  Same gradients."""
    rng = np.random.default_rng(7 * d)
    U, I = tables(rng, d)
    ipw = ips_weights(COUNTS, 4.0)[1]
    users, pos, neg = batch(rng, 300)
    order = np.argsort(pos, kind="stable")
    b = (users[order], pos[order], neg[order])
    for norm in (False, True):
        ref = ips_grads(U, I, *b, ipw, norm=norm, regs=REGS, reg_div=300)
        check(run_grads(dev, U, I, b, ipw, norm, 300, grouped=True)[:3], ref, tolerance(ipw, b[1], norm), "grouped d=%d" % d)
    b = (rng.permutation(NU).astype(np.int32),) + batch(rng, NU)[1:]
    ref = ips_grads(U, I, *b, ipw, norm=True, regs=REGS, reg_div=NU)
    for grouped in (False, True):       # (an ungrouped batch under the grouped rule: equal positives apart are separate atomics, still the same sum)
        check(run_grads(dev, U, I, b, ipw, True, NU, users_distinct=True, grouped=grouped)[:3], ref, TOL, "distinct users d=%d" % d)


@pytest.mark.parametrize("B", [7, 2048])
@pytest.mark.parametrize("d", DIMS)
def test_all_weights_one_is_the_plain_bpr_step(dev, d, B):
    from pda_amd import ops
    U, I, b, _, _ = parity_case(d, B, "plain")
    loss, gU, gI, _ = run_grads(dev, U, I, b, np.ones(NI, dtype=np.float32), False, B)
    Ut, It, ut, pt, nt = to(dev, U, I, *b)
    hU, hI, hl = torch.zeros_like(Ut), torch.zeros_like(It), torch.zeros(3, device=dev)
    ops.bpr_step(Ut, It, ut, pt, nt, regs=REGS, reg_div=B, mode=ops.UPD_DENSE_GRAD, gU=hU, gI=hI, loss_acc=hl)
    check((loss, gU, gI), (hl.cpu().numpy(), hU.cpu().numpy(), hI.cpu().numpy()), TOL, "ipw = 1 against pda_bpr_step_f32, d=%d B=%d" % (d, B))


def test_ops_checks_ids_and_the_kernel_skips_a_triplet_outside_the_tables(dev):
    from pda_amd import ops
    rng = np.random.default_rng(1)
    U, I = tables(rng, 32)
    ipw = ips_weights(COUNTS)[1]
    b = batch(rng, 9)
    Ut, It, ut, pt, nt, wt = to(dev, U, I, *b, ipw)
    st = State(Ut, It)
    kw = dict(regs=REGS, reg_div=9, step=1)
    bad = pt.clone()
    bad[4] = NI
    with pytest.raises(ValueError, match="outside the tables"):
        ops.ips_grads(Ut, It, ut, bad, nt, wt, st.gU, st.gI, st.tagU, st.tagI, **kw)
    with pytest.raises(TypeError, match="ipw"):
        ops.ips_grads(Ut, It, ut, pt, nt, wt.double(), st.gU, st.gI, st.tagU, st.tagI, **kw)
    with pytest.raises(ValueError, match="one float32 per item"):
        ops.ips_grads(Ut, It, ut, pt, nt, wt[:-1].contiguous(), st.gU, st.gI, st.tagU, st.tagI, **kw)
    with pytest.raises(ValueError, match="embedding width"):
        ops.ips_grads(Ut[:, :24].contiguous(), It[:, :24].contiguous(), ut, pt, nt, wt, st.gU, st.gI, st.tagU, st.tagI, **kw)
    assert float(st.gU.abs().max()) == 0.0 and int(st.tagU.abs().max()) == 0           # nothing was launched
    # the kernel skips a triplet with an id outside the tables (memory safety when the host check is off): the other eight still count --
    # with the mean over B = 9 when unnormalised, and with S over the eight when normalised
    keep = np.arange(9) != 4
    b8 = [x[keep] for x in b]
    for norm in (False, True):
        st = State(Ut, It)
        loss = torch.zeros(3, device=dev)
        ops.ips_grads(Ut, It, ut, bad, nt, wt, st.gU, st.gI, st.tagU, st.tagI, wsum=st.wsum if norm else None, loss_acc=loss, check_ids=False, **kw)
        terms, rU, rI = ips_grads(U, I, *b8, ipw, norm=norm, regs=REGS, reg_div=9, B=9)
        check((loss.cpu().numpy(), st.gU.cpu().numpy(), st.gI.cpu().numpy()), (terms, rU, rI), tolerance(ipw, b8[1], norm), "one skipped, norm=%d" % norm)
        if norm:
            assert float(st.wsum) == float(ipw[b8[1]].astype(np.float64).sum()) != float(ipw[b[1]].astype(np.float64).sum())
    for bad_ids in ((torch.full_like(ut, -1), pt, nt), (ut, pt, torch.full_like(nt, NI))):        # every triplet skipped: S = 0, nothing moves
        st = State(Ut, It)
        loss = torch.zeros(3, device=dev)
        ops.ips_grads(Ut, It, *bad_ids, wt, st.gU, st.gI, st.tagU, st.tagI, wsum=st.wsum, loss_acc=loss, check_ids=False, **kw)
        assert float(st.wsum) == 0.0 and float(loss.abs().max()) == 0.0 and float(st.gU.abs().max()) == 0.0 and float(st.gI.abs().max()) == 0.0


@pytest.mark.parametrize("d", [32, 256])
def test_a_refused_triplet_inside_a_run_of_equal_positives(dev, d):
    """The contract of the shared scatter of the positives' gradients (pos_scatter_any / pos_run_head / pos_scatter_run, pda_train_common.h) where
    its callers differ: a workgroup holds TPB = 512 / (d / 4) triplets, the batch TPB + 3 (the run crosses a workgroup boundary, the last workgroup
    is mostly empty), every positive is the same item, and two triplets are refused by the kernel -- triplet 2 (pos = n_items) inside the run of
    the first workgroup, triplet TPB (users = -1) at the head of the second.  Under either rule the batch equals the kept triplets with the
    means over the whole B, and the tags are set on exactly the kept triplets' rows."""
    from pda_amd import ops
    TPB = 512 // (d // 4)
    B = TPB + 3
    rng = np.random.default_rng(11 * d)
    U, I = tables(rng, d)
    ipw = ips_weights(COUNTS, 4.0)[1]
    users, pos, neg = batch(rng, B)
    pos[:] = 7
    pos[2], users[TPB] = NI, -1
    keep = ~np.isin(np.arange(B), [2, TPB])
    kept = [x[keep] for x in (users, pos, neg)]
    Ut, It, ut, pt, nt, wt = to(dev, U, I, users, pos, neg, ipw)
    for norm in (False, True):
        ref = ips_grads(U, I, *kept, ipw, norm=norm, regs=REGS, reg_div=B, B=B)
        for grouped in (False, True):
            st = State(Ut, It)
            loss = torch.zeros(3, device=dev)
            ops.ips_grads(Ut, It, ut, pt, nt, wt, st.gU, st.gI, st.tagU, st.tagI, wsum=st.wsum if norm else None, regs=REGS, reg_div=B, step=5,
                          grouped=grouped, loss_acc=loss, check_ids=False)
            check((loss.cpu().numpy(), st.gU.cpu().numpy(), st.gI.cpu().numpy()), ref, tolerance(ipw, kept[1], norm),
                  "refused inside a run d=%d norm=%d grouped=%d" % (d, norm, grouped))
            S_u, S_i = np.unique(kept[0]), np.unique(np.concatenate(kept[1:]))
            tagU, tagI = st.tagU.cpu().numpy(), st.tagI.cpu().numpy()
            assert (np.nonzero(tagU)[0] == S_u).all() and (np.nonzero(tagI)[0] == S_i).all() and set(tagU[S_u]) == {5} and set(tagI[S_i]) == {5}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_three_whole_steps_against_the_restatement(dev, variant):
    from pda_amd import ops
    d, B, lr = 32, 64, 1e-2
    rng = np.random.default_rng(33)
    U, I = tables(rng, d)
    v = VARIANTS[variant]
    ipw = ips_weights(COUNTS, v["clip"])[1]
    Ut, It, wt = to(dev, U, I, ipw)
    st = State(Ut, It)
    Ur, Ir, state = U.astype(np.float64), I.astype(np.float64), None
    for t in (1, 2, 3):
        b = batch(rng, B)
        Ur, Ir, state, terms = ips_adam(Ur, Ir, state, t, lr, *b, ipw, norm=v["norm"], regs=REGS, reg_div=B)
        loss = torch.zeros(3, device=dev)
        ops.ips_adam_step(*st.adam(Ut, It), *to(dev, *b), wt, wsum=st.wsum if v["norm"] else None, regs=REGS, reg_div=B, step=t,
                          lr_t=ops.adam_lr_t(lr, t), loss_acc=loss, check_ids=True)
        np.testing.assert_allclose(loss.cpu().numpy(), terms, atol=tolerance(ipw, b[1], v["norm"]), rtol=0)
        assert float(st.gU.abs().max()) == 0.0 and float(st.gI.abs().max()) == 0.0
    got = dict(U=Ut, I=It, mU=st.mU, vU=st.vU, mI=st.mI, vI=st.vI)
    ref = dict(U=Ur, I=Ir, **state)
    for k in got:
        print("ips three steps (%s): max |%s err| %.3g" % (variant, k, np.abs(got[k].cpu().numpy() - ref[k]).max()))
    for k in got:
        np.testing.assert_allclose(got[k].cpu().numpy(), ref[k], atol=TOL, rtol=0, err_msg=k)


@pytest.mark.parametrize("norm", [False, True])
def test_untouched_rows_take_the_dense_decay_of_the_bpr_step(dev, norm):
    """After one pda_ips_adam_step_f32 the rows outside the batch equal, bit for bit, the idle rows of pda_adam_step_f32 on the same tables (the
    same sweep kernel, g = 0), and both gradient tables are zero again."""
    from pda_amd import ops
    d, B, lr_t = 32, 16, 3e-3
    rng = np.random.default_rng(21)
    U, I = tables(rng, d, 300, 200)
    mom = [np.abs(rng.standard_normal(x.shape)).astype(np.float32) * 1e-3 for x in (U, U, I, I)]
    b = batch(rng, B, 300, 200)
    ipw = ips_weights(rng.integers(0, 50, 200))[1]
    Ut, It, ut, pt, nt, wt = to(dev, U, I, *b, ipw)
    st = State(Ut, It)
    for t, m in zip((st.mU, st.vU, st.mI, st.vI), mom):
        t.copy_(torch.from_numpy(m))
    ops.ips_adam_step(*st.adam(Ut, It), ut, pt, nt, wt, wsum=st.wsum if norm else None, regs=REGS, reg_div=B, step=1, lr_t=lr_t)
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
    assert float(st.gU.abs().max()) == 0.0 and float(st.gI.abs().max()) == 0.0
    assert torch.equal(st.tagU, tagU) and torch.equal(st.tagI, tagI)


def test_the_weight_sum_keeps_its_bits_and_is_within_an_ulp(dev):
    from pda_amd import ops
    B = 2048
    rng = np.random.default_rng(9)
    ipw = ips_weights(rng.integers(0, 1000, NI))[1]                    # arbitrary float32 weights: their float32 sums do round
    b = batch(rng, B)
    ut, pt, nt, wt = to(dev, *b, ipw)
    exact = ipw[b[1]].astype(np.float64).sum()
    one, two = ops.ips_weight_sum(wt, ut, pt, nt, NU), ops.ips_weight_sum(wt, ut, pt, nt, NU)
    assert torch.equal(one.view(torch.int32), two.view(torch.int32))
    got = float(one)
    print("ips weight sum: %.9g against %.17g (%.3g ulp)" % (got, exact, abs(got - exact) / np.spacing(np.float32(exact))))
    assert abs(got - exact) <= np.spacing(np.float32(exact))
    for n in (1, 7, 1023, 1025):                                       # fewer triplets than threads, and one past a stride
        s = ops.ips_weight_sum(wt, ut[:n].contiguous(), pt[:n].contiguous(), nt[:n].contiguous(), NU)
        ex = ipw[b[1][:n]].astype(np.float64).sum()
        assert abs(float(s) - ex) <= np.spacing(np.float32(ex))


@pytest.mark.parametrize("norm", [False, True])
def test_the_step_replays_from_a_captured_graph(dev, norm):
    """pda_ips_adam_step_f32 reads nothing back on the host -- the weight sum stays in device memory: two steps (tags 1 and 2) captured once
    and replayed give the tables of the same two steps launched directly."""
    from pda_amd import ops
    d, B = 64, 200
    rng = np.random.default_rng(5)
    U, I = tables(rng, d)
    bt = to(dev, *batch(rng, B), ips_weights(COUNTS, 4.0)[1])

    def two_steps(Ut, It, st, loss):
        for t in (1, 2):
            ops.ips_adam_step(*st.adam(Ut, It), *bt, wsum=st.wsum if norm else None, regs=REGS, reg_div=B, step=t, lr_t=ops.adam_lr_t(1e-2, t),
                              loss_acc=loss)
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
    assert not norm or float(sb.wsum) == float(sa.wsum) > 0


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------------
def test_cli_trains_ips_and_export_topk_restores_it(dev, tmp_path):
    """python -m pda_amd.train_new_api --train ips --test ips --ips_clip 8 --ips_norm 1 in a child process, two epochs on the smallest synthetic
    dataset: it ends, prints the result lines, writes a BPRMF-format best_ckpt.ckpt, lowers mf_loss, and export_topk restores the checkpoint --
    by --train ips, and, the file copied into a --train normal directory, as the BPRMF it is."""
    import re
    import shutil
    from pda_amd import synthetic
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    synthetic.write_dataset(str(tmp_path / "data" / "toy"), n_users=200, n_items=150, mean_hist=12)
    argv = ["--data_path", str(tmp_path / "data") + "/", "--dataset", "toy", "--train", "ips", "--test", "ips", "--epoch", "2", "--embed_size", "32",
            "--log_interval", "1", "--batch_size", "128", "--lr", "1e-2", "--regs", "1e-3", "--valid_set", "valid", "--pop_exp", "0.22",
            "--save_dir", str(tmp_path / "ckpt") + "/", "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t", "--cuda", "0", "--eval_block", "128",
            "--ips_clip", "8", "--ips_norm", "1"]
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "pda_amd.train_new_api"] + argv, cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert "running IPS" in out and "recall=[" in out and "---- IPS result:" in out and "training and testing end!!!!" in out
    assert "best expo" not in out                                     # --test ips: the main_branch head alone, no gamma search
    mf = [float(m.group(1)) for m in re.finditer(r"Epoch \d+ \[[^\]]*\]: train==\[[-\d.]+=([-\d.]+) \+ [-\d.]+\]", out)]
    assert len(mf) == 2 and mf[1] < mf[0] < 0.75, mf                  # self-normalised: a weighted MEAN of -log sigmoid, log 2 at the start
    ck = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path / "ckpt") for f in fs]
    best = [f for f in ck if f.endswith("best_ckpt.ckpt")]
    assert len(best) == 1 and "ips_train_ips" in best[0]
    sd = torch.load(best[0], map_location="cpu")
    assert "model" not in sd and sd["format"] == "pda_amd/2" and sd["embed_size"] == 32 and sd["user_embedding"].shape == (200, 32) and "mU" in sd
    assert (sd["ips_clip"], sd["ips_norm"]) == (8.0, 1)
    from pda_amd import export_topk
    res = export_topk.main(argv + ["--export_out", str(tmp_path / "lists.npz")])
    assert res["idx"].shape[1] == 50 and res["idx"].shape[0] == len(res["users"]) > 0 and np.isfinite(res["val"]).all()
    # a BPRMF loads the file: the same lists from a --train normal directory
    rel = os.path.relpath(os.path.dirname(best[0]), tmp_path / "ckpt").replace("ips_train_ips", "_train_normal")
    os.makedirs(tmp_path / "ckpt2" / rel)
    shutil.copy(best[0], tmp_path / "ckpt2" / rel / "best_ckpt.ckpt")
    plain = [a if a != "ips" else "normal" for a in argv[:argv.index("--ips_clip")]]
    res2 = export_topk.main(plain + ["--save_dir", str(tmp_path / "ckpt2") + "/", "--export_out", str(tmp_path / "lists2.npz")])
    np.testing.assert_array_equal(res["idx"], res2["idx"])
    np.testing.assert_array_equal(res["val"], res2["val"])
