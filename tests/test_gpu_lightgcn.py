"""GPU: the LightGCN backbone (`--model lightgcn`, include/pda_hip_gcn.h) -- the weighted CSR x dense product, its fused forms, the propagation,
the train step stage by stage (every stage fed the GPU's own output of the stage before it, so every bound is a-priori), three whole steps,
--gcn_layers 0 against the matrix-factorisation oracle, graph replay and the CLI.

Bounds: tests/lightgcn_ref.py derives them (the product and its fused forms, the propagation, the Horner backward pass, the regulariser);
tests/train_ref.py bounds the triplet gradient on the final tables.  Tables and moments after three Adam steps are held to the suite's 1e-5.

Every test prints its largest err / bound.  Observed on an MI355X (records, not thresholds): the RECORD below.

RECORD
    product err / bound           0.29 - 0.35 (small), 0.42 - 0.44 (hub), every d; bit-equal to the fp32 emulation of the work list at d = 32
    fused forms                   addend <= 0.43, running sum <= 0.66, both at once <= 0.98 (rows without edges: the bound is the half ulp of
                                  the two additions there); against the unfused composition the same figures
    propagation L = 1, 2, 3       <= 0.43, 0.33, 0.18
    stages (d, B, both heads)     G <= 0.054 (train_ref.bound)   backward <= 0.24   ego gradient <= 0.65 (B = 300)   mf <= 0.036   reg <= 0.038
                                  loss <= 0.037
    three steps                   tables 1.8e-7, m 3.8e-10, v 4.9e-13 against 1e-5; the first step's moments err / bound 0.19 (m), 0.21 (v)
    --gcn_layers 0 against MF     1.4e-7 against 1e-5
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import lightgcn_ref as lr
import train_ref as tr
from oracle import pda_oracle as po

pytestmark = pytest.mark.gpu
_GRAPHS = {}


def to(dev, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


def dgraph(dev, name):
    from pda_amd import ops
    if name not in _GRAPHS:
        c = lr.graph_case(name)
        _GRAPHS[name] = ops.GcnGraph(*c["pairs"], c["n_users"], c["n_items"], dev)
    return _GRAPHS[name]


def ratio(got, ref, bound):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(bound, 1e-300)).max())


def report(what, **ratios):
    print("lightgcn %s: " % what + "  ".join("%s err/bound %.3g" % kv for kv in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (what, k, v)


# ---- the product -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", lr.DIMS)
@pytest.mark.parametrize("name", lr.GRAPHS)
def test_product_against_float64_within_the_bound_and_bit_stable(dev, name, d):
    """Y = A X element for element.  small: rows of degree 0 and 1, the last row non-empty, 501 entries (no multiple of a workgroup's share);
    hub: item rows of exactly chunk - 1, chunk, chunk + 1 and more than 4 chunk edges (one entry, one, two chunks, five)."""
    from pda_amd import ops
    g, c = dgraph(dev, name), lr.graph_case(name)
    X = lr.table(name, d)
    Xt, = to(dev, X)
    Y, _ = ops.gcn_spmm(g, Xt)
    ref = c["g"]["A"] @ X.astype(np.float64)
    report("product %s d=%d" % (name, d), Y=ratio(Y, ref, lr.product_bound(c["g"], X)))
    assert np.abs(ref).max() > 0.1 and (Y[np.flatnonzero(c["g"]["deg"] == 0)] == 0).all()
    Y2, _ = ops.gcn_spmm(g, Xt)
    assert torch.equal(Y, Y2)
    # the kernel's order, bit for bit: the emulation of tests/lightgcn_ref.py on the same work list (the products round once each: no contraction)
    if d == 32:
        assert np.array_equal(lr.emulate_spmm(g.host, X)[0], Y.cpu().numpy())


@pytest.mark.parametrize("d", lr.DIMS)
@pytest.mark.parametrize("name", lr.GRAPHS)
def test_fused_forms_equal_their_unfused_composition(dev, name, d):
    """The addend (the Horner step), the running sum (read and written by the row's owner, in place too) and the scale, each against float64 under
    the bound of the fused launch, and against the composition of the plain product's own output with torch, under the same bound."""
    from pda_amd import ops
    g, c = dgraph(dev, name), lr.graph_case(name)
    X, add, S = lr.table(name, d), lr.table(name, d, seed=2), lr.table(name, d, seed=3)
    Xt, at, St = to(dev, X, add, S)
    y = c["g"]["A"] @ X.astype(np.float64)
    plain = ops.gcn_spmm(g, Xt)[0].cpu().numpy().astype(np.float64)
    out = {}
    # Y = scale (add + A X)
    b, _ = lr.fused_bound(c["g"], X, add=add, scale=0.25)
    Y, _ = ops.gcn_spmm(g, Xt, add=at, scale=0.25)
    out["addend"], out["addend_vs_unfused"] = ratio(Y, 0.25 * (add + y), b), ratio(Y, 0.25 * (add + plain), b)
    # Y = A X and sum_out = scale (sum_in + Y)
    by, bs = lr.fused_bound(c["g"], X, sum_in=S, scale=1.0 / 3)
    Y, So = ops.gcn_spmm(g, Xt, Y=torch.empty_like(Xt), sum_in=St, sum_out=torch.empty_like(Xt), scale=1.0 / 3)
    out["sum_Y"], out["sum"], out["sum_vs_unfused"] = ratio(Y, y, by), ratio(So, (S + y) / 3, bs), ratio(So, (S + plain) / 3, bs)
    assert np.array_equal(Y.cpu().numpy().astype(np.float64), plain)
    # the same in place and without Y; with the addend on top
    S2 = St.clone()
    _, So2 = ops.gcn_spmm(g, Xt, sum_in=S2, sum_out=S2, scale=1.0 / 3)
    assert So2 is S2 and torch.equal(S2, So)
    _, So3 = ops.gcn_spmm(g, Xt, add=at, sum_in=St, sum_out=torch.empty_like(Xt))
    p = lr.fused_bound(c["g"], X, add=add)[0]
    total = S.astype(np.float64) + add + y
    out["addend_and_sum"] = ratio(So3, total, p + lr.U32 * (np.abs(total) + p))
    report("fused forms %s d=%d" % (name, d), **out)
    assert torch.equal(St.cpu(), torch.from_numpy(S)) and torch.equal(at.cpu(), torch.from_numpy(add))       # inputs untouched


# ---- the propagation ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [0, 1, 2, 3])
@pytest.mark.parametrize("name, d", [("small", 64), ("hub", 64), ("small", 256), ("hub", 32)])
def test_propagation_within_the_bound(dev, name, d, L):
    from pda_amd import ops
    g, c = dgraph(dev, name), lr.graph_case(name)
    nu = c["n_users"]
    E0 = lr.table(name, d)
    Ut, It = to(dev, E0[:nu], E0[nu:])
    F_U, F_I = ops.gcn_propagate(g, Ut, It, L)
    got = torch.cat([F_U, F_I]).cpu().numpy()
    if L == 0:
        assert np.array_equal(got, E0) and F_U.data_ptr() == Ut.data_ptr()
        return
    _, ref = lr.propagate(c["g"]["A"], E0, L)
    report("propagation %s d=%d L=%d" % (name, d, L), F=ratio(got, ref, lr.propagate_bound(c["g"], E0, L)))
    E = torch.from_numpy(E0).to(dev)                         # the model's layout: one buffer, no copy
    F2 = torch.cat(ops.gcn_propagate(g, E[:nu], E[nu:], L)).cpu().numpy()
    assert np.array_equal(F2, got)
    assert np.array_equal(E.cpu().numpy(), E0)


# ---- the step, stage by stage ------------------------------------------------------------------------------------------------------------------
def stage_bounds(mc, pop, F_gpu, L):
    """The triplet stage on the GPU's own final tables: train_ref's case with regs = 0 (the regulariser is not the triplet kernel's here)."""
    b, nu = mc["batch"], mc["n_users"]
    c = tr.Case(F_gpu[:nu], F_gpu[nu:], b["users"], b["pos"], b["neg"], b["pp"], b["pn"], regs=0.0, reg_div=mc["reg_div"])
    due, dpe, dne = tr.reference_grads(c, pop)
    gU, gI = po.dense_grads(nu, mc["n_items"], b["users"], b["pos"], b["neg"], due, dpe, dne)
    bd = tr.bound(c, pop, tables=False)
    fw = po.bpr_forward(c.U, c.I, c.users, c.pos, c.neg, *c.heads(pop))
    return np.concatenate([gU, gI]), np.concatenate([bd["gU"], bd["gI"]]), po.bpr_loss(fw, 0.0, mc["reg_div"])[1], bd["loss"][1]


@pytest.mark.parametrize("pop", [False, True])
@pytest.mark.parametrize("d, B", [(64, 1), (64, 37), (64, 300), (32, 37), (128, 37), (256, 37)])
def test_the_step_stage_by_stage(dev, d, B, pop):
    """Propagate -> G = d mf / dF by ops.bpr_step(regs = 0) -> the backward pass -> the ego-row regulariser, with both heads, hot rows (a third of
    the positives is the hub item) and repeated ids, L = 3 on `small`."""
    from pda_amd import ops
    L, name = 3, "small"
    g, mc = dgraph(dev, name), lr.model_case(name, d, B)
    nu, b, A = mc["n_users"], mc["batch"], mc["g"]["A"]
    E = torch.from_numpy(mc["E0"]).to(dev)
    ut, pt, nt, ppt, pnt = to(dev, b["users"], b["pos"], b["neg"], b["pp"], b["pn"])
    F_U, F_I = ops.gcn_propagate(g, E[:nu], E[nu:], L)
    F_gpu = torch.cat([F_U, F_I]).cpu().numpy()
    G = torch.zeros_like(E)
    loss = torch.zeros(3, device=dev)
    ops.bpr_step(F_U, F_I, ut, pt, nt, ppt if pop else None, pnt if pop else None, regs=0.0, reg_div=B, mode=ops.UPD_DENSE_GRAD, gU=G[:nu], gI=G[nu:],
                 loss_acc=loss)
    G_ref, G_bound, mf_ref, mf_bound = stage_bounds(mc, pop, F_gpu, L)
    G_gpu = G.cpu().numpy()
    H_U, H_I = ops.gcn_backward(g, G[:nu], G[nu:], L)
    H_gpu = torch.cat([H_U, H_I]).cpu().numpy()
    _, H_ref = lr.backward(A, G_gpu, L)
    H_bound = lr.backward_bound(mc["g"], G_gpu, L)
    ops.gcn_reg(E[:nu], E[nu:], ut, pt, nt, H_U, H_I, regs=mc["regs"], reg_div=B, loss_acc=loss)
    add, occ, reg_ref = lr.reg_terms(mc["E0"], nu, b["users"], b["pos"], b["neg"], mc["regs"], B)
    d_g, d_reg = lr.reg_bound(mc["E0"], nu, b["users"], b["pos"], b["neg"], mc["regs"], B, H_ref)
    grad = torch.cat([H_U, H_I]).cpu().numpy()
    got = loss.cpu().numpy().astype(np.float64)
    n_wg = -(-B // tr.tpb(d)) + 2
    d_loss = mf_bound + d_reg + tr.g_(2 * n_wg + 2) * (abs(mf_ref) + reg_ref)
    report("stages d=%d B=%d pop=%s" % (d, B, pop), G=ratio(G_gpu, G_ref, G_bound), backward=ratio(H_gpu, H_ref, H_bound),
           ego_gradient=ratio(grad, H_ref + add, H_bound + d_g), mf=abs(got[1] - mf_ref) / mf_bound, reg=abs(got[2] - reg_ref) / d_reg,
           loss=abs(got[0] - (mf_ref + reg_ref)) / d_loss)
    assert np.abs(G_ref).max() > 1e-4 and np.abs(add).max() > 1e-6 and (B < 37 or occ.max() >= 10)
    # the regulariser does not propagate and sits on the ego rows: exactly the rows of the batch moved, by c x the EGO row
    moved = np.flatnonzero(np.abs(grad - H_gpu).max(1) > 0)
    assert set(moved) <= set(np.flatnonzero(occ)) and np.allclose((grad - H_gpu)[moved], add[moved], rtol=1e-3, atol=1e-9)


def test_the_regulariser_skips_ids_outside_the_tables(dev):
    from pda_amd import ops
    mc = lr.model_case("small", 32, 37)
    nu, b = mc["n_users"], mc["batch"]
    E = torch.from_numpy(mc["E0"]).to(dev)
    users, pos, neg = b["users"].copy(), b["pos"].copy(), b["neg"].copy()
    users[3], pos[7], neg[11] = -1, mc["n_items"], 2 ** 31 - 1
    keep = np.ones(37, bool)
    keep[[3, 7, 11]] = False
    out = []
    for u, p, n in ((users, pos, neg), (users[keep], pos[keep], neg[keep])):
        H, loss = torch.zeros_like(E), torch.zeros(3, device=dev)
        ops.gcn_reg(E[:nu], E[nu:], *to(dev, u, p, n), H[:nu], H[nu:], regs=1e-2, reg_div=37, loss_acc=loss)
        out.append((H.cpu().numpy(), loss.cpu().numpy()))
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(out[0][1], out[1][1], rtol=1e-5, atol=0)
    assert out[0][1][1] == 0 and out[0][1][0] == out[0][1][2] > 0


# ---- whole steps -------------------------------------------------------------------------------------------------------------------------------
def make_model(dev, mc, L, pop, lr_, B, d):
    from pda_amd.model_api import ConditionalLightGCN, LightGCN
    from pda_amd.parse import parse_args
    argv = ["--model", "lightgcn", "--embed_size", str(d), "--batch_size", str(B), "--gcn_layers", str(L), "--lr", str(lr_), "--regs", str(mc["regs"]),
            "--verbose", "0"] + (["--train", "s_condition", "--test", "s_condition"] if pop else [])
    cfg = {"n_users": mc["n_users"], "n_items": mc["n_items"], "gcn_train_pairs": mc["pairs"]}
    m = (ConditionalLightGCN if pop else LightGCN)(parse_args(argv), cfg, device=dev)
    m._E0.copy_(torch.from_numpy(mc["E0"]))
    return m


def batches(dev, name, d, B, n=3):
    bs = [lr.model_case(name, d, B, seed=s)["batch"] for s in range(n)]
    return bs, [to(dev, b["users"], b["pos"], b["neg"], b["pp"], b["pn"]) for b in bs]


@pytest.mark.parametrize("pop", [False, True])
@pytest.mark.parametrize("d, L", [(64, 3), (32, 2)])
def test_three_whole_steps_against_the_reference(dev, d, L, pop):
    """LightGCN.train_step three times against three float64 steps: tables, moments and losses at the suite's 1e-5; the first step's moments
    within the bound of the gradient that made them -- the triplet gradient's bound on the GPU's own final tables carried through
    (1 / (L + 1)) sum_k |A|^k, plus the backward pass's and the regulariser's own rounding -- as tests/test_gpu_bpr_step.py holds its first step."""
    name, B, lr_ = "small", 101, 1e-3
    mc = lr.model_case(name, d, B)
    nu = mc["n_users"]
    m = make_model(dev, mc, L, pop, lr_, B, d)
    bs, bt = batches(dev, name, d, B)
    E_ref, m_ref, v_ref, loss_ref = lr.train_steps(mc, L, pop, lr_, 3, bs)
    worst = {}
    for t in range(3):
        row = m.train_step(*bt[t])
        st = m._opt_state()
        if t == 0:
            F_gpu = m.graph.buffers(d)["F"].cpu().numpy()
            G_ref, G_bound, _, _ = stage_bounds(dict(mc, batch=bs[0]), pop, F_gpu, L)
            _, R = lr.backward(mc["g"]["A"], G_ref, L)
            _, carried = lr.backward(np.abs(mc["g"]["A"]), G_bound, L)
            b0 = bs[0]
            add, _, _ = lr.reg_terms(mc["E0"], nu, b0["users"], b0["pos"], b0["neg"], mc["regs"], B)
            d_g = carried + lr.backward_bound(mc["g"], G_ref, L) + lr.reg_bound(mc["E0"], nu, b0["users"], b0["pos"], b0["neg"], mc["regs"], B, R)[0]
            g1 = np.abs(R + add)
            d_m = 0.1 * d_g + tr.g_(10) * 0.1 * g1
            d_v = 0.001 * (2 * g1 * d_g + d_g ** 2) + tr.g_(1001) * 0.001 * g1 * g1
            mg, vg = (torch.cat([st[a + "U"], st[a + "I"]]).cpu().numpy() for a in "mv")
            live = g1 > 0
            worst["first_m"], worst["first_v"] = ratio(mg[live], 0.1 * (R + add)[live], d_m[live]), ratio(vg[live], 0.001 * (g1 * g1)[live], d_v[live])
            assert (mg[~live] == 0).all() and (vg[~live] == 0).all() and live.mean() > 0.5
        np.testing.assert_allclose(row.cpu().numpy(), loss_ref[t], atol=1e-5, rtol=0)
        for got, ref, what in ((m._E0, E_ref[t], "tables"), (torch.cat([st["mU"], st["mI"]]), m_ref[t], "m"), (torch.cat([st["vU"], st["vI"]]), v_ref[t], "v")):
            err = float(np.abs(got.cpu().numpy() - ref).max())
            worst[what] = max(worst.get(what, 0.0), err)
            assert err <= 1e-5, (what, t, err)
    print("lightgcn three steps d=%d L=%d pop=%s: " % (d, L, pop) + "  ".join("%s %.3g" % kv for kv in worst.items()))
    assert worst["first_m"] <= 1.0 and worst["first_v"] <= 1.0
    assert float(np.abs(E_ref[2] - mc["E0"]).max()) > 2e-3 and m._t == 3                    # the tables moved, far above the tolerance
    F = torch.cat(m.score_tables()).cpu().numpy()                                            # the final tables of the updated ego tables
    np.testing.assert_allclose(F, lr.propagate(mc["g"]["A"], E_ref[2], L)[1], atol=1e-5, rtol=0)
    assert m.score_tables()[0] is m.score_tables()[0]                                        # cached until a step runs


def test_zero_layers_is_matrix_factorisation_by_the_oracle(dev):
    """--gcn_layers 0 through the new path (propagate: nothing; bpr_step at regs = 0; backward: nothing; gcn_reg; the dense sweep) against
    oracle.pda_oracle.train_step(..., "adam") over three steps, with both heads."""
    name, d, B, lr_ = "small", 64, 101, 1e-3
    mc = lr.model_case(name, d, B)
    nu = mc["n_users"]
    bs, bt = batches(dev, name, d, B)
    for pop in (False, True):
        m = make_model(dev, mc, 0, pop, lr_, B, d)
        U, I, state = mc["E0"][:nu].astype(np.float64), mc["E0"][nu:].astype(np.float64), None
        worst = 0.0
        for t in range(3):
            b = bs[t]
            row = m.train_step(*bt[t])
            U, I, state, losses = po.train_step(U, I, b["users"], b["pos"], b["neg"], b["pp"] if pop else None, b["pn"] if pop else None, mc["regs"], B, lr_,
                                                optimizer="adam", state=state, t=t + 1)
            st = m._opt_state()
            for got, ref in ((m.weights["user_embedding"], U), (m.weights["item_embedding"], I), (st["mU"], state["mU"]), (st["vI"], state["vI"])):
                err = float(np.abs(got.cpu().numpy() - ref).max())
                worst = max(worst, err)
                assert err <= 1e-5
            np.testing.assert_allclose(row.cpu().numpy(), losses, atol=1e-5, rtol=0)
        print("lightgcn L=0 against the MF oracle, pop=%s: max err %.3g" % (pop, worst))
        assert float(np.abs(U - mc["E0"][:nu]).max()) > 2e-3


def test_two_steps_replay_from_a_captured_graph(dev):
    """train_step reads nothing back on the host: two steps captured in one torch.cuda.graph (a linear graph: no parallel branches) and replayed give
    the tables, moments and losses of the same two steps launched directly."""
    name, d, B, L = "small", 64, 101, 2
    mc = lr.model_case(name, d, B)
    _, bt = batches(dev, name, d, B, n=2)
    a, b = (make_model(dev, mc, L, True, 1e-3, B, d) for _ in range(2))
    a.start_loss_rows(2)
    for t in range(2):
        a.train_step(*bt[t])
    la = a._loss_rows.clone()
    b._opt_state()                                           # everything a step allocates, before the capture
    b._G = torch.zeros_like(b._E0)
    b.graph.buffers(d)
    b.start_loss_rows(2)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for t in range(2):
                b.train_step(*bt[t])
    torch.cuda.synchronize()
    assert np.array_equal(b._E0.cpu().numpy(), mc["E0"])    # capturing runs nothing
    g.replay()
    torch.cuda.synchronize()
    torch.testing.assert_close(b._E0, a._E0, atol=2e-6, rtol=0)
    for k in ("mU", "vU", "mI", "vI"):
        torch.testing.assert_close(b._state[k], a._state[k], atol=2e-6, rtol=0)
    torch.testing.assert_close(b._loss_rows, la, atol=1e-5, rtol=0)
    assert not np.array_equal(b._E0.cpu().numpy(), mc["E0"])


# ---- through the CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_trains_pda_on_lightgcn_and_the_checkpoint_restores(dev, tmp_path):
    """python -m pda_amd.train_new_api --model lightgcn --train s_condition --test s_condition --gcn_layers 2 in a child process, two epochs on the
    smallest synthetic dataset: the loss falls, the lists of an evaluation are torch.topk of the masked dense scores of score_tables(), a checkpoint
    round trip reproduces the metrics exactly, and a refused combination exits with its message."""
    from pda_amd import synthetic
    from pda_amd import train_new_api as t
    from pda_amd.load_data import get_popularity_from_load, load_popularity
    from pda_amd.model_api import BPRMF, ConditionalLightGCN, gcn_train_pairs
    from pda_amd.sampler import DeviceSampler
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    synthetic.write_dataset(str(tmp_path / "data" / "toy"), n_users=200, n_items=150, mean_hist=12)
    argv = ["--data_path", str(tmp_path / "data") + "/", "--dataset", "toy", "--model", "lightgcn", "--gcn_layers", "2", "--train", "s_condition",
            "--test", "s_condition", "--epoch", "2", "--embed_size", "64", "--log_interval", "1", "--batch_size", "128", "--lr", "1e-2", "--regs", "1e-3",
            "--valid_set", "valid", "--pop_exp", "0.22", "--save_dir", str(tmp_path / "ckpt") + "/", "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t",
            "--cuda", "0", "--eval_block", "128"]
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "pda_amd.train_new_api"] + argv, cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert "running PD & PDA model" in out and "recall=[" in out and "training and testing end!!!!" in out
    losses = [[float(x) for x in m.groups()] for m in re.finditer(r"Epoch \d+ \[[^\]]*\]: train==\[([-\d.]+)=([-\d.]+) \+ ([-\d.]+)\]", out)]
    assert len(losses) == 2 and np.isfinite(losses).all() and losses[1][0] < losses[0][0] and losses[0][2] > 0, losses
    bad = subprocess.run([sys.executable, "-m", "pda_amd.train_new_api"] + argv + ["--optimizer", "sgd"], cwd=root, env=env, capture_output=True, text=True,
                         timeout=300)
    assert bad.returncode != 0 and "NotImplementedError: --model lightgcn --optimizer sgd" in bad.stderr
    ck = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path / "ckpt") for f in fs if f == "best_ckpt.ckpt"]
    assert len(ck) == 1 and "lightgcn_toy_checkpoint" in ck[0]
    sd = torch.load(ck[0], map_location=dev)
    assert (sd["model"], sd["format"], sd["gcn_layers"], sd["embed_size"]) == ("lightgcn", "pda_amd/2", 2, 64) and "mU" in sd and sd["adam_t"] > 0

    t.configure(argv)
    data = t.data
    pop_all = load_popularity(t.args)
    data.add_expo_popularity(np.power(get_popularity_from_load(pop_all), t.args.pop_exp))
    cfg = {"n_users": data.n_users, "n_items": data.n_items, "gcn_train_pairs": gcn_train_pairs(data.train_user_list)}
    with pytest.raises(ValueError, match="checkpoint of a lightgcn model cannot be loaded into BPRMF"):
        BPRMF(t.parse_args(["--embed_size", "64"]), cfg, device=dev).load_state_dict(sd)

    def restored(state):
        model = t.DatasetApi_Model(t.args, cfg, 128, DeviceSampler(data, dev, True), dev)
        assert isinstance(model.Recommender, ConditionalLightGCN)
        model.Recommender.load_state_dict(state)
        ev = t.evaluation(data, [20, 50], dev, block=128)
        ev.set_evaluate_obj_pre("valid")
        ev.set_testing_popularity(None)
        return model, ev, ev.eval(model, None, rec_type="main_branch")

    model, ev, ret = restored(sd)
    # the report of the child process on the same checkpoint ("validation result in best epoch", printed to five decimals)
    m = re.search(r"---- result without pop:\n\|\|-+ recall=\[([\d.]+), ([\d.]+)\]", out)
    assert m and abs(float(m.group(1)) - ret["recall"][0]) < 1e-5 and abs(float(m.group(2)) - ret["recall"][-1]) < 1e-5 and ret["recall"][-1] > 0
    _, _, ret2 = restored(model.Recommender.state_dict())     # the round trip: the same metrics, exactly
    assert all(np.array_equal(ret[k], ret2[k]) for k in ret)
    # the lists: torch.topk of the masked dense scores of score_tables()
    users = np.asarray(list(data.valid_user_list.keys())[:100], dtype=np.int32)
    idx, val = model.recommend_device(users, None, "main_branch", mask=ev._hist)
    dense = torch.from_numpy(model.testing(None, users, list(range(data.n_items)), "main_branch")).to(dev)
    F_U, F_I = model.Recommender.score_tables()
    np.testing.assert_allclose(dense.cpu().numpy(), (F_U[torch.from_numpy(users).long().to(dev)].double() @ F_I.double().T).cpu().numpy(), atol=1e-5, rtol=0)
    assert not torch.equal(F_U, model.Recommender.weights["user_embedding"])                 # the final tables, not the ego tables
    for r_, u in enumerate(users):
        dense[r_, torch.as_tensor(data.train_user_list[int(u)], device=dev, dtype=torch.long)] = -float("inf")
    tv, ti = torch.topk(dense, 50, dim=1)
    assert torch.equal(val, tv) and torch.equal(idx.long(), ti)
