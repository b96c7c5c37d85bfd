"""GPU suite for iALS++ (`--train ials --ials_solver block`, include/pda_hip_ialspp.h) against the float64 restatement
tests/ialspp_ref.py.  Every tolerance is an a-priori bound derived there (or in tests/ials_ref.py), evaluated on the test's own inputs; the
tests print observed / bound.  Largest observed / bound on MI355X: see DESIGN.md 5v.

Shapes: one side with rows of 0, 1, 31, 32, 33, 300 and 2 * 4096 + 5 pairs (two chunk boundaries) in one shuffled call.  The longest row has
8 197 distinct partners, so the other table has ials_ref.N_OTHER = 8 232 rows (a table of about 600 rows cannot hold that row).
"""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import dirty_buffers as db
import ials_ref as ir
import ialspp_ref as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0, 1, 31, 32, 33, 300, 2 * ir.CHUNK + 5)
NR = len(LENGTHS)
CASES = [(32, 32), (64, 32), (128, 64), (128, 128), (256, 32), (256, 128)]
A0, LAM, NU = ir.PARAMS[0]


def bits(t):
    return t.contiguous().view(torch.int32)


def last_block(d, k):
    return d // k - 1            # a non-first block wherever there is one: p0 > 0


@pytest.fixture(scope="module")
def lengths():
    rows, cols = ir.length_graph(lengths=LENGTHS)
    indptr, indices = ir.csr(rows, cols, NR)
    return rows, cols, indptr, indices


def graph_of(dev, rows, cols, n_rows, n_other, a0=A0, lam=LAM, nu=NU):
    from pda_amd import ops
    return ops.IalsGraph(rows, cols, n_rows, n_other, dev, lam=lam, alpha0=a0, nu=nu)


_TABLES = {}


def tables(kind, d):
    """(Z32 [N_OTHER, d], X32 [NR, d]) of a kind, made once."""
    if (kind, d) not in _TABLES:
        _TABLES[kind, d] = (ir.table(kind, ir.N_OTHER, d), ir.table(kind, NR, d, seed=5))
    return _TABLES[kind, d]


# ---- 1. exact sums -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, k", CASES)
def test_the_block_system_is_exact_bit_for_bit(dev, lengths, d, k):
    """Eighths tables, a dyadic e, alpha0 and lam_row: every entry of (H, g) is exact in fp32 whatever the order (the headroom below 2^24 is
    asserted), so dbg equals the restatement's fp32-order sums AND exact arithmetic bit for bit; a wrong tile, a wrong column offset, a dropped
    tail block or a lost chunk shows as a difference of whole grid units."""
    from pda_amd import ops
    rows, cols, indptr, indices = lengths
    a0, blk = 0.25, last_block(d, k)
    p0 = blk * k
    g = graph_of(dev, rows, cols, NR, ir.N_OTHER, a0, 1.0, 0.0)
    Z32, X32, lam, rng = pr.exact_inputs(d, NR, ir.N_OTHER)
    e32 = (rng.integers(-4, 9, len(indices)) / 4.0).astype(np.float32)
    assert pr.exact_headroom(indptr, indices, Z32, X32, e32, a0, lam, p0, k) < 2 ** 24
    g.user.lam_row = torch.from_numpy(lam).to(dev)
    Z, X, e = (torch.from_numpy(a.copy()).to(dev) for a in (Z32, X32, e32))
    G = ops.ialspp_gram(Z)
    G64 = Z32.astype(np.float64).T @ Z32.astype(np.float64)
    assert np.abs(Z32.astype(np.float64)).T.dot(np.abs(Z32.astype(np.float64))).max() * 64 < 2 ** 24
    assert torch.equal(bits(G), bits(torch.from_numpy(G64.astype(np.float32)).to(dev)))
    G32 = G64.astype(np.float32)
    dbg = torch.full((NR, k * k + k), float("nan"), device=dev)
    work = g.user.sub_list(range(NR), shuffle_seed=1)
    assert work.n_long == 1 and work.n_slots == 3 and work.n_work == NR - 1 + 3
    ops.ialspp_block_pass(g, "user", Z, X, blk, k, G=G, e=e, work=work, dbg=dbg)
    got = dbg.cpu().numpy()
    for r in range(NR):
        H, gg = pr.system32(indptr, indices, None, Z32, G32, X32[r], e32, a0, lam, r, p0, k)
        a, b = indptr[r], indptr[r + 1]
        H64, g64 = pr.block_system(X32[r], e32[a:b], Z32[indices[a:b]], G64, a0, lam[r], p0, k)
        assert np.array_equal(H.astype(np.float64), H64) and np.array_equal(gg.astype(np.float64), g64)
        assert np.array_equal(got[r, :k * k].reshape(k, k).view(np.int32), H.view(np.int32)), (r, LENGTHS[r])
        assert np.array_equal(got[r, k * k:].view(np.int32), gg.view(np.int32)), (r, LENGTHS[r], np.abs(got[r, k * k:] - gg).max())
    assert torch.isfinite(X).all() and torch.isfinite(e).all() and ops.ialspp_buffers(g, d)["fail"].item() == 0


# ---- 2. a pass against float64 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ir.TABLES)
@pytest.mark.parametrize("d, k", CASES)
def test_a_pass_stays_inside_the_a_priori_bound(dev, lengths, d, k, kind):
    """The new x_{r,pi} and e of every listed row lie inside the bound; the row that is not listed, its e, and every coordinate outside the
    block are untouched bit for bit."""
    from pda_amd import ops
    rows, cols, indptr, indices = lengths
    blk = last_block(d, k)
    p0 = blk * k
    g = graph_of(dev, rows, cols, NR, ir.N_OTHER)
    lam_row = ir.lam_row(np.diff(indptr), ir.N_OTHER, LAM, A0, NU)
    np.testing.assert_array_equal(g.user.host_lam_row, lam_row)
    Z32, X32 = tables(kind, d)
    e32 = pr.predictions(X32, Z32, indptr, indices).astype(np.float32)
    listed = [r for r in range(NR) if r != 4]                                               # the row of 33 pairs stays out
    Z, X, e = (torch.from_numpy(a.copy()).to(dev) for a in (Z32, X32, e32))
    ops.ialspp_block_pass(g, "user", Z, X, blk, k, e=e, work=g.user.sub_list(listed, shuffle_seed=2))
    o = pr.pass_bounds(X32, e32, indptr, indices, None, Z32, A0, lam_row, p0, k, rows=listed)
    assert np.isfinite(o["dX"]).all() and np.isfinite(o["de"]).all()
    x, ee = X.cpu().numpy(), e.cpu().numpy()
    assert np.isfinite(x).all() and np.isfinite(ee).all() and ops.ialspp_buffers(g, d)["fail"].item() == 0
    outside = np.ones(d, dtype=bool)
    outside[p0:p0 + k] = False
    assert np.array_equal(x[:, outside].view(np.int32), X32[:, outside].view(np.int32))
    assert np.array_equal(x[4].view(np.int32), X32[4].view(np.int32))
    assert np.array_equal(ee[indptr[4]:indptr[5]].view(np.int32), e32[indptr[4]:indptr[5]].view(np.int32))
    ex = np.linalg.norm(x.astype(np.float64) - o["X"], axis=1)
    ed = np.abs(ee.astype(np.float64) - o["e"])
    print("ialspp pass d=%d k=%d %s: observed / bound max %.3g (x), %.3g (e)" %
          (d, k, kind, np.max(ex[listed] / o["dX"][listed]), np.max(ed / np.maximum(o["de"], 1e-300))))
    assert (ex <= o["dX"]).all(), (ex / np.maximum(o["dX"], 1e-300)).max()
    assert (ed <= o["de"]).all(), (ed / np.maximum(o["de"], 1e-300)).max()
    assert (np.abs(x[listed][:, p0:p0 + k] - X32[listed][:, p0:p0 + k]).max(1) > 0).all()  # (and every listed row did move)


# ---- 3. k = d is the half-sweep ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [32, 128])
def test_a_block_of_all_coordinates_is_the_exact_half_sweep(dev, lengths, d):
    from pda_amd import ops
    rows, cols, indptr, indices = lengths
    g = graph_of(dev, rows, cols, NR, ir.N_OTHER)
    lam_row = g.user.host_lam_row
    Z32, X32 = tables("gauss0.3", d)
    Z = torch.from_numpy(Z32).to(dev)
    want = torch.full((NR, d), float("nan"), device=dev)
    ops.ials_half_sweep(g, "user", Z, want)
    hb = ir.row_bounds(indptr, indices, Z32, A0, lam_row, range(NR))
    for scale in (1.0, 0.0):                                                                # from a random start and from zero
        X0 = (X32 * np.float32(scale)).astype(np.float32)
        true = pr.predictions(X0, Z32, indptr, indices)
        e32 = true.astype(np.float32)                                                       # the cache the kernel reads: the predictions, rounded
        X, e = torch.from_numpy(X0.copy()).to(dev), torch.from_numpy(e32).to(dev)
        ops.ialspp_block_pass(g, "user", Z, X, 0, d, e=e)
        o = pr.pass_bounds(X0, true, indptr, indices, None, Z32, A0, lam_row, 0, d, de=ir.U32 * np.abs(true))
        np.testing.assert_allclose(o["X"], hb["x"], atol=1e-9)                              # (the two restatements agree: k = d is the half-sweep)
        gap = np.linalg.norm(X.cpu().numpy().astype(np.float64) - want.cpu().numpy().astype(np.float64), axis=1)
        allowed = o["dX"] + hb["bound"] * hb["xnorm"] + 1e-9
        print("ialspp k = d = %d from %g x: gap / (both bounds) max %.3g" % (d, scale, (gap / allowed).max()))
        assert np.isfinite(allowed).all() and (gap <= allowed).all()


# ---- 4. the item side: pair_perm and cut rows behind it ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, k", [(64, 32), (256, 128)])
def test_the_item_pass_keeps_the_cache_true_through_pair_perm(dev, lengths, d, k):
    """The lengths graph transposed: 7 items over 8 232 users, so the item side has the cut row and addresses e through a permutation that is
    far from the identity.  After predict and one item pass, e gathered through pair_perm equals the predictions recomputed in float64 from
    the tables the kernel left, within predict_bound + cache_drift_bound; the pass itself lies inside its bound."""
    from pda_amd import ops
    rows, cols, indptr, indices = lengths                                                   # item CSR: rows are items, cols users
    nu, ni = ir.N_OTHER, NR
    g = graph_of(dev, cols, rows, nu, ni)
    np.testing.assert_array_equal(g.item.host["indptr"], indptr)
    np.testing.assert_array_equal(g.item.host["indices"], indices)
    up, ui = g.user.host["indptr"], g.user.host["indices"]
    perm = pr.pair_perm(up, ui, indptr, indices)
    np.testing.assert_array_equal(g.pair_perm.cpu().numpy(), perm)
    assert (perm != np.arange(len(perm))).mean() > 0.9
    X32, Y32 = tables("gauss0.3", d)                                                        # users [8232, d], items [7, d]
    blk = last_block(d, k)
    p0 = blk * k
    X, Y = torch.from_numpy(X32).to(dev), torch.from_numpy(Y32.copy()).to(dev)
    e = ops.ialspp_predict(g, X, Y)
    assert e.data_ptr() == g.e.data_ptr()
    e0 = e.cpu().numpy()
    true0 = pr.predictions(X32, Y32, up, ui)
    de0 = pr.predict_bound(X32, Y32, up, ui)
    assert (np.abs(e0 - true0) <= de0).all()
    ops.ialspp_block_pass(g, "item", X, Y, blk, k)
    o = pr.pass_bounds(Y32, true0, indptr, indices, perm, X32, A0, g.item.host_lam_row, p0, k, de=de0)
    y, e1 = Y.cpu().numpy(), e.cpu().numpy()
    assert np.isfinite(o["dX"]).all() and (np.linalg.norm(y.astype(np.float64) - o["X"], axis=1) <= o["dX"]).all()
    assert (np.abs(e1 - o["e"]) <= o["de"]).all()
    fresh = pr.predictions(X32, y, up, ui)                                                  # from the tables as the kernel left them
    ratio = np.abs(e1 - fresh) / o["drift"]
    print("ialspp item pass d=%d k=%d: cache against float64 predictions, observed / bound max %.3g" % (d, k, ratio.max()))
    assert (np.abs(e1 - fresh) <= o["drift"]).all()
    assert ops.ialspp_buffers(g, d)["fail"].item() == 0


# ---- 5. epochs: the cache, the objective, the loss -------------------------------------------------------------------------------------------------
def toy_pairs(seed=3, nu=70, ni=45, n=2500):
    g = np.random.default_rng(seed)
    return g.integers(0, nu - 1, n), np.minimum(g.zipf(1.4, n) - 1, ni - 2), nu, ni      # the last user and the last item stay without pairs


def make_model(dev, d, k, **over):
    from pda_amd.model_api import IALSMF, gcn_train_pairs
    from pda_amd.parse import parse_args
    args = parse_args(["--train", "ials", "--ials_solver", "block", "--ials_block", str(k), "--embed_size", str(d), "--regs", "0.05", "--verbose", "0"])
    for key, v in over.items():
        setattr(args, key, v)
    u, i, nu, ni = toy_pairs()
    lists = {int(x): [] for x in range(nu)}
    for a, b in zip(u.tolist(), i.tolist()):
        lists[a].append(b)                                                                  # (with duplicates: the graph counts a pair once)
    return IALSMF(args, {"n_users": nu, "n_items": ni, "gcn_train_pairs": gcn_train_pairs(lists)}, device=dev), (u, i, nu, ni)


def m_args(d, **over):
    from pda_amd.parse import parse_args
    args = parse_args(["--embed_size", str(d), "--verbose", "0"])
    for k, v in over.items():
        setattr(args, k, v)
    return args


def toy_csrs(u, i, nu, ni):
    eu, ei = ir.dedup_pairs(u, i, ni)
    up, ui = ir.csr(eu, ei, nu)
    ip, ii = ir.csr(ei, eu, ni)
    return eu, ei, up, ui, ip, ii


@pytest.mark.parametrize("d", [64, 256])
def test_six_epochs_never_raise_the_objective_and_the_cache_stays_true(dev, d):
    """Pass by pass, as ops.ialspp_epoch runs them.  The reference of every pass is the pair of fp32 tables the kernels left, and de bounds
    |cache - x . z|: predict_bound after the predict, cache_drift_bound after every pass.  A pass is the exact minimiser over the block up to
    an error of delta of at most err (step_bounds, with de as the only input error), and the objective is quadratic in the block with Hessian
    H, so the pass may raise the float64 objective by at most sum_r lambda_max(H_r) err_r^2.  After every epoch the cache lies within de +
    predict_bound of a fresh ialspp_predict, and the loss equals the float64 objective within ials_ref.loss_bound."""
    from pda_amd import ops
    k = 32
    m, (u, i, nu, ni) = make_model(dev, d, k)
    eu, ei, up, ui, ip, ii = toy_csrs(u, i, nu, ni)
    g = m.graph
    lu, li = g.user.host_lam_row, g.item.host_lam_row
    perm = g.pair_perm.cpu().numpy()
    X, Y = m.weights["user_embedding"], m.weights["item_embedding"]
    host = lambda: (X.cpu().numpy(), Y.cpu().numpy())                                       # noqa: E731
    obj = lambda: ir.objective(*host(), eu, ei, A0, lu, li)[0]                              # noqa: E731
    last, worst, worst_cache = obj(), -np.inf, 0.0
    for epoch in range(6):
        x32, y32 = host()
        e = ops.ialspp_predict(g, X, Y)
        de = pr.predict_bound(x32, y32, up, ui)
        for blk, p0 in enumerate(g.blocks(d, k)):
            for side in ("user", "item"):
                x32, y32 = host()
                true = pr.predictions(x32, y32, up, ui)
                assert (np.abs(e.cpu().numpy() - true) <= de).all(), (epoch, blk, side)
                if side == "user":
                    o = pr.pass_bounds(x32, true, up, ui, None, y32, A0, lu, p0, k, de=de)
                    ops.ialspp_block_pass(g, "user", Y, X, blk, k)
                else:
                    o = pr.pass_bounds(y32, true, ip, ii, perm, x32, A0, li, p0, k, de=de)
                    ops.ialspp_block_pass(g, "item", X, Y, blk, k)
                allowance = float(np.sum(o["lmax"] * o["err"] ** 2))
                assert np.isfinite(allowance)
                de = o["drift"]
                now = obj()
                worst = max(worst, (now - last) / last)
                assert now <= last + allowance, (epoch, blk, side, now - last, allowance)
                last = now
        x32, y32 = host()
        cached, fresh = e.cpu().numpy().copy(), ops.ialspp_predict(g, X, Y, torch.full_like(e, float("nan"))).cpu().numpy()
        allowed = de + pr.predict_bound(x32, y32, up, ui)
        worst_cache = max(worst_cache, float(np.max(np.abs(cached - fresh) / allowed)))
        assert (np.abs(cached - fresh) <= allowed).all(), epoch
    print("ialspp d=%d: worst relative step of the objective %.3g over %d passes, final %.6g; cache / bound max %.3g" %
          (d, worst, 12 * (d // k), last, worst_cache))
    assert m.failed_pivots().item() == 0 and torch.isfinite(X).all() and torch.isfinite(Y).all()
    got = ops.ialspp_loss(g, X, Y).cpu().numpy()
    x32, y32 = host()
    L, fit, reg = ir.objective(x32, y32, eu, ei, A0, lu, li)
    bound = ir.loss_bound(x32, y32, up, ui, A0, lu, L)
    print("ialspp loss d=%d: |L^ - L| / bound = %.3g" % (d, abs(got[0] - L) / bound))
    assert got.dtype == np.float64 and abs(got[0] - L) <= bound and abs(got[1] - fit) <= bound and abs(got[2] - reg) <= bound
    if d <= 128:
        assert torch.equal(ops.ialspp_loss(g, X, Y), ops.ials_loss(g, X, Y))
        assert torch.equal(bits(ops.ialspp_gram(Y)), bits(ops.ials_gram(Y)))


@pytest.mark.parametrize("d", [32, 128, 256])
def test_the_loss_equals_the_float64_objective_on_the_lengths_graph(dev, lengths, d):
    from pda_amd import ops
    rows, cols, indptr, indices = lengths
    g = graph_of(dev, rows, cols, NR, ir.N_OTHER)
    Y32, X32 = tables("gauss0.3", d)
    got = ops.ialspp_loss(g, torch.from_numpy(X32).to(dev), torch.from_numpy(Y32).to(dev)).cpu().numpy()
    lu, li = g.user.host_lam_row, g.item.host_lam_row
    L, fit, reg = ir.objective(X32, Y32, rows, cols, A0, lu, li)
    bound = ir.loss_bound(X32, Y32, indptr, indices, A0, lu, L)
    print("ialspp loss lengths-%d: |L^ - L| / bound = %.3g" % (d, abs(got[0] - L) / bound))
    assert abs(got[0] - L) <= bound and abs(got[1] - fit) <= bound and abs(got[2] - reg) <= bound


@pytest.mark.parametrize("d, k", [(32, 32), (64, 32), (256, 32)])
def test_one_epoch_of_the_model_is_the_restatement_s_epoch(dev, d, k):
    """train_epoch() gives the bits of predict + the passes in the restatement's order, run one by one; every one of those passes lies within
    pass_bounds of the restatement's pass from the state the kernels left (tables and cache).  At k = d, two passes, the whole epoch is also
    held to the restatement's epoch from the initial tables within epoch_bounds; with more blocks that bound is infinite (ialspp_ref)."""
    from pda_amd import ops
    from pda_amd.model_api import BPRMF
    m, (u, i, nu, ni) = make_model(dev, d, k)
    eu, ei, up, ui, ip, ii = toy_csrs(u, i, nu, ni)
    lu, li = ir.lam_row(np.diff(up), ni, LAM, A0, NU), ir.lam_row(np.diff(ip), nu, LAM, A0, NU)
    np.testing.assert_array_equal(m.graph.user.host_lam_row, lu)
    np.testing.assert_array_equal(m.graph.item.host_lam_row, li)
    ref = BPRMF(m_args(d), {"n_users": nu, "n_items": ni}, device=dev)                      # the usual initialisation: it matters to a block step
    assert torch.equal(ref.weights["user_embedding"], m.weights["user_embedding"]) and torch.equal(ref.weights["item_embedding"], m.weights["item_embedding"])
    X0, Y0 = (m.weights[key].cpu().numpy() for key in ("user_embedding", "item_embedding"))
    out = m.train_epoch()
    assert out.dtype == torch.float64 and out.shape == (3,) and out.is_cuda
    X, Y = (m.weights[key].cpu().numpy() for key in ("user_embedding", "item_embedding"))
    e_model = m.graph.e.cpu().numpy().copy()
    assert np.isfinite(X).all() and np.isfinite(Y).all() and m.failed_pivots().item() == 0
    L, fit, reg = ir.objective(X, Y, eu, ei, A0, lu, li)
    bound = ir.loss_bound(X, Y, up, ui, A0, lu, L)
    got = out.cpu().numpy() * len(eu)
    assert abs(got[0] - L) <= bound and abs(got[1] - fit) <= bound and abs(got[2] - reg) <= bound
    # the same epoch by hand, pass by pass
    g = m.graph
    perm = pr.pair_perm(up, ui, ip, ii)
    X2, Y2 = torch.from_numpy(X0).to(dev), torch.from_numpy(Y0).to(dev)
    e = ops.ialspp_predict(g, X2, Y2)
    assert (np.abs(e.cpu().numpy() - pr.predictions(X0, Y0, up, ui)) <= pr.predict_bound(X0, Y0, up, ui)).all()
    worst = 0.0
    for blk, p0 in enumerate(g.blocks(d, k)):
        for side in ("user", "item"):
            x32, y32, e32 = X2.cpu().numpy(), Y2.cpu().numpy(), e.cpu().numpy().copy()
            if side == "user":
                o = pr.pass_bounds(x32, e32, up, ui, None, y32, A0, lu, p0, k)
                new = ops.ialspp_block_pass(g, "user", Y2, X2, blk, k).cpu().numpy()
            else:
                o = pr.pass_bounds(y32, e32, ip, ii, perm, x32, A0, li, p0, k)
                new = ops.ialspp_block_pass(g, "item", X2, Y2, blk, k).cpu().numpy()
            ex, ed = np.linalg.norm(new - o["X"], axis=1), np.abs(e.cpu().numpy() - o["e"])
            assert np.isfinite(o["dX"]).all() and (ex <= o["dX"]).all() and (ed <= o["de"]).all(), (blk, side)
            worst = max(worst, float(np.max(ex / o["dX"])), float(np.max(ed / np.maximum(o["de"], 1e-300))))
    print("ialspp model epoch d=%d k=%d: observed / bound max %.3g over the passes" % (d, k, worst))
    assert torch.equal(bits(X2), bits(m.weights["user_embedding"])) and torch.equal(bits(Y2), bits(m.weights["item_embedding"]))
    assert np.array_equal(e.cpu().numpy().view(np.int32), e_model.view(np.int32))
    if k == d:
        o = pr.epoch_bounds(X0, Y0, up, ui, ip, ii, A0, lu, li, k)
        X1, Y1, e1 = pr.epoch(X0, Y0, up, ui, ip, ii, A0, lu, li, k)
        np.testing.assert_allclose(o["X"], X1, atol=1e-12)
        np.testing.assert_allclose(o["Y"], Y1, atol=1e-12)
        ex, ey = np.linalg.norm(X - X1, axis=1), np.linalg.norm(Y - Y1, axis=1)
        print("ialspp model epoch d=%d k=%d: observed / bound max %.3g (users), %.3g (items)" % (d, k, np.max(ex / o["dX"]), np.max(ey / o["dY"])))
        assert np.isfinite(o["dY"]).all() and (ex <= o["dX"]).all() and (ey <= o["dY"]).all() and (np.abs(e_model - e1) <= o["de"]).all()
    sd = m.state_dict()
    assert sd.get("model", "mf") == "mf" and not any(key in sd for key in ("mU", "vU", "mI", "vI", "e", "pair_perm"))
    assert sd["ials_solver"] == "block" and sd["ials_block"] == k
    plain = BPRMF(m_args(d, optimizer="sgd"), {"n_users": nu, "n_items": ni}, device=dev)
    plain.load_state_dict(sd)
    assert torch.equal(plain.weights["user_embedding"], m.weights["user_embedding"])
    exact, _ = make_model(dev, 64, 32, ials_solver="exact")
    assert "ials_solver" not in exact.state_dict() and "ials_block" not in exact.state_dict() and "_pp" not in exact.graph.__dict__


# ---- 6. determinism ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, k", [(64, 32), (256, 128)])
def test_bits_do_not_depend_on_the_call(dev, d, k):
    """Two calls are bit-equal; a row solved alone equals the same row solved among the others; a permuted work list gives the same bits."""
    from pda_amd import ops
    n = 40
    rs = np.random.default_rng(4)
    lens = list(LENGTHS) + [int(v) for v in rs.integers(1, 60, n - NR)]
    rows, cols = ir.length_graph(seed=9, lengths=lens)
    indptr, indices = ir.csr(rows, cols, n)
    g = graph_of(dev, rows, cols, n, ir.N_OTHER)
    Z32 = tables("gauss0.3", d)[0]
    X32 = ir.table("gauss0.3", n, d, seed=8)
    e32 = pr.predictions(X32, Z32, indptr, indices).astype(np.float32)
    Z = torch.from_numpy(Z32).to(dev)
    G = ops.ialspp_gram(Z)
    assert torch.equal(bits(G), bits(ops.ialspp_gram(Z))) and torch.equal(bits(G), bits(G.t().contiguous()))
    blk = last_block(d, k)

    def run(work):
        X, e = torch.from_numpy(X32.copy()).to(dev), torch.from_numpy(e32.copy()).to(dev)
        ops.ialspp_block_pass(g, "user", Z, X, blk, k, G=G, e=e, work=work)
        return X, e

    bx, be = run(None)
    assert torch.isfinite(bx).all() and torch.isfinite(be).all()
    for work in (None, g.user.sub_list(range(n), shuffle_seed=1), g.user.sub_list(range(n), shuffle_seed=2)):
        x, e = run(work)
        assert torch.equal(bits(bx), bits(x)) and torch.equal(bits(be), bits(e))
    X0, e0 = torch.from_numpy(X32).to(dev), torch.from_numpy(e32).to(dev)
    for r in (0, 1, 5, NR - 1, n - 1):                                                      # empty, one pair, 300 pairs, three chunks, the last
        x, e = run(g.user.sub_list([r]))
        a, b = int(indptr[r]), int(indptr[r + 1])
        assert torch.equal(bits(x[r]), bits(bx[r])) and torch.equal(bits(e[a:b]), bits(be[a:b])), r
        others = torch.ones(n, dtype=torch.bool, device=dev)
        others[r] = False
        pairs = torch.ones(len(e32), dtype=torch.bool, device=dev)
        pairs[a:b] = False
        assert torch.equal(bits(x[others]), bits(X0[others])) and torch.equal(bits(e[pairs]), bits(e0[pairs]))   # what a call does not list stays
    ea, eb = (ops.ialspp_predict(g, torch.from_numpy(X32).to(dev), Z, torch.full((len(e32),), float("nan"), device=dev)) for _ in range(2))
    assert torch.equal(bits(ea), bits(eb)) and torch.isfinite(ea).all()


# ---- 7. dirty buffers --------------------------------------------------------------------------------------------------------------------------------
def test_no_call_depends_on_what_its_scratch_held(dev, lengths):
    """The Gram workspace, the slots, the delta buffer, the loss rows and G itself hold the 0xFF pattern (NaN) in one run and 0x3F in the other,
    each of exactly the size the header's formulas give; every tensor the calls leave behind is bit-equal between the runs."""
    from pda_amd import ops
    rows, cols, indptr, indices = lengths
    d, k, blk = 256, 32, 7
    g = graph_of(dev, rows, cols, NR, ir.N_OTHER)
    Z32, X32 = tables("gauss0.3", d)
    e32 = pr.predictions(X32, Z32, indptr, indices).astype(np.float32)
    Z = torch.from_numpy(Z32).to(dev)
    n_slots = g.user.all_rows.n_slots
    assert n_slots == 3
    ops.ialspp_buffers(g, d, k)                                                             # (built once, outside: both runs make the same calls)

    def filled(n, fill):
        return torch.full((4 * n,), fill, dtype=torch.uint8, device=dev).view(torch.float32)

    records = {}
    for fill in (0xFF, 0x3F):
        assert fill in db.FILLS
        X, e = torch.from_numpy(X32.copy()).to(dev), torch.from_numpy(e32.copy()).to(dev)
        with db.Recorder(fill) as rec:
            G = ops.ialspp_gram(Z, filled(d * d, fill).view(d, d), filled(-(-ir.N_OTHER // ir.GRAM_ROWS) * (d * d + d), fill))
            ops.ialspp_block_pass(g, "user", Z, X, blk, k, G=G, e=e, slots=filled(n_slots * (k * k + k), fill), delta_ws=filled(n_slots * k, fill))
            Gs = ops.ialspp_gram(Z[:600].contiguous(), filled(d * d, fill).view(d, d), filled(3 * (d * d + d), fill))
            ops.ialspp_predict(g, X, Z, filled(len(e32), fill))
            ops.ialspp_loss(g, X, Z, G=G, rows=filled(NR * 3, fill).view(NR, 3))
            assert torch.isfinite(Gs).all()
        assert torch.isfinite(X).all() and torch.isfinite(e).all()
        records[fill] = rec.records
    assert {"ialspp_gram", "ialspp_block_pass", "ialspp_predict", "ialspp_loss"} <= {n for n, _ in records[0xFF]}
    assert [n for n, _ in records[0xFF]].count("ialspp_gram") == 2
    db.same_records(records[0xFF], records[0x3F], "iALS++ scratch under two fills")


# ---- 8. through the CLI ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from pda_amd import synthetic
    root = tmp_path_factory.mktemp("ialspp_data")
    synthetic.write_dataset(str(root / "toy"), n_users=400, n_items=300, mean_hist=20)
    return str(root) + "/"


def _argv(toy, save, extra=()):
    return ["--data_path", toy, "--dataset", "toy", "--train", "ials", "--test", "normal", "--epoch", "3", "--log_interval", "1", "--embed_size", "256",
            "--regs", "0.05", "--valid_set", "valid", "--pop_exp", "0.22", "--save_dir", save, "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t",
            "--cuda", "0", "--eval_block", "128"] + list(extra)


BLOCK = ("--ials_solver", "block", "--ials_block", "32")


def test_the_cli_trains_checkpoints_restores_and_exports_at_256(dev, toy, tmp_path):
    from pda_amd.model_api import BPRMF
    save = str(tmp_path / "a") + "/"
    r = subprocess.run([sys.executable, "-m", "pda_amd.train_new_api"] + _argv(toy, save, BLOCK), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout
    losses = [[float(x) for x in mm.groups()] for mm in re.finditer(r"Epoch \d+ \[[^\]]*\]: train==\[([-\d.]+)=([-\d.]+) \+ ([-\d.]+)\]", out)]
    assert len(losses) == 3 and np.isfinite(losses).all(), out[-2000:]
    assert losses[0][0] > losses[1][0] > losses[2][0]                                       # the printed loss falls
    assert "recall=[" in out and "running iALS" in out
    found = glob.glob(os.path.join(save, "**", "best_ckpt.ckpt"), recursive=True)
    assert len(found) == 1 and "_train_ials" in found[0] and os.path.basename(os.path.dirname(found[0])).endswith("ials"), found
    sd = torch.load(found[0], map_location="cpu")
    assert sd.get("model", "mf") == "mf" and "mU" not in sd and tuple(sd["user_embedding"].shape) == (400, 256)
    assert sd["ials_solver"] == "block" and sd["ials_block"] == 32
    plain = BPRMF(m_args(256, optimizer="sgd"), {"n_users": 400, "n_items": 300}, device=dev)
    plain.load_state_dict(sd)
    assert torch.equal(plain.weights["item_embedding"].cpu(), sd["item_embedding"]) and torch.isfinite(sd["item_embedding"]).all()
    npz = str(tmp_path / "lists.npz")
    r = subprocess.run([sys.executable, "-m", "pda_amd.export_topk"] + _argv(toy, save, BLOCK + ("--export_out", npz)), cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lists = np.load(npz)
    assert lists["idx"].shape[1] == 50 and lists["idx"].shape[0] == lists["users"].shape[0] > 0 and (lists["idx"] < 300).all()
    # the same command without --ials_solver block: the exact solver still refuses the width
    r = subprocess.run([sys.executable, "-m", "pda_amd.train_new_api"] + _argv(toy, str(tmp_path / "b") + "/"), cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "--embed_size 256" in r.stderr and "NotImplementedError" in r.stderr, r.stderr[-2000:]
