"""GPU suite for item-weighted iALS (`--train ials --ials_item_power`, include/pda_hip_ials_itemw.h) against the float64
restatement tests/ials_itemw_ref.py.  Every tolerance is an a-priori bound derived there (or in tests/ials_ref.py, tests/ialspp_ref.py),
evaluated on the test's own inputs; the tests print observed / bound.  Largest observed / bound on MI355X: see DESIGN.md 5y.

Shapes: the side of tests/test_gpu_ials.py -- ials_ref.ROW_LENGTHS, ten rows from 0 to 2 * 4096 + 5 pairs (two cut rows, five slots) over
ials_ref.N_OTHER = 8 232 columns -- in one shuffled call; "user side" means solved against the scaled Gram matrix G_w with the scalar alpha0,
"item side" solved against the plain G with the row's own alpha_row.
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
import ials_itemw_ref as wr
import ials_ref as ir
import ialspp_ref as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NR = len(ir.ROW_LENGTHS)
A0, LAM, NU = ir.PARAMS[0]
NEW_ENTRY_POINTS = ("pda_ials_gram_scaled_f32", "pda_ialspp_gram256_scaled_f32", "pda_ials_half_sweep_rowalpha_f32", "pda_ialspp_block_pass_rowalpha_f32")


def bits(t):
    return t.contiguous().view(torch.int32)


def to(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev) for a in arrays)


@pytest.fixture(scope="module")
def lengths():
    rows, cols = ir.length_graph()
    indptr, indices = ir.csr(rows, cols, NR)
    return rows, cols, indptr, indices


def graph_of(dev, rows, cols, n_rows, n_other, a0=A0, lam=LAM, nu=NU, **kw):
    from pda_amd import ops
    return ops.IalsGraph(rows, cols, n_rows, n_other, dev, lam=lam, alpha0=a0, nu=nu, **kw)


_TABLES = {}


def tables(kind, d):
    """(Z32 [N_OTHER, d], X32 [NR, d]) of a kind, made once."""
    if (kind, d) not in _TABLES:
        _TABLES[kind, d] = (ir.table(kind, ir.N_OTHER, d), ir.table(kind, NR, d, seed=5))
    return _TABLES[kind, d]


class CountCalls:
    """While active, counts the calls of the given entry points of the loaded library."""

    def __init__(self, names):
        self.names, self.calls, self._saved = names, {n: 0 for n in names}, {}

    def __enter__(self):
        from pda_amd import _lib
        lib = _lib.load()
        for n in self.names:
            fn = self._saved[n] = getattr(lib, n)

            def wrapper(*a, _fn=fn, _n=n):
                self.calls[_n] += 1
                return _fn(*a)
            setattr(lib, n, wrapper)
        return self

    def __exit__(self, *exc):
        from pda_amd import _lib
        for n, fn in self._saved.items():
            setattr(_lib.load(), n, fn)
        return False


# ---- 1. the scaled Gram matrix, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, ir.N_OTHER])
@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_the_scaled_gram_matrix_is_exact_bit_for_bit(dev, d, n):
    """Eighths tables with s in {1/2, 1, 2}: the scaled rows are sixteenths, every sum is exact in fp32 whatever the order, so G_w equals the
    fp32-order restatement AND exact arithmetic bit for bit, and is symmetric; a scale read from the wrong row, a dropped tail block or a row
    scaled twice shows as whole grid units."""
    from pda_amd import ops
    Z32, s32 = ir.eighths_table(n, d, 2), wr.pow2_scale(n)
    Z, s = to(dev, Z32, s32)
    fill = torch.full((d, d), float("nan"), device=dev)
    G = ops.ialspp_gram(Z, fill, scale=s)
    assert G.data_ptr() == fill.data_ptr()
    exact = wr.gram_w(Z32, s32)
    assert np.abs(Z32.astype(np.float64) * s32[:, None]).T.dot(np.abs(Z32.astype(np.float64) * s32[:, None])).max() * 256 < 2 ** 24
    want = wr.gram_scaled32(Z32, s32)
    np.testing.assert_array_equal(want.astype(np.float64), exact)
    assert torch.equal(bits(G), bits(torch.from_numpy(want).to(dev)))
    assert torch.equal(bits(G), bits(G.t().contiguous()))
    if n > 1:
        assert not torch.equal(bits(G), bits(ops.ialspp_gram(Z)))                           # the scale does something
    if d <= 128:
        assert torch.equal(bits(ops.ials_gram(Z, scale=s)), bits(G))                        # the exact solver's binding reaches the same entry point
    Zc = Z.clone()
    ops.ialspp_gram(Z, scale=s)
    assert torch.equal(bits(Z), bits(Zc))                                                   # no scaled copy is written back into the table


# ---- 2. the row systems, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [32, 64, 128])
def test_the_normal_equations_are_exact_bit_for_bit_on_both_sides(dev, lengths, d):
    """The inputs of tests/test_gpu_ials.py's exact test, scaled by s in {1/2, 1, 2} on the user side and with alpha_row in {1/4, 1/2, 1} on the
    item side: every entry of (A_r, b_r) is exact in fp32 (tests/test_ials_itemw_host.py), so dbg_normal equals the restatement's chunk-ordered
    sums bit for bit."""
    from pda_amd import ops
    rows, cols, indptr, indices = lengths
    a0 = 0.25
    g = graph_of(dev, rows, cols, NR, ir.N_OTHER, a0, 1.0, 0.0)
    lam = (np.arange(NR) % 5 * 0.25 + 0.5).astype(np.float32)
    g.user.lam_row = torch.from_numpy(lam).to(dev)
    Z32, s32, al32 = ir.eighths_table(ir.N_OTHER, d, 2), wr.pow2_scale(ir.N_OTHER), wr.pow2_alpha(NR)
    Z, s, al = to(dev, Z32, s32, al32)
    work = g.user.sub_list(range(NR), shuffle_seed=1)
    assert work.n_long == 2 and work.n_slots == 5 and work.n_work == NR - 2 + 5
    Gw32 = wr.gram_w(Z32, s32).astype(np.float32)
    G32 = (Z32.astype(np.float64).T @ Z32.astype(np.float64)).astype(np.float32)
    sides = (("user", ops.ials_gram(Z, scale=s), Gw32, None, lambda r: ir.normal32(indptr, indices, Z32, Gw32, a0, lam, r)),
             ("item", ops.ials_gram(Z), G32, al, lambda r: wr.normal32(indptr, indices, Z32, G32, al32, lam, r)))
    for name, G, want_G, alpha_row, ref in sides:
        assert torch.equal(bits(G), bits(torch.from_numpy(want_G).to(dev))), name
        X = torch.full((NR, d), 7.0, device=dev)
        dbg = torch.full((NR, d * d + d), float("nan"), device=dev)
        ops.ials_half_sweep(g, "user", Z, X, G=G, work=work, dbg_normal=dbg, alpha_row=alpha_row)
        got = dbg.cpu().numpy()
        for r in range(NR):
            A, b = ref(r)
            assert np.array_equal(got[r, :d * d].reshape(d, d).view(np.int32), A.view(np.int32)), (name, r, ir.ROW_LENGTHS[r])
            assert np.array_equal(got[r, d * d:].view(np.int32), b.view(np.int32)), (name, r, ir.ROW_LENGTHS[r])
        x = X.cpu().numpy()
        assert (x[0] == 0).all() and np.isfinite(x).all() and g.buffers(d)["fail"].item() == 0


@pytest.mark.parametrize("d, k", [(64, 32), (256, 128)])
def test_the_block_system_is_bit_for_bit_the_stated_order_on_both_sides(dev, lengths, d, k):
    """(H, g) from dbg against ialspp_ref.system32, which carries out the stated order operation by operation (its fmaf chains are float64
    sums of exact products rounded once: exact emulations at these magnitudes), with G_w for G on the user side and alpha_row[r] for alpha0 on
    the item side.  H is exact whatever the order; g follows the order of the header."""
    from pda_amd import ops
    rows, cols, indptr, indices = lengths
    a0, blk = 0.25, d // k - 1
    p0 = blk * k
    g = graph_of(dev, rows, cols, NR, ir.N_OTHER, a0, 1.0, 0.0)
    Z32, X32, lam, rng = pr.exact_inputs(d, NR, ir.N_OTHER)
    e32 = (rng.integers(-4, 9, len(indices)) / 4.0).astype(np.float32)
    s32, al32 = wr.pow2_scale(ir.N_OTHER), wr.pow2_alpha(NR)
    g.user.lam_row = torch.from_numpy(lam).to(dev)
    Z, s, al = to(dev, Z32, s32, al32)
    work = g.user.sub_list(range(NR), shuffle_seed=1)
    assert work.n_long == 2 and work.n_slots == 5
    Gw32 = wr.gram_w(Z32, s32).astype(np.float32)
    G32 = (Z32.astype(np.float64).T @ Z32.astype(np.float64)).astype(np.float32)
    sides = (("user", ops.ialspp_gram(Z, scale=s), Gw32, None, lambda r: pr.system32(indptr, indices, None, Z32, Gw32, X32[r], e32, a0, lam, r, p0, k)),
             ("item", ops.ialspp_gram(Z), G32, al, lambda r: wr.system32(indptr, indices, None, Z32, G32, X32[r], e32, al32, lam, r, p0, k)))
    for name, G, want_G, alpha_row, ref in sides:
        assert torch.equal(bits(G), bits(torch.from_numpy(want_G).to(dev))), name
        X, e = to(dev, X32, e32)
        dbg = torch.full((NR, k * k + k), float("nan"), device=dev)
        ops.ialspp_block_pass(g, "user", Z, X, blk, k, G=G, e=e, work=work, dbg=dbg, alpha_row=alpha_row)
        got = dbg.cpu().numpy()
        for r in range(NR):
            H, gg = ref(r)
            assert np.array_equal(got[r, :k * k].reshape(k, k).view(np.int32), H.view(np.int32)), (name, r, ir.ROW_LENGTHS[r])
            assert np.array_equal(got[r, k * k:].view(np.int32), gg.view(np.int32)), (name, r, ir.ROW_LENGTHS[r], np.abs(got[r, k * k:] - gg).max())
        assert torch.isfinite(X).all() and torch.isfinite(e).all() and ops.ialspp_buffers(g, d)["fail"].item() == 0


# ---- 3. solutions and passes against float64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", ir.PARAMS, ids=lambda p: "a%g-l%g-n%g" % p)
@pytest.mark.parametrize("kind", ir.TABLES)
@pytest.mark.parametrize("d", [32, 64, 128])
def test_the_solve_stays_inside_the_a_priori_bound_on_both_sides(dev, lengths, d, kind, params):
    from pda_amd import ops
    rows, cols, indptr, indices = lengths
    a0, lam, nu = params
    b = wr.bound_inputs(a0)
    g = graph_of(dev, rows, cols, NR, ir.N_OTHER, a0, lam, nu)
    Z32 = tables(kind, d)[0]
    Z, s, al = to(dev, Z32, b["s"], b["alpha_rows"])
    work = g.user.sub_list(range(NR), shuffle_seed=2)
    lam_user = ir.lam_row(np.diff(indptr), ir.N_OTHER, lam, a0, nu)
    lam_item = wr.lam_row_items(np.diff(indptr), ir.N_OTHER, lam, a0, nu, b["w_rows"])
    for name, lam_row, alpha_row, G, o in (
            ("user", lam_user, None, ops.ials_gram(Z, scale=s), wr.row_bounds(indptr, indices, Z32, a0, lam_user, range(NR), scale=b["s"])),
            ("item", lam_item, al, None, wr.row_bounds(indptr, indices, Z32, b["alpha_rows"], lam_item, range(NR)))):
        g.user.lam_row = torch.from_numpy(lam_row).to(dev)
        X = torch.full((NR, d), float("nan"), device=dev)
        ops.ials_half_sweep(g, "user", Z, X, G=G, work=work, alpha_row=alpha_row)
        assert (o["kappa"] * o["eta"]).max() < 0.1                                          # the condition on the inputs (the host suite has it too)
        x = X.cpu().numpy().astype(np.float64)
        err = np.linalg.norm(x - o["x"], axis=1)
        allowed = o["bound"] * o["xnorm"]
        ratio = np.divide(err, allowed, out=np.zeros_like(err), where=allowed > 0)
        print("ials itemw solve %s d=%d %s %s: observed / bound max %.3g (row of %d pairs), kappa max %.1f" %
              (name, d, kind, params, ratio.max(), ir.ROW_LENGTHS[int(ratio.argmax())], o["kappa"].max()))
        assert (x[0] == 0).all() and np.isfinite(x).all() and g.buffers(d)["fail"].item() == 0
        assert (err <= allowed).all(), (name, (err / np.maximum(allowed, 1e-300)).max())


@pytest.mark.parametrize("kind", ir.TABLES)
@pytest.mark.parametrize("d, k", [(32, 32), (64, 32), (128, 64), (128, 128), (256, 32), (256, 128)])
def test_a_pass_stays_inside_the_a_priori_bound_on_both_sides(dev, lengths, d, k, kind):
    """As tests/test_gpu_ialspp.py holds a pass: the new x_{r,pi} and e of every listed row inside the bound, everything else untouched."""
    from pda_amd import ops
    rows, cols, indptr, indices = lengths
    blk = d // k - 1
    p0 = blk * k
    b = wr.bound_inputs(A0)
    g = graph_of(dev, rows, cols, NR, ir.N_OTHER)
    Z32, X32 = tables(kind, d)
    e32 = pr.predictions(X32, Z32, indptr, indices).astype(np.float32)
    listed = [r for r in range(NR) if r != 4]                                               # the row of 32 pairs stays out
    Z, s, al = to(dev, Z32, b["s"], b["alpha_rows"])
    lam_user = ir.lam_row(np.diff(indptr), ir.N_OTHER, LAM, A0, NU)
    lam_item = wr.lam_row_items(np.diff(indptr), ir.N_OTHER, LAM, A0, NU, b["w_rows"])
    outside = np.ones(d, dtype=bool)
    outside[p0:p0 + k] = False
    for name, lam_row, alpha_row, scale in (("user", lam_user, None, s), ("item", lam_item, al, None)):
        g.user.lam_row = torch.from_numpy(lam_row).to(dev)
        X, e = to(dev, X32, e32)
        G = ops.ialspp_gram(Z, scale=scale)
        ops.ialspp_block_pass(g, "user", Z, X, blk, k, G=G, e=e, work=g.user.sub_list(listed, shuffle_seed=2), alpha_row=alpha_row)
        o = wr.pass_bounds(X32, e32, indptr, indices, None, Z32, A0 if name == "user" else b["alpha_rows"], lam_row, p0, k,
                           scale=b["s"] if name == "user" else None, rows=listed)
        assert np.isfinite(o["dX"]).all() and np.isfinite(o["de"]).all()
        x, ee = X.cpu().numpy(), e.cpu().numpy()
        assert np.isfinite(x).all() and np.isfinite(ee).all() and ops.ialspp_buffers(g, d)["fail"].item() == 0
        assert np.array_equal(x[:, outside].view(np.int32), X32[:, outside].view(np.int32))
        assert np.array_equal(x[4].view(np.int32), X32[4].view(np.int32))
        assert np.array_equal(ee[indptr[4]:indptr[5]].view(np.int32), e32[indptr[4]:indptr[5]].view(np.int32))
        ex = np.linalg.norm(x.astype(np.float64) - o["X"], axis=1)
        ed = np.abs(ee.astype(np.float64) - o["e"])
        print("ials itemw pass %s d=%d k=%d %s: observed / bound max %.3g (x), %.3g (e)" %
              (name, d, k, kind, np.max(ex[listed] / o["dX"][listed]), np.max(ed / np.maximum(o["de"], 1e-300))))
        assert (ex <= o["dX"]).all(), (name, (ex / np.maximum(o["dX"], 1e-300)).max())
        assert (ed <= o["de"]).all(), (name, (ed / np.maximum(o["de"], 1e-300)).max())


# ---- 4. the loss ---------------------------------------------------------------------------------------------------------------------------------------
def toy_pairs(seed=3, nu=70, ni=45, n=2500):
    g = np.random.default_rng(seed)
    return g.integers(0, nu - 1, n), np.minimum(g.zipf(1.4, n) - 1, ni - 2), nu, ni      # the last user and the last item stay without pairs


def toy_csrs(u, i, nu, ni):
    eu, ei = ir.dedup_pairs(u, i, ni)
    up, ui = ir.csr(eu, ei, nu)
    ip, ii = ir.csr(ei, eu, ni)
    return eu, ei, up, ui, ip, ii


@pytest.mark.parametrize("case", ["toy-32", "toy-128", "toy-256", "lengths-64", "lengths-256"])
def test_the_loss_equals_the_float64_weighted_objective_within_its_bound(dev, lengths, case):
    from pda_amd import ops
    d = int(case.split("-")[1])
    if case.startswith("toy"):
        u, i, nu, ni = toy_pairs()
    else:
        u, i, nu, ni = lengths[0], lengths[1], NR, ir.N_OTHER
    g = graph_of(dev, u, i, nu, ni, item_power=wr.BETA)
    eu, ei, up, ui, ip, ii = toy_csrs(u, i, nu, ni)
    iw = wr.item_weights(np.diff(ip), wr.BETA, A0)
    np.testing.assert_array_equal(g.item_weights.host_scale, iw["s"])
    X32, Y32 = ir.table("gauss0.3", nu, d, seed=5), ir.table("gauss0.3", ni, d, seed=6)
    X, Y = to(dev, X32, Y32)
    got = (ops.ialspp_loss(g, X, Y) if d == 256 else ops.ials_loss(g, X, Y)).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (3,)
    lu, li = g.user.host_lam_row, g.item.host_lam_row
    np.testing.assert_array_equal(li, wr.lam_row_items(np.diff(ip), nu, LAM, A0, NU, iw["w"]))
    L, fit, reg = wr.objective(X32, Y32, eu, ei, wr.user_item_alpha(A0, iw["s"]), lu, li)
    bound = wr.loss_bound(X32, Y32, up, ui, A0, iw["s"], lu, L)
    print("ials itemw loss %s: |L^ - L| / bound = %.3g (L = %.6g, bound = %.3g)" % (case, abs(got[0] - L) / bound, L, bound))
    assert abs(got[0] - L) <= bound and abs(got[1] - fit) <= bound and abs(got[2] - reg) <= bound
    if d <= 128:
        assert torch.equal(ops.ialspp_loss(g, X, Y), ops.ials_loss(g, X, Y))


# ---- 5. identity with today's paths ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, k", [(32, 32), (64, 32), (128, 128), (256, 32), (256, 128)])
def test_unit_scale_and_constant_alpha_row_give_the_bits_of_the_unweighted_entry_points(dev, lengths, d, k):
    from pda_amd import ops
    rows, cols, indptr, indices = lengths
    g = graph_of(dev, rows, cols, NR, ir.N_OTHER)
    Z32, X32 = tables("gauss0.3", d)
    Z, = to(dev, Z32)
    ones = torch.ones(ir.N_OTHER, device=dev)
    al = torch.full((NR,), float(np.float32(A0)), device=dev)
    with CountCalls(NEW_ENTRY_POINTS) as cc:
        G = ops.ialspp_gram(Z)
        assert sum(cc.calls.values()) == 0
        assert torch.equal(bits(ops.ialspp_gram(Z, scale=ones)), bits(G))
        assert cc.calls["pda_ials_gram_scaled_f32"] == 1
        if d <= 128:
            assert torch.equal(bits(ops.ials_gram(Z, scale=ones)), bits(ops.ials_gram(Z)))
            A, B = torch.full((NR, d), float("nan"), device=dev), torch.full((NR, d), float("nan"), device=dev)
            da, dbb = torch.zeros((NR, d * d + d), device=dev), torch.zeros((NR, d * d + d), device=dev)
            ops.ials_half_sweep(g, "user", Z, A, G=G, dbg_normal=da)
            before = cc.calls["pda_ials_half_sweep_rowalpha_f32"]
            ops.ials_half_sweep(g, "user", Z, B, G=G, dbg_normal=dbb, alpha_row=al)
            assert cc.calls["pda_ials_half_sweep_rowalpha_f32"] == before + 1
            assert torch.equal(bits(A), bits(B)) and torch.equal(bits(da), bits(dbb)) and torch.isfinite(A).all()
        e32 = pr.predictions(X32, Z32, indptr, indices).astype(np.float32)
        out = []
        for alpha_row in (None, al):
            X, e = to(dev, X32, e32)
            dbg = torch.zeros((NR, k * k + k), device=dev)
            ops.ialspp_block_pass(g, "user", Z, X, d // k - 1, k, G=G, e=e, dbg=dbg, alpha_row=alpha_row)
            out.append((X, e, dbg))
        assert cc.calls["pda_ialspp_block_pass_rowalpha_f32"] == 1
    for a, b in zip(*out):
        assert torch.equal(bits(a), bits(b))
    assert torch.isfinite(out[0][0]).all() and not torch.equal(bits(out[0][0]), bits(torch.from_numpy(X32).to(dev)))


def make_model(dev, d, solver="exact", k=32, **over):
    from pda_amd.model_api import IALSMF, gcn_train_pairs
    from pda_amd.parse import parse_args
    args = parse_args(["--train", "ials", "--ials_solver", solver, "--ials_block", str(k), "--embed_size", str(d), "--regs", "0.05", "--verbose", "0"])
    for key, v in over.items():
        setattr(args, key, v)
    u, i, nu, ni = toy_pairs()
    lists = {int(x): [] for x in range(nu)}
    for a, b in zip(u.tolist(), i.tolist()):
        lists[a].append(b)                                                                  # (with duplicates: the graph counts a pair once)
    return IALSMF(args, {"n_users": nu, "n_items": ni, "gcn_train_pairs": gcn_train_pairs(lists)}, device=dev), (u, i, nu, ni)


@pytest.mark.parametrize("d, solver", [(64, "exact"), (64, "block"), (256, "block")])
def test_an_epoch_at_power_zero_is_bit_for_bit_the_unweighted_epoch_on_the_unweighted_entry_points(dev, d, solver):
    """Two epochs of the model at --ials_item_power 0 (the default, and given as 0.0) against the same two epochs made by hand from the
    unweighted entry points on a graph that was never told about weights; none of the new entry points is called.  At 0.5 the bits differ and
    the new entry points are the ones that run."""
    from pda_amd import _lib, ops
    lib = _lib.load()
    m, (u, i, nu, ni) = make_model(dev, d, solver, ials_item_power=0.0)
    assert m.graph.item_weights is None and "ials_item_power" not in m.state_dict()
    X0, Y0 = (m.weights[key].clone() for key in ("user_embedding", "item_embedding"))
    with CountCalls(NEW_ENTRY_POINTS) as cc:
        losses = [m.train_epoch().clone() for _ in range(2)]
    assert sum(cc.calls.values()) == 0
    g = ops.IalsGraph(u, i, nu, ni, dev, lam=0.05, alpha0=0.1, nu=1.0)
    X, Y = X0.clone(), Y0.clone()
    for ep in range(2):                                                                     # the library, called directly
        if solver == "exact":
            for side, fixed, out in (("user", Y, X), ("item", X, Y)):
                s = g.side(side)
                b = g.buffers(d)
                ops.check(lib.pda_ials_gram_f32(ops.ptr(fixed), fixed.shape[0], d, ops.ptr(b["G"]), ops.ptr(b["ws"]), b["ws"].numel(), ops.stream_ptr()), "gram")
                w = s.all_rows
                ops.check(lib.pda_ials_half_sweep_f32(ops.ptr(s.indptr), ops.ptr(s.indices), s.n_rows, s.nnz, ops.ptr(w.work), w.n_work,
                                                      ops.ptr(w.long_rows) if w.n_long else None, w.n_long, w.n_slots, ops.ptr(fixed), s.n_other,
                                                      ops.ptr(b["G"]), d, 0.1, ops.ptr(s.lam_row), ops.ptr(out), ops.ptr(b["fail"]), None,
                                                      ops.ptr(b["ws"]) if w.n_slots else None, b["ws"].numel() if w.n_slots else 0, ops.stream_ptr()), "sweep")
            L = ops.ials_loss(g, X, Y) / g.nnz
        else:
            L = ops.ialspp_epoch(g, X, Y, 32) / g.nnz
        assert torch.equal(L, losses[ep]), ep
    assert torch.equal(bits(X), bits(m.weights["user_embedding"])) and torch.equal(bits(Y), bits(m.weights["item_embedding"]))
    assert torch.isfinite(X).all() and m.failed_pivots().item() == 0
    mw, _ = make_model(dev, d, solver, ials_item_power=0.5)
    assert torch.equal(bits(mw.weights["user_embedding"]), bits(X0))                        # the same start
    with CountCalls(NEW_ENTRY_POINTS) as cc:
        mw.train_epoch()
    assert cc.calls["pda_ials_gram_scaled_f32"] >= 2 and (cc.calls["pda_ials_half_sweep_rowalpha_f32"] == 1 if solver == "exact"
                                                          else cc.calls["pda_ialspp_block_pass_rowalpha_f32"] == d // 32)
    assert cc.calls["pda_ialspp_gram256_scaled_f32"] == 0                                   # (reached through pda_ials_gram_scaled_f32, inside the library)
    assert mw.state_dict()["ials_item_power"] == 0.5 and mw.failed_pivots().item() == 0


# ---- 6. training ---------------------------------------------------------------------------------------------------------------------------------------
def weighted_setup(m, u, i, nu, ni):
    eu, ei, up, ui, ip, ii = toy_csrs(u, i, nu, ni)
    iw = wr.item_weights(np.diff(ip), wr.BETA, A0)
    g = m.graph
    np.testing.assert_array_equal(g.item_weights.host_scale, iw["s"])
    np.testing.assert_array_equal(g.item_weights.host_alpha_row, iw["alpha_row"])
    lu, li = ir.lam_row(np.diff(up), ni, LAM, A0, NU), wr.lam_row_items(np.diff(ip), nu, LAM, A0, NU, iw["w"])
    np.testing.assert_array_equal(g.user.host_lam_row, lu)
    np.testing.assert_array_equal(g.item.host_lam_row, li)
    a_user = wr.user_item_alpha(A0, iw["s"])
    return eu, ei, up, ui, ip, ii, iw, lu, li, a_user, np.abs(wr.item_alpha(iw["alpha_row"]) - a_user)


def test_six_epochs_of_the_exact_solver_never_raise_the_weighted_objective(dev):
    """tests/test_gpu_ials.py's six epochs at beta = 0.5, d = 64: the float64 weighted objective after every half-sweep against the one before,
    with the allowance of that test, sum_r lambda_max(A_r) |dx_r|^2 (the item side through ials_itemw_ref.item_allowance, which also counts
    the one rounding between the weights of the two sides)."""
    from pda_amd import ops
    m, (u, i, nu, ni) = make_model(dev, 64, ials_item_power=wr.BETA)
    eu, ei, up, ui, ip, ii, iw, lu, li, a_user, da = weighted_setup(m, u, i, nu, ni)
    X, Y = m.weights["user_embedding"], m.weights["item_embedding"]
    obj = lambda: wr.objective(X.cpu().numpy(), Y.cpu().numpy(), eu, ei, a_user, lu, li)[0]   # noqa: E731
    last, worst = obj(), -np.inf
    for epoch in range(6):
        b = wr.row_bounds(up, ui, Y.cpu().numpy(), A0, lu, range(nu), scale=iw["s"])
        allowance = float(np.sum(b["lmax"] * (b["bound"] * b["xnorm"]) ** 2))
        ops.ials_half_sweep(m.graph, "user", Y, X)
        now = obj()
        worst = max(worst, (now - last) / last)
        assert now <= last + allowance, (epoch, "user", now - last, allowance)
        last = now
        x32 = X.cpu().numpy()
        b = wr.row_bounds(ip, ii, x32, iw["alpha_row"], li, range(ni))
        Gn = np.linalg.norm(x32.astype(np.float64).T @ x32.astype(np.float64), 2)
        allowance = wr.item_allowance(b["lmax"], b["lmin"], b["bound"] * b["xnorm"], da, Gn, b["xnorm"])
        ops.ials_half_sweep(m.graph, "item", X, Y)
        now = obj()
        worst = max(worst, (now - last) / last)
        assert np.isfinite(allowance) and now <= last + allowance, (epoch, "item", now - last, allowance)
        last = now
    print("ials itemw objective over 12 half-sweeps: worst relative step %.3g, final %.6g" % (worst, last))
    assert m.failed_pivots().item() == 0 and torch.isfinite(X).all() and torch.isfinite(Y).all()


def test_six_epochs_of_the_block_solver_never_raise_the_weighted_objective(dev):
    """tests/test_gpu_ialspp.py's six epochs at beta = 0.5, d = 256, k = 32, pass by pass as ops.ialspp_epoch runs them, with that test's
    allowance sum_r lambda_max(H_r) err_r^2 (the item side through item_allowance) and its hold on the cache."""
    from pda_amd import ops
    d, k = 256, 32
    m, (u, i, nu, ni) = make_model(dev, d, "block", k, ials_item_power=wr.BETA)
    eu, ei, up, ui, ip, ii, iw, lu, li, a_user, da = weighted_setup(m, u, i, nu, ni)
    g = m.graph
    perm = g.pair_perm.cpu().numpy()
    X, Y = m.weights["user_embedding"], m.weights["item_embedding"]
    host = lambda: (X.cpu().numpy(), Y.cpu().numpy())                                       # noqa: E731
    obj = lambda: wr.objective(*host(), eu, ei, a_user, lu, li)[0]                          # noqa: E731
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
                    o = wr.pass_bounds(x32, true, up, ui, None, y32, A0, lu, p0, k, scale=iw["s"], de=de)
                    allowance = float(np.sum(o["lmax"] * o["err"] ** 2))
                    ops.ialspp_block_pass(g, "user", Y, X, blk, k)
                else:
                    o = wr.pass_bounds(y32, true, ip, ii, perm, x32, iw["alpha_row"], li, p0, k, de=de)
                    Gn = np.linalg.norm(x32.astype(np.float64).T @ x32.astype(np.float64), 2)
                    allowance = wr.item_allowance(o["lmax"], o["lmin"], o["err"], da, Gn, o["xnorm"], o["delta_norm"])
                    ops.ialspp_block_pass(g, "item", X, Y, blk, k)
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
    print("ials itemw block d=%d: worst relative step of the objective %.3g over %d passes, final %.6g; cache / bound max %.3g" %
          (d, worst, 12 * (d // k), last, worst_cache))
    assert m.failed_pivots().item() == 0 and torch.isfinite(X).all() and torch.isfinite(Y).all()
    got = ops.ialspp_loss(g, X, Y).cpu().numpy()
    x32, y32 = host()
    L, fit, reg = wr.objective(x32, y32, eu, ei, a_user, lu, li)
    bound = wr.loss_bound(x32, y32, up, ui, A0, iw["s"], lu, L)
    assert abs(got[0] - L) <= bound and abs(got[1] - fit) <= bound and abs(got[2] - reg) <= bound


def test_one_epoch_of_the_exact_model_is_the_restatement_s_epoch(dev):
    m, (u, i, nu, ni) = make_model(dev, 32, ials_item_power=wr.BETA)
    eu, ei, up, ui, ip, ii, iw, lu, li, a_user, da = weighted_setup(m, u, i, nu, ni)
    X0, Y0 = (m.weights[key].cpu().numpy() for key in ("user_embedding", "item_embedding"))
    out = m.train_epoch()
    assert out.dtype == torch.float64 and out.shape == (3,) and out.is_cuda
    X, Y = (m.weights[key].cpu().numpy().astype(np.float64) for key in ("user_embedding", "item_embedding"))
    bx = wr.row_bounds(up, ui, Y0, A0, lu, range(nu), scale=iw["s"])
    X1, Y1 = wr.epoch(X0, Y0, up, ui, ip, ii, A0, iw["s"], iw["alpha_row"], lu, li)
    np.testing.assert_allclose(bx["x"], X1, atol=1e-12)
    ex = np.linalg.norm(X - X1, axis=1)
    assert (ex <= bx["bound"] * bx["xnorm"]).all()
    by = wr.row_bounds(ip, ii, X1, iw["alpha_row"], li, range(ni), dZ=bx["bound"] * bx["xnorm"])      # the user side's error, propagated
    np.testing.assert_allclose(by["x"], Y1, atol=1e-12)
    ey = np.linalg.norm(Y - Y1, axis=1)
    print("ials itemw model epoch: observed / bound max %.3g (users), %.3g (items)" %
          (np.max(ex / np.maximum(bx["bound"] * bx["xnorm"], 1e-300)), np.max(ey / np.maximum(by["bound"] * by["xnorm"], 1e-300))))
    assert np.isfinite(by["bound"]).all() and (ey <= by["bound"] * by["xnorm"]).all()
    assert (X[-1] == 0).all() and (Y[-1] == 0).all() and m.failed_pivots().item() == 0     # the user and the item without pairs
    X0u, _ = ir.epoch(X0, Y0, up, ui, ip, ii, A0, lu, ir.lam_row(np.diff(ip), nu, LAM, A0, NU))
    assert np.linalg.norm(X - X0u, axis=1).max() > 10 * (bx["bound"] * bx["xnorm"]).max()    # (not the unweighted epoch)
    X32, Y32 = (m.weights[key].cpu().numpy() for key in ("user_embedding", "item_embedding"))
    L, fit, reg = wr.objective(X32, Y32, eu, ei, a_user, lu, li)
    bound = wr.loss_bound(X32, Y32, up, ui, A0, iw["s"], lu, L)
    got = out.cpu().numpy() * len(eu)
    assert abs(got[0] - L) <= bound and abs(got[1] - fit) <= bound and abs(got[2] - reg) <= bound


@pytest.mark.parametrize("d, k", [(64, 32), (256, 32)])
def test_one_epoch_of_the_block_model_is_the_restatement_s_epoch(dev, d, k):
    """train_epoch() gives the bits of predict + the passes in the restatement's order, run one by one with the weights handed over by hand;
    every one of those passes lies within pass_bounds of the restatement's pass from the state the kernels left."""
    from pda_amd import ops
    m, (u, i, nu, ni) = make_model(dev, d, "block", k, ials_item_power=wr.BETA)
    eu, ei, up, ui, ip, ii, iw, lu, li, a_user, da = weighted_setup(m, u, i, nu, ni)
    X0, Y0 = (m.weights[key].cpu().numpy() for key in ("user_embedding", "item_embedding"))
    out = m.train_epoch()
    e_model = m.graph.e.cpu().numpy().copy()
    assert m.failed_pivots().item() == 0
    g = ops.IalsGraph(u, i, nu, ni, dev, lam=LAM, alpha0=A0, nu=NU)                         # a graph without weights: they come by hand
    g.item.lam_row = torch.from_numpy(li).to(dev)
    perm = pr.pair_perm(up, ui, ip, ii)
    X2, Y2, s, al = to(dev, X0, Y0, iw["s"], iw["alpha_row"])
    e = ops.ialspp_predict(g, X2, Y2)
    worst = 0.0
    for blk, p0 in enumerate(g.blocks(d, k)):
        for side in ("user", "item"):
            x32, y32, e32 = X2.cpu().numpy(), Y2.cpu().numpy(), e.cpu().numpy().copy()
            if side == "user":
                o = wr.pass_bounds(x32, e32, up, ui, None, y32, A0, lu, p0, k, scale=iw["s"])
                new = ops.ialspp_block_pass(g, "user", Y2, X2, blk, k, G=ops.ialspp_gram(Y2, scale=s)).cpu().numpy()
            else:
                o = wr.pass_bounds(y32, e32, ip, ii, perm, x32, iw["alpha_row"], li, p0, k)
                new = ops.ialspp_block_pass(g, "item", X2, Y2, blk, k, alpha_row=al).cpu().numpy()
            ex, ed = np.linalg.norm(new - o["X"], axis=1), np.abs(e.cpu().numpy() - o["e"])
            assert np.isfinite(o["dX"]).all() and (ex <= o["dX"]).all() and (ed <= o["de"]).all(), (blk, side)
            worst = max(worst, float(np.max(ex / o["dX"])), float(np.max(ed / np.maximum(o["de"], 1e-300))))
    print("ials itemw block model epoch d=%d k=%d: observed / bound max %.3g over the passes" % (d, k, worst))
    assert torch.equal(bits(X2), bits(m.weights["user_embedding"])) and torch.equal(bits(Y2), bits(m.weights["item_embedding"]))
    assert np.array_equal(e.cpu().numpy().view(np.int32), e_model.view(np.int32))
    X32, Y32 = X2.cpu().numpy(), Y2.cpu().numpy()
    L, fit, reg = wr.objective(X32, Y32, eu, ei, a_user, lu, li)
    bound = wr.loss_bound(X32, Y32, up, ui, A0, iw["s"], lu, L)
    got = out.cpu().numpy() * len(eu)
    assert abs(got[0] - L) <= bound and abs(got[1] - fit) <= bound and abs(got[2] - reg) <= bound


# ---- 7. robustness -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, k", [(64, 32), (256, 128)])
def test_bits_do_not_depend_on_the_call(dev, d, k):
    """Two calls are bit-equal; a row solved alone equals the same row solved among the others; a permuted work list gives the same bits --
    for the half-sweep with alpha_row against G_w (d <= 128) and for the block pass."""
    from pda_amd import ops
    n = 40
    rs = np.random.default_rng(4)
    lens = list(ir.ROW_LENGTHS) + [int(v) for v in rs.integers(1, 60, n - NR)]
    rows, cols = ir.length_graph(seed=9, lengths=lens)
    indptr, indices = ir.csr(rows, cols, n)
    g = graph_of(dev, rows, cols, n, ir.N_OTHER)
    Z32 = tables("gauss0.3", d)[0]
    X32 = ir.table("gauss0.3", n, d, seed=8)
    e32 = pr.predictions(X32, Z32, indptr, indices).astype(np.float32)
    iw = wr.item_weights(wr.bound_counts(), wr.BETA, A0)
    al32 = wr.item_weights(rs.integers(0, 500, n), wr.BETA, A0)["alpha_row"]
    Z, s, al = to(dev, Z32, iw["s"], al32)
    G = ops.ialspp_gram(Z, scale=s)
    assert torch.equal(bits(G), bits(ops.ialspp_gram(Z, scale=s))) and torch.equal(bits(G), bits(G.t().contiguous()))
    blk = d // k - 1

    def run_pass(work):
        X, e = to(dev, X32, e32)
        ops.ialspp_block_pass(g, "user", Z, X, blk, k, G=G, e=e, work=work, alpha_row=al)
        return X, e

    def run_sweep(work):
        X = torch.full((n, d), float("nan"), device=dev)
        ops.ials_half_sweep(g, "user", Z, X, G=G, work=work, alpha_row=al)
        return X

    bx, be = run_pass(None)
    assert torch.isfinite(bx).all() and torch.isfinite(be).all()
    shuffled = [None, g.user.sub_list(range(n), shuffle_seed=1), g.user.sub_list(range(n), shuffle_seed=2)]
    for work in shuffled:
        x, e = run_pass(work)
        assert torch.equal(bits(bx), bits(x)) and torch.equal(bits(be), bits(e))
    X0, e0 = to(dev, X32, e32)
    singles = (0, 1, NR - 2, NR - 1, n - 1)                                                 # empty, one pair, one chunk + 1, three chunks, the last
    for r in singles:
        x, e = run_pass(g.user.sub_list([r]))
        a, b = int(indptr[r]), int(indptr[r + 1])
        assert torch.equal(bits(x[r]), bits(bx[r])) and torch.equal(bits(e[a:b]), bits(be[a:b])), r
        others = torch.ones(n, dtype=torch.bool, device=dev)
        others[r] = False
        pairs = torch.ones(len(e32), dtype=torch.bool, device=dev)
        pairs[a:b] = False
        assert torch.equal(bits(x[others]), bits(X0[others])) and torch.equal(bits(e[pairs]), bits(e0[pairs]))   # what a call does not list stays
    if d <= 128:
        base = run_sweep(None)
        assert torch.isfinite(base).all()
        for work in shuffled:
            assert torch.equal(bits(base), bits(run_sweep(work)))
        for r in singles:
            alone = run_sweep(g.user.sub_list([r]))
            assert torch.equal(bits(alone[r]), bits(base[r])), r
            others = torch.ones(n, dtype=torch.bool, device=dev)
            others[r] = False
            assert torch.isnan(alone[others]).all()


def test_no_call_depends_on_what_its_scratch_held(dev, lengths):
    """The Gram workspace, the slots, the delta buffer, the half-sweep's workspace and G itself hold the 0xFF pattern (NaN) in one run and
    0x3F in the other, each of exactly the size the headers' formulas give; every tensor the calls leave behind is bit-equal between the runs."""
    from pda_amd import ops
    rows, cols, indptr, indices = lengths
    g = graph_of(dev, rows, cols, NR, ir.N_OTHER)
    n_slots = g.user.all_rows.n_slots
    assert n_slots == 5
    b = wr.bound_inputs(A0)
    nb = -(-ir.N_OTHER // ir.GRAM_ROWS)
    ops.ialspp_buffers(g, 256, 32)                                                          # (built once, outside: both runs make the same calls)
    ops.ialspp_buffers(g, 64, 32)

    def filled(n, fill):
        return torch.full((4 * n,), fill, dtype=torch.uint8, device=dev).view(torch.float32)

    records = {}
    for fill in (0xFF, 0x3F):
        assert fill in db.FILLS
        with db.Recorder(fill) as rec:
            for d, k, blk in ((256, 32, 7), (64, 32, 1)):
                Z32, X32 = tables("gauss0.3", d)
                e32 = pr.predictions(X32, Z32, indptr, indices).astype(np.float32)
                Z, s, al, X, e = to(dev, Z32, b["s"], b["alpha_rows"], X32, e32)
                G = ops.ialspp_gram(Z, filled(d * d, fill).view(d, d), filled(nb * (d * d + d), fill), scale=s)
                ops.ialspp_block_pass(g, "user", Z, X, blk, k, G=G, e=e, slots=filled(n_slots * (k * k + k), fill), delta_ws=filled(n_slots * k, fill),
                                      alpha_row=al)
                Gs = ops.ialspp_gram(Z[:600].contiguous(), filled(d * d, fill).view(d, d), filled(3 * (d * d + d), fill), scale=s[:600].contiguous())
                assert torch.isfinite(Gs).all() and torch.isfinite(X).all() and torch.isfinite(e).all()
            d = 64
            g.buffers(d)["ws"] = filled(n_slots * (d * d + d), fill).view(torch.uint8)
            Gx = ops.ials_gram(Z, filled(d * d, fill).view(d, d), filled(nb * (d * d + d), fill).view(torch.uint8), scale=s)
            Xo = filled(NR * d, fill).view(NR, d)
            ops.ials_half_sweep(g, "user", Z, Xo, G=Gx, alpha_row=al)
            assert torch.isfinite(Xo).all()
        records[fill] = rec.records
    names = [n for n, _ in records[0xFF]]
    assert names.count("ialspp_gram") == 4 and names.count("ialspp_block_pass") == 2 and names.count("ials_gram") == 1 and names.count("ials_half_sweep") == 1
    db.same_records(records[0xFF], records[0x3F], "item-weighted iALS scratch under two fills")


# ---- 8. through the CLI ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from pda_amd import synthetic
    root = tmp_path_factory.mktemp("ials_itemw_data")
    synthetic.write_dataset(str(root / "toy"), n_users=400, n_items=300, mean_hist=20)
    return str(root) + "/"


def _argv(toy, save, extra=()):
    return ["--data_path", toy, "--dataset", "toy", "--train", "ials", "--test", "normal", "--epoch", "3", "--log_interval", "1", "--embed_size", "32",
            "--regs", "0.05", "--valid_set", "valid", "--pop_exp", "0.22", "--save_dir", save, "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t",
            "--cuda", "0", "--eval_block", "128"] + list(extra)


def _run(module, argv):
    r = subprocess.run([sys.executable, "-m", module] + argv, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _ckpt(save):
    found = glob.glob(os.path.join(save, "**", "best_ckpt.ckpt"), recursive=True)
    assert len(found) == 1 and "_train_ials" in found[0] and os.path.basename(os.path.dirname(found[0])).endswith("ials"), found
    return torch.load(found[0], map_location="cpu")


def test_the_cli_trains_checkpoints_restores_and_exports_with_item_weights(dev, toy, tmp_path):
    from pda_amd.model_api import BPRMF
    from pda_amd.parse import parse_args
    saves = [str(tmp_path / k) + "/" for k in "ab"]
    W = ("--ials_item_power", "0.5")
    out = _run("pda_amd.train_new_api", _argv(toy, saves[0], W))
    losses = [[float(x) for x in mm.groups()] for mm in re.finditer(r"Epoch \d+ \[[^\]]*\]: train==\[([-\d.]+)=([-\d.]+) \+ ([-\d.]+)\]", out)]
    assert len(losses) == 3 and np.isfinite(losses).all(), out[-2000:]
    assert losses[0][0] > losses[1][0] > losses[2][0]                                       # the printed loss falls
    line = re.findall(r"^\|\|--- ials item_power=(\S+) w_min=(\S+) w_max=(\S+)$", out, flags=re.M)
    assert len(line) == 1 and float(line[0][0]) == 0.5 and 0 < float(line[0][1]) < 1 < float(line[0][2])
    assert "recall=[" in out and "running iALS" in out
    sd = _ckpt(saves[0])                                                                    # the run directory's suffix stays "ials"
    assert sd.get("model", "mf") == "mf" and "mU" not in sd and tuple(sd["user_embedding"].shape) == (400, 32) and sd["ials_item_power"] == 0.5
    plain = BPRMF(parse_args(["--embed_size", "32", "--verbose", "0", "--optimizer", "sgd"]), {"n_users": 400, "n_items": 300}, device=dev)
    plain.load_state_dict(sd)
    assert torch.equal(plain.weights["item_embedding"].cpu(), sd["item_embedding"]) and torch.isfinite(sd["item_embedding"]).all()
    npz = str(tmp_path / "lists.npz")
    _run("pda_amd.export_topk", _argv(toy, saves[0], W + ("--export_out", npz)))
    lists = np.load(npz)
    assert lists["idx"].shape[1] == 50 and lists["idx"].shape[0] == lists["users"].shape[0] > 0 and (lists["idx"] < 300).all()
    # a run at 0 writes the checkpoint of before (no key), restores and exports as before, and is another model than the weighted one
    out0 = _run("pda_amd.train_new_api", _argv(toy, saves[1], ("--ials_item_power", "0")))
    assert "ials item_power" not in out0
    sd0 = _ckpt(saves[1])
    assert "ials_item_power" not in sd0 and not torch.equal(sd0["item_embedding"], sd["item_embedding"])
    plain.load_state_dict(sd0)
    assert torch.equal(plain.weights["user_embedding"].cpu(), sd0["user_embedding"])
    npz0 = str(tmp_path / "lists0.npz")
    _run("pda_amd.export_topk", _argv(toy, saves[1], ("--export_out", npz0)))
    assert np.load(npz0)["idx"].shape == lists["idx"].shape
