"""CPU suite for item-weighted iALS (`--train ials --ials_item_power`, include/pda_hip_ials_itemw.h): the weights and the item side's
lam_row against the stated formulas, the flag and its refusals, the state dict, the binding against the header, the new entry points' argument
checks (every call carries a violation, so none reaches a launch), and the properties of the restatement tests/ials_itemw_ref.py that the GPU
suite leans on: every row solution zeroes the float64 gradient of the stated objective, an epoch of either solver never raises it, the exact
tests' inputs are exact in fp32, and the bound test's inputs keep kappa eta below a tenth on both sides."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ials_itemw_ref as wr
import ials_ref as ir
import ialspp_ref as pr
from test_abi import declared_in

ERR_ARG, ERR_UNSUPPORTED = -1, -2
NULL = C.c_void_p(None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pda_ials_gram_scaled_f32", "pda_ials_half_sweep_rowalpha_f32", "pda_ialspp_block_pass_rowalpha_f32", "pda_ialspp_gram256_scaled_f32"]


def make_args(**over):
    from pda_amd.parse import parse_args
    a = parse_args(["--train", "ials", "--embed_size", "32", "--regs", "0.05"])
    for k, v in over.items():
        setattr(a, k, v)
    return a


def zipf_counts(n=300, seed=1):
    return np.minimum(np.random.default_rng(seed).zipf(1.3, n) - 1, 5000)


# ---- the weights ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a0", [0.1, 0.25, 1e-3, 0.0])
def test_power_zero_is_the_unweighted_model_exactly(a0):
    from pda_amd import ops
    for counts in (zipf_counts(), np.zeros(49, dtype=np.int64), np.arange(7)):
        h = ops.ials_item_weight_arrays(counts, 0.0, a0)
        assert h["scale"].dtype == np.float32 and h["alpha_row"].dtype == np.float32 and h["w"].dtype == np.float64
        assert (h["scale"] == np.float32(1.0)).all() and (h["w"] == 1.0).all()
        assert (h["alpha_row"] == np.float32(a0)).all()
        r = wr.item_weights(counts, 0.0, a0)
        assert (r["s"] == 1).all() and (r["w"] == 1).all() and (r["alpha_row"] == np.float32(a0)).all()


@pytest.mark.parametrize("beta", [0.25, 0.5, 1.0, 2.0, 4.0])
def test_the_weights_follow_the_stated_formulas_and_their_mean_is_one(beta):
    from pda_amd import ops
    for counts in (zipf_counts(), wr.bound_counts(), np.array([0, 0, 3, 100000])):
        h = ops.ials_item_weight_arrays(counts, beta, 0.1)
        r = wr.item_weights(counts, beta, 0.1)
        np.testing.assert_array_equal(h["scale"], r["s"])
        np.testing.assert_array_equal(h["w"], r["w"])
        np.testing.assert_array_equal(h["alpha_row"], r["alpha_row"])
        n = len(counts)
        p = [(float(c) + 1.0) ** beta for c in counts]
        s = np.array([np.float32(np.sqrt(n * (v / sum(p)))) for v in p])                    # the formulas, item by item
        np.testing.assert_allclose(h["scale"], s, rtol=2e-7)                                # (sum() adds in another order than numpy's: one ulp)
        np.testing.assert_array_equal(h["w"], h["scale"].astype(np.float64) ** 2)
        np.testing.assert_array_equal(h["alpha_row"], (0.1 * h["w"]).astype(np.float32))
        assert abs(h["w"].mean() - 1.0) < 1e-6
        assert abs(h["q"].sum() - 1.0) < 1e-12 and (np.diff(h["w"][np.argsort(counts, kind="stable")]) >= 0).all()      # popular items weigh more


def test_the_bound_tests_weights_span_what_the_issue_states():
    h = wr.item_weights(wr.bound_counts(), wr.BETA, 0.1)
    assert 0.7 < h["w"].min() < 0.85 and 30 < h["w"].max() < 40 and abs(h["w"].mean() - 1) < 1e-6
    b = wr.bound_inputs(0.1)
    assert b["w_rows"].min() == h["w"].min() and b["w_rows"].max() == h["w"].max() and len(b["alpha_rows"]) == len(ir.ROW_LENGTHS)


def test_bad_weights_are_refused():
    from pda_amd import ops
    for beta in (-0.1, 4.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="item power"):
            ops.ials_item_weight_arrays([1, 2], beta, 0.1)
    with pytest.raises(ValueError, match="alpha0"):
        ops.ials_item_weight_arrays([1, 2], 0.5, -1.0)
    with pytest.raises(ValueError, match="count"):
        ops.ials_item_weight_arrays([1, -2], 0.5, 0.1)
    with pytest.raises(ValueError, match="count"):
        ops.ials_item_weight_arrays([], 0.5, 0.1)


def toy_pairs(seed=3, nu=70, ni=45, n=2500):
    g = np.random.default_rng(seed)
    return g.integers(0, nu - 1, n), np.minimum(g.zipf(1.4, n) - 1, ni - 2), nu, ni


@pytest.mark.parametrize("lam, a0, nu", [(0.05, 0.1, 1.0), (0.01, 1e-3, 0.0), (0.003, 0.7, 0.5)])
def test_the_graph_holds_the_weights_and_the_item_lam_row_of_the_stated_formula(lam, a0, nu):
    import torch
    from pda_amd import ops
    u, i, n_users, n_items = toy_pairs()
    g0 = ops.IalsGraph(u, i, n_users, n_items, "cpu", lam=lam, alpha0=a0, nu=nu)
    assert g0.item_weights is None and g0.item_power == 0.0
    g00 = ops.IalsGraph(u, i, n_users, n_items, "cpu", lam=lam, alpha0=a0, nu=nu, item_power=0.0)
    assert g00.item_weights is None
    np.testing.assert_array_equal(g00.item.host_lam_row, g0.item.host_lam_row)
    g = ops.IalsGraph(u, i, n_users, n_items, "cpu", lam=lam, alpha0=a0, nu=nu, item_power=0.5)
    iw = g.item_weights
    assert isinstance(iw, ops.IalsItemWeights) and iw.power == 0.5
    deg = g.host["item"]["deg"]
    eu, ei = ir.dedup_pairs(u, i, n_items)
    np.testing.assert_array_equal(deg, np.bincount(ei, minlength=n_items))                  # c_i: the DISTINCT train pairs of the item
    r = wr.item_weights(deg, 0.5, a0)
    np.testing.assert_array_equal(iw.w, r["w"])
    np.testing.assert_array_equal(iw.host_scale, r["s"])
    np.testing.assert_array_equal(iw.host_alpha_row, r["alpha_row"])
    assert iw.scale.dtype == torch.float32 and iw.alpha_row.dtype == torch.float32
    np.testing.assert_array_equal(iw.scale.numpy(), r["s"])
    np.testing.assert_array_equal(iw.alpha_row.numpy(), r["alpha_row"])
    want = np.array([np.float32(lam * (float(n) + a0 * wi * n_users) ** nu) for n, wi in zip(deg, iw.w)])
    np.testing.assert_array_equal(g.item.host_lam_row, want)
    np.testing.assert_array_equal(g.item.host_lam_row, wr.lam_row_items(deg, n_users, lam, a0, nu, iw.w))
    np.testing.assert_array_equal(g.user.host_lam_row, g0.user.host_lam_row)                # sum_i alpha0 w_i = alpha0 n_items: the users' is unchanged
    np.testing.assert_array_equal(ops.ials_lam_row_items(deg, n_users, lam, a0, nu, np.ones(n_items)), g0.item.host_lam_row)
    if nu > 0 and a0 > 0:
        assert (g.item.host_lam_row != g0.item.host_lam_row).any()
    for bad in (-1.0, 5.0, float("nan")):
        with pytest.raises(ValueError, match="item power"):
            ops.IalsGraph(u, i, n_users, n_items, "cpu", lam=lam, alpha0=a0, nu=nu, item_power=bad)


# ---- the flag, its refusals, the state dict ----------------------------------------------------------------------------------------------------
def test_the_flag_parses_defaults_to_zero_and_is_an_extension():
    from pda_amd import parse
    from pda_amd.model_api import check_ials
    assert parse.parse_args([]).ials_item_power == 0.0
    b = parse.parse_args("--train ials --ials_item_power 0.5".split())
    assert b.ials_item_power == 0.5
    check_ials(b)
    ext = {f[0]: f[3] for f in parse._EXTENSION_FLAGS}
    assert "ials_item_power" in ext and "ials_item_power" not in parse.reference_flag_names()
    assert "0 .. 4" in ext["ials_item_power"] and "bit for bit" in ext["ials_item_power"]
    for over in ({"ials_item_power": 0.0}, {"ials_item_power": 4.0}, {"ials_item_power": 0.5, "ials_solver": "block", "embed_size": 256},
                 {"ials_item_power": 1.0, "test": "ials"}):
        check_ials(make_args(**over))
    for train in ("normal", "s_condition", "ssm"):                                          # nothing to refuse for any other trainer
        check_ials(make_args(train=train, test="normal", ials_item_power=-3.0))


@pytest.mark.parametrize("beta", [-0.01, 4.01, float("nan"), float("inf"), -float("inf")])
def test_values_outside_zero_to_four_are_value_errors_that_name_the_flag(beta):
    from pda_amd.model_api import check_ials
    with pytest.raises(ValueError, match="--ials_item_power"):
        check_ials(make_args(ials_item_power=beta))
    with pytest.raises(ValueError, match="--ials_item_power"):
        check_ials(make_args(ials_item_power=beta, ials_solver="block"))


def model(capsys=None, **over):
    from pda_amd.model_api import IALSMF, gcn_train_pairs
    u, i, nu, ni = toy_pairs()
    lists = {int(x): [] for x in range(nu)}
    for a, b in zip(u.tolist(), i.tolist()):
        lists[a].append(b)
    return IALSMF(make_args(verbose=0, **over), {"n_users": nu, "n_items": ni, "gcn_train_pairs": gcn_train_pairs(lists)}, device="cpu")


def test_the_state_dict_carries_the_key_only_when_the_power_is_not_zero(capsys):
    m0 = model()
    out0 = capsys.readouterr().out
    assert "ials_item_power" not in m0.state_dict() and "ials item_power" not in out0 and m0.graph.item_weights is None
    m = model(ials_item_power=0.5)
    out = capsys.readouterr().out
    sd = m.state_dict()
    assert sd["ials_item_power"] == 0.5 and sd["optimizer"] == "ials" and set(sd) - set(m0.state_dict()) == {"ials_item_power"}
    assert not any(k in sd for k in ("w", "scale", "alpha_row"))                            # rebuilt from the train pairs, never stored
    line = re.search(r"^\|\|--- ials item_power=(\S+) w_min=(\S+) w_max=(\S+)$", out, flags=re.M)
    assert line and float(line.group(1)) == 0.5 and out.count("ials item_power") == 1
    w = m.graph.item_weights.w
    assert abs(float(line.group(2)) - w.min()) <= 1e-5 * w.min() and abs(float(line.group(3)) - w.max()) <= 1e-5 * w.max()
    mb = model(ials_item_power=0.5, ials_solver="block", embed_size=64)
    assert {"ials_item_power", "ials_solver", "ials_block"} <= set(mb.state_dict())
    assert "ials_item_power" not in model(ials_solver="block", embed_size=64).state_dict()


def test_the_run_directory_suffix_stays_ials():
    src = open(os.path.join(ROOT, "pda_amd", "train_new_api.py")).read() + open(os.path.join(ROOT, "pda_amd", "export_topk.py")).read()
    assert "item_power" not in src and "itemw" not in src                                   # the trainer and the exporter name their directories as before


# ---- the binding and the argument checks ---------------------------------------------------------------------------------------------------
def test_the_binding_equals_the_header():
    from pda_amd import _lib
    lib = _lib.load()
    assert declared_in("pda_hip_ials_itemw.h") == sorted(_lib.IALS_ITEMW_SIGNATURES) == NAMES
    others = [v for k, v in vars(_lib).items() if k.endswith("SIGNATURES") and k != "IALS_ITEMW_SIGNATURES"]
    assert len(others) >= 21
    for d in others:
        assert not set(NAMES) & set(d)
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "pda_hip_ials_itemw.h":
            assert not set(NAMES) & set(declared_in(h)), h
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pda_hip_ials_itemw.h")).read(), flags=re.S)
    for n in NAMES:
        assert getattr(lib, n).argtypes == _lib.IALS_ITEMW_SIGNATURES[n][1] and getattr(lib, n).restype is C.c_int
        params = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert len(params.split(",")) == len(_lib.IALS_ITEMW_SIGNATURES[n][1]), n
    # the arguments are those of the unweighted entry points with a pointer where the scalar alpha0 stood
    for new, old, sigs in (("pda_ials_half_sweep_rowalpha_f32", "pda_ials_half_sweep_f32", _lib.IALS_SIGNATURES),
                           ("pda_ialspp_block_pass_rowalpha_f32", "pda_ialspp_block_pass_f32", _lib.IALSPP_SIGNATURES)):
        a, b = _lib.IALS_ITEMW_SIGNATURES[new][1], sigs[old][1]
        assert len(a) == len(b) and [x for x, y in zip(a, b) if x is not y] == [C.c_void_p] and [y for x, y in zip(a, b) if x is not y] == [C.c_float]


@pytest.fixture(scope="module")
def entry_points():
    """name -> call(**what differs from a sound call); distinct non-null addresses stand for the buffers (never dereferenced)."""
    from pda_amd import _lib
    lib = _lib.load()
    keep = C.create_string_buffer(4096)
    b, c, g, e, al = (C.c_void_p(C.addressof(keep) + 64 * k) for k in range(5))
    big = 1 << 30

    def gram(Z=b, scale=al, n=9, d=256, G=g, ws=c, ws_floats=big):
        return lib.pda_ials_gram_scaled_f32(Z, scale, n, d, G, ws, ws_floats, NULL)

    def gram256(Z=b, scale=al, n=9, G=g, ws=c, ws_floats=big):
        return lib.pda_ialspp_gram256_scaled_f32(Z, scale, n, G, ws, ws_floats, NULL)

    def sweep(indptr=b, indices=b, n_rows=9, nnz=20, work=b, n_work=9, long_rows=NULL, n_long=0, n_slots=0, Z=b, n_z=12, G=g, d=64, alpha_row=al,
              lam_row=b, X=c, fail=b, dbg=NULL, ws=NULL, ws_bytes=0):
        return lib.pda_ials_half_sweep_rowalpha_f32(indptr, indices, n_rows, nnz, work, n_work, long_rows, n_long, n_slots, Z, n_z, G, d, alpha_row,
                                                    lam_row, X, fail, dbg, ws, ws_bytes, NULL)

    def bpass(indptr=b, indices=b, perm=NULL, n_rows=9, nnz=20, work=b, n_work=9, long_rows=NULL, n_long=0, n_slots=0, Z=b, n_z=12, G=g, d=64, k=32,
              p0=32, alpha_row=al, lam_row=b, X=c, e=e, fail=b, dbg=NULL, slots=NULL, slot_floats=0, delta=NULL, delta_floats=0):
        return lib.pda_ialspp_block_pass_rowalpha_f32(indptr, indices, perm, n_rows, nnz, work, n_work, long_rows, n_long, n_slots, Z, n_z, G, d, k, p0,
                                                      alpha_row, lam_row, X, e, fail, dbg, slots, slot_floats, delta, delta_floats, NULL)

    yield {"gram": gram, "gram256": gram256, "sweep": sweep, "pass": bpass}, b, c, g, e, al
    del keep


def test_every_argument_error_comes_back_before_any_launch(entry_points):
    eps, b, c, g, e, al = entry_points
    gram, gram256, sweep, bpass = eps["gram"], eps["gram256"], eps["sweep"], eps["pass"]
    for fn in (gram, gram256):
        for arg in ("Z", "scale", "G", "ws"):
            assert fn(**{arg: NULL}) == ERR_ARG, arg
        assert fn(n=0) == ERR_ARG and fn(n=1 << 31) == ERR_ARG and fn(G=b) == ERR_ARG and fn(G=al) == ERR_ARG
        assert fn(n=257, ws_floats=2 * (256 * 256 + 256) - 1) == ERR_ARG
    assert gram(n=257, d=64, ws_floats=2 * (64 * 64 + 64) - 1) == ERR_ARG and gram(n=256, d=32, ws_floats=32 * 32 + 31) == ERR_ARG
    for d in (16, 48, 512, 0):
        assert gram(d=d) == ERR_UNSUPPORTED, d
    assert gram(d=48, n=0) == ERR_ARG and gram(d=48, scale=NULL) == ERR_ARG                  # (the argument errors come first)

    for arg in ("indptr", "indices", "work", "Z", "G", "alpha_row", "lam_row", "X", "fail"):
        assert sweep(**{arg: NULL}) == ERR_ARG, arg
    assert sweep(n_rows=0) == ERR_ARG and sweep(n_z=0) == ERR_ARG and sweep(n_work=0) == ERR_ARG and sweep(n_rows=1 << 31) == ERR_ARG
    assert sweep(X=b) == ERR_ARG and sweep(X=g) == ERR_ARG and sweep(X=al) == ERR_ARG
    assert sweep(n_long=1, n_slots=2) == ERR_ARG and sweep(n_slots=2) == ERR_ARG
    assert sweep(long_rows=b, n_long=1, n_slots=1, ws=c, ws_bytes=1 << 30) == ERR_ARG         # at least two chunks
    assert sweep(long_rows=b, n_long=1, n_slots=2, n_work=10) == ERR_ARG                    # slots without a workspace
    assert sweep(long_rows=b, n_long=1, n_slots=2, n_work=10, ws=c, ws_bytes=2 * (64 * 64 + 64) * 4 - 1) == ERR_ARG
    for d in (16, 48, 256, 0):
        assert sweep(d=d) == ERR_UNSUPPORTED, d
    assert sweep(d=256, alpha_row=NULL) == ERR_ARG

    for arg in ("indptr", "indices", "work", "Z", "G", "alpha_row", "lam_row", "X", "e", "fail"):
        assert bpass(**{arg: NULL}) == ERR_ARG, arg
    assert bpass(n_rows=0) == ERR_ARG and bpass(n_z=0) == ERR_ARG and bpass(n_work=0) == ERR_ARG
    assert bpass(X=b) == ERR_ARG and bpass(X=g) == ERR_ARG and bpass(X=al) == ERR_ARG and bpass(e=c) == ERR_ARG and bpass(e=al) == ERR_ARG
    assert bpass(n_long=1, n_slots=2) == ERR_ARG and bpass(n_slots=2) == ERR_ARG
    sound = dict(long_rows=b, n_long=1, n_slots=2, n_work=10, slots=c, delta=g)
    assert bpass(slot_floats=2 * (32 * 32 + 32) - 1, delta_floats=64, **sound) == ERR_ARG and bpass(slot_floats=2 * (32 * 32 + 32), delta_floats=63, **sound) == ERR_ARG
    for d, k in ((48, 32), (512, 64), (64, 16), (256, 256)):
        assert bpass(d=d, k=k, p0=0) == ERR_UNSUPPORTED, (d, k)
    assert bpass(d=32, k=64, p0=0) == ERR_ARG and bpass(p0=-32) == ERR_ARG and bpass(p0=64) == ERR_ARG and bpass(p0=16) == ERR_ARG
    assert bpass(k=16, alpha_row=NULL) == ERR_ARG


def test_ops_refuses_bad_vectors_before_the_library():
    import torch
    from pda_amd import ops
    with pytest.raises(ValueError, match="HBM"):
        ops.ials_gram(torch.zeros(9, 64), scale=torch.ones(9))
    u, i, nu, ni = toy_pairs()
    g = ops.IalsGraph(u, i, nu, ni, "cpu", lam=0.05)
    with pytest.raises(ValueError, match="HBM"):
        ops.ials_half_sweep(g, "item", torch.zeros(nu, 32), torch.zeros(ni, 32), alpha_row=torch.ones(ni))


# ---- the restatement's own properties ------------------------------------------------------------------------------------------------------------
def toy(seed=5, nu=6, ni=5, d=4):
    g = np.random.default_rng(seed)
    eu, ei = ir.dedup_pairs(g.integers(0, nu, 14), g.integers(0, ni, 14), ni)
    X, Y = g.standard_normal((nu, d)) * 0.4, g.standard_normal((ni, d)) * 0.4
    up, ui = ir.csr(eu, ei, nu)
    ip, ii = ir.csr(ei, eu, ni)
    return eu, ei, X, Y, up, ui, ip, ii


@pytest.mark.parametrize("a0, lam, nu, beta", [(0.25, 0.05, 1.0, 0.5), (0.5, 1e-3, 0.0, 1.0), (0.1, 0.1, 0.5, 2.0), (0.25, 0.05, 1.0, 0.0)])
def test_every_row_solution_zeroes_the_float64_gradient_of_the_stated_objective(a0, lam, nu, beta):
    """L as the issue writes it, by autograd on a toy graph.  The gradient of each side is taken at the weights that side is handed: the user
    side's alpha32(alpha0) s_i^2 and the item side's alpha_row[i] = fl32(alpha0 w_i) differ by one rounding of fp32 (w = s^2 has up to 48
    significant bits), which the assertion on their distance states."""
    import torch
    eu, ei, X, Y, up, ui, ip, ii = toy()
    n_users, n_items = X.shape[0], Y.shape[0]
    iw = wr.item_weights(np.diff(ip), beta, a0)
    lu = ir.lam_row(np.diff(up), n_items, lam, a0, nu)
    li = wr.lam_row_items(np.diff(ip), n_users, lam, a0, nu, iw["w"])
    a_user, a_item = wr.user_item_alpha(a0, iw["s"]), wr.item_alpha(iw["alpha_row"])
    np.testing.assert_allclose(a_user, a_item, rtol=2.0 ** -23)

    def L(Xt, Yt, a):
        s = (Xt[eu] * Yt[ei]).sum(1)
        return ((s - 1) ** 2).sum() + (torch.from_numpy(a) * (Xt @ Yt.T) ** 2).sum() + (torch.from_numpy(lu.astype(np.float64)) * (Xt * Xt).sum(1)).sum() \
            + (torch.from_numpy(li.astype(np.float64)) * (Yt * Yt).sum(1)).sum()

    np.testing.assert_allclose(L(torch.from_numpy(X), torch.from_numpy(Y), a_user).item(), wr.objective(X, Y, eu, ei, a_user, lu, li)[0], rtol=1e-13)
    X1 = wr.user_half_sweep(up, ui, Y, iw["s"], a0, lu)
    Xt, Yt = torch.from_numpy(X1).requires_grad_(), torch.from_numpy(Y).requires_grad_()
    gX, = torch.autograd.grad(L(Xt, Yt, a_user), Xt)
    assert gX.abs().max().item() < 1e-12                                                    # the user rows sit at their minimiser
    Y1 = wr.item_half_sweep(ip, ii, X1, iw["alpha_row"], li)
    Xt, Yt = torch.from_numpy(X1).requires_grad_(), torch.from_numpy(Y1).requires_grad_()
    gY, = torch.autograd.grad(L(Xt, Yt, a_item), Yt)
    assert gY.abs().max().item() < 1e-12
    # a block step at k = d from any start is the same minimiser, on both sides
    Xb, _ = wr.block_pass(X * 3.0, pr.predictions(X * 3.0, Y, up, ui), up, ui, None, Y, a0, lu, 0, X.shape[1], scale=iw["s"])
    np.testing.assert_allclose(Xb, X1, atol=1e-11)
    perm = pr.pair_perm(up, ui, ip, ii)
    Yb, _ = wr.block_pass(Y * 3.0, pr.predictions(X1, Y * 3.0, up, ui), ip, ii, perm, X1, iw["alpha_row"], li, 0, X.shape[1])
    np.testing.assert_allclose(Yb, Y1, atol=1e-11)
    if beta == 0.0:                                                                         # the unweighted restatement, to the last bit of float64
        np.testing.assert_array_equal(X1, ir.half_sweep(up, ui, Y, a0, lu))
        np.testing.assert_array_equal(Y1, ir.half_sweep(ip, ii, X1, a0, ir.lam_row(np.diff(ip), n_users, lam, a0, nu)))


def test_an_epoch_of_either_solver_never_raises_the_weighted_objective():
    u, i, nu, ni = toy_pairs()
    eu, ei = ir.dedup_pairs(u, i, ni)
    up, ui = ir.csr(eu, ei, nu)
    ip, ii = ir.csr(ei, eu, ni)
    g = np.random.default_rng(1)
    a0, lam, nuu = 0.25, 0.05, 1.0
    iw = wr.item_weights(np.diff(ip), 0.5, a0)
    lu, li = ir.lam_row(np.diff(up), ni, lam, a0, nuu), wr.lam_row_items(np.diff(ip), nu, lam, a0, nuu, iw["w"])
    a = wr.user_item_alpha(a0, iw["s"])             # the item side solves at weights one fp32 rounding away: a second-order 1e-15 of the objective
    X, Y = g.standard_normal((nu, 8)) * 0.3, g.standard_normal((ni, 8)) * 0.3
    last = wr.objective(X, Y, eu, ei, a, lu, li)[0]
    for _ in range(3):
        X1, Y1 = wr.epoch(X, Y, up, ui, ip, ii, a0, iw["s"], iw["alpha_row"], lu, li)
        mid, now = wr.objective(X1, Y, eu, ei, a, lu, li)[0], wr.objective(X1, Y1, eu, ei, a, lu, li)[0]
        assert mid <= last * (1 + 1e-13) and now <= mid * (1 + 1e-13)
        X, Y, last = X1, Y1, now
    assert (X[-1] == 0).all() and (Y[-1] == 0).all()
    for _ in range(2):
        X, Y, e = wr.block_epoch(X, Y, up, ui, ip, ii, a0, iw["s"], iw["alpha_row"], lu, li, 4)
        now = wr.objective(X, Y, eu, ei, a, lu, li)[0]
        assert now <= last * (1 + 1e-13)
        last = now
        np.testing.assert_allclose(e, pr.predictions(X, Y, up, ui), atol=1e-12)
    # the weighting changes the solution: the unweighted epoch from the same tables lands elsewhere
    X0, _ = ir.epoch(X, Y, up, ui, ip, ii, a0, lu, ir.lam_row(np.diff(ip), nu, lam, a0, nuu))
    X1, _ = wr.epoch(X, Y, up, ui, ip, ii, a0, iw["s"], iw["alpha_row"], lu, li)
    assert np.abs(X0 - X1).max() > 1e-3


def test_the_exact_tests_inputs_are_exact_in_fp32_whatever_the_order():
    """Eighths tables scaled by 1/2, 1 or 2 are tables of sixteenths with |z'| <= 1: every product is a multiple of 1/256 and the Gram
    matrix of N_OTHER rows stays below 2^24 grid units even as a sum of absolute values, so every order gives the exact sum; alpha in powers
    of two keeps fl(alpha G) exact and the row systems follow."""
    n = 600
    Z, s = ir.eighths_table(n, 32, 2), wr.pow2_scale(n)
    assert set(np.unique(s)) == {0.5, 1.0, 2.0} and set(np.unique(wr.pow2_alpha(n))) == {0.25, 0.5, 1.0}
    Zs = wr.scaled32(Z, s)
    np.testing.assert_array_equal(Zs.astype(np.float64), Z.astype(np.float64) * s.astype(np.float64)[:, None])
    np.testing.assert_array_equal(wr.gram_scaled32(Z, s).astype(np.float64), wr.gram_w(Z, s))
    assert ir.N_OTHER * 1.0 * 256 < 2 ** 24
    rows, cols = ir.length_graph(lengths=(0, 1, 33, 300, 2 * 256 + 5), n_other=n)
    ip, ix = ir.csr(rows, cols, 5)
    lam = np.array([0.5, 1.25, 3.0, 0.75, 2.5], dtype=np.float32)
    Gw32, G32 = wr.gram_scaled32(Z, s), ir.gram32(Z)
    al = wr.pow2_alpha(5)
    for r in range(5):
        A32, b32 = ir.normal32(ip, ix, Z, Gw32, 0.25, lam, r, chunk=256)                    # the user side: the scalar against G_w
        A, b = ir.normal_equations(ip, ix, Z, 0.25, lam, r, wr.gram_w(Z, s))
        np.testing.assert_array_equal(A32.astype(np.float64), A)
        np.testing.assert_array_equal(b32.astype(np.float64), b)
        A32, b32 = wr.normal32(ip, ix, Z, G32, al, lam, r, chunk=256)                       # the item side: the row's alpha against G
        A, b = ir.normal_equations(ip, ix, Z, float(al[r]), lam, r)
        np.testing.assert_array_equal(A32.astype(np.float64), A)
        np.testing.assert_array_equal(b32.astype(np.float64), b)
    # the sizes of the GPU test: |z'| <= 1, |z| <= 1/2, alpha <= 1, lam <= 8, on the grid 1 / 1024 of alpha0 G_w
    c = 2 * ir.CHUNK + 5
    assert (c * 0.25 + 1.0 * ir.N_OTHER * 1.0 + 8.0) * 1024 < 2 ** 24


@pytest.mark.parametrize("d", [32, 64, 128])
def test_the_bound_tests_inputs_keep_kappa_eta_below_a_tenth_on_both_sides(d):
    rows, cols = ir.length_graph()
    ip, ix = ir.csr(rows, cols, len(ir.ROW_LENGTHS))
    nr = len(ir.ROW_LENGTHS)
    worst = 0.0
    for kind in ir.TABLES:
        Z = ir.table(kind, ir.N_OTHER, d)
        for a0, lam, nu in ir.PARAMS:
            b = wr.bound_inputs(a0)
            o = wr.row_bounds(ip, ix, Z, a0, ir.lam_row(np.diff(ip), ir.N_OTHER, lam, a0, nu), range(nr), scale=b["s"])
            assert (o["kappa"] * o["eta"]).max() < 0.1, ("user", kind, a0, lam, nu, (o["kappa"] * o["eta"]).max())
            assert (o["x"][0] == 0).all() and np.isfinite(o["bound"]).all()
            li = wr.lam_row_items(np.diff(ip), ir.N_OTHER, lam, a0, nu, b["w_rows"])
            o2 = wr.row_bounds(ip, ix, Z, b["alpha_rows"], li, range(nr))
            assert (o2["kappa"] * o2["eta"]).max() < 0.1, ("item", kind, a0, lam, nu, (o2["kappa"] * o2["eta"]).max())
            assert (o2["x"][0] == 0).all() and np.isfinite(o2["bound"]).all()
            worst = max(worst, (o["kappa"] * o["eta"]).max(), (o2["kappa"] * o2["eta"]).max())
    print("item-weighted kappa eta max at d=%d: %.3g" % (d, worst))


def test_the_bounds_fall_back_to_the_unweighted_ones_without_weights():
    rows, cols = ir.length_graph(lengths=(0, 1, 33, 90), n_other=120)
    ip, ix = ir.csr(rows, cols, 4)
    Z = ir.table("gauss0.3", 120, 32)
    lam = ir.lam_row(np.diff(ip), 120, 0.05, 0.1, 1.0)
    a, b = ir.row_bounds(ip, ix, Z, 0.1, lam, range(4)), wr.row_bounds(ip, ix, Z, 0.1, lam, range(4))
    for key in ("kappa", "eta", "bound", "xnorm", "lmax", "x"):
        np.testing.assert_allclose(a[key], b[key], rtol=1e-12)
    c = wr.row_bounds(ip, ix, Z, 0.1, lam, range(4), scale=np.ones(120, dtype=np.float32))
    assert (c["eta"] >= a["eta"]).all() and (c["eta"] <= a["eta"] * 1.01).all()            # the scale's two roundings, nothing else
    X = ir.table("gauss0.3", 4, 32, seed=5)
    e = pr.predictions(X, Z, ip, ix).astype(np.float32)
    p, q = pr.pass_bounds(X, e, ip, ix, None, Z, 0.1, lam, 0, 32), wr.pass_bounds(X, e, ip, ix, None, Z, 0.1, lam, 0, 32)
    for key in ("X", "e", "dX", "de", "err"):
        np.testing.assert_allclose(p[key], q[key], rtol=1e-12)
    q2 = wr.pass_bounds(X, e, ip, ix, None, Z, 0.1, lam, 0, 32, scale=np.ones(120, dtype=np.float32))
    assert (q2["dX"] >= p["dX"]).all() and (q2["dX"] <= p["dX"] * 1.01).all()
