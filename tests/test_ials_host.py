"""CPU suite for the iALS baseline (`--train ials`, include/pda_hip_ials.h): the flags, the refusals of check_ials, the binding against the
header, the entry points' argument checks (every call carries a violation, so none reaches a launch), the work lists, and the properties of
the restatement tests/ials_ref.py that the GPU suite leans on: the row solution zeroes the gradient, a half-sweep never raises the objective,
the exact test's inputs are exact in fp32 whatever the order, and kappa eta < 0.1 on every row of the parity test."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ials_ref as ir
from test_abi import declared_in

ERR_ARG, ERR_UNSUPPORTED = -1, -2
NULL = C.c_void_p(None)
NAMES = ["pda_ials_gram_f32", "pda_ials_half_sweep_f32", "pda_ials_loss_f32", "pda_ials_workspace_bytes"]


def make_args(**over):
    from pda_amd.parse import parse_args
    a = parse_args(["--train", "ials", "--embed_size", "32", "--regs", "0.05"])
    for k, v in over.items():
        setattr(a, k, v)
    return a


# ---- flags and refusals --------------------------------------------------------------------------------------------------------------------
def test_flags_parse_and_the_defaults_leave_every_other_train_untouched():
    from pda_amd import parse
    from pda_amd.model_api import check_ials
    a = parse.parse_args([])
    assert (a.ials_alpha0, a.ials_nu, a.train) == (0.1, 1.0, "normal")
    for train in ("normal", "s_condition", "temp_pop", "dice", "ips", "macr", "ssm"):      # nothing to refuse, whatever else is set
        check_ials(make_args(train=train, test="normal", model="lightgcn", table_dtype="bf16", gpus=4, embed_size=256, regs=0.0, ials_nu=7.0))
    b = parse.parse_args("--train ials --test ials --ials_alpha0 0.5 --ials_nu 0.25".split())
    assert (b.train, b.test, b.ials_alpha0, b.ials_nu) == ("ials", "ials", 0.5, 0.25)
    ext = [f[0] for f in parse._EXTENSION_FLAGS]
    assert {"ials_alpha0", "ials_nu"} <= set(ext) and not set(ext) & set(parse.reference_flag_names())
    helps = {f[0]: f[3] for f in parse._REFERENCE_FLAGS}
    assert "ials" in helps["train"] and "ials" in helps["test"]
    unused = {f[0]: f[3] for f in parse._EXTENSION_FLAGS}["ials_alpha0"]
    for flag in ("--lr", "--optimizer", "--batch_size", "--sampler", "--adam_sweep"):
        assert flag in unused and "unused" in unused


REFUSED = [({"model": "lightgcn"}, "--model"), ({"table_dtype": "bf16"}, "--table_dtype"), ({"gpus": 2}, "--gpus"),
           ({"neg_sampler": "dns"}, "--neg_sampler"), ({"embed_size": 256}, "--embed_size"), ({"embed_size": 16}, "--embed_size"),
           ({"embed_size": 48}, "--embed_size"), ({"test": "s_condition"}, "--test"), ({"test": "macr"}, "--test"), ({"test": "ips"}, "--test"),
           ({"train": "normal", "test": "ials"}, "--test ials")]
BAD_VALUES = [({"regs": 0.0}, "--regs"), ({"regs": -1e-3}, "--regs"), ({"regs": float("nan")}, "--regs"), ({"ials_alpha0": -0.1}, "--ials_alpha0"),
              ({"ials_alpha0": float("inf")}, "--ials_alpha0"), ({"ials_nu": -0.01}, "--ials_nu"), ({"ials_nu": 1.5}, "--ials_nu"),
              ({"ials_nu": float("nan")}, "--ials_nu")]


@pytest.mark.parametrize("over, flag", REFUSED)
def test_refused_options_name_their_flag(over, flag):
    from pda_amd.model_api import check_ials
    with pytest.raises(NotImplementedError, match=flag):
        check_ials(make_args(**over))


@pytest.mark.parametrize("over, flag", BAD_VALUES)
def test_bad_values_are_value_errors_that_name_their_flag(over, flag):
    from pda_amd.model_api import check_ials
    with pytest.raises(ValueError, match=flag):
        check_ials(make_args(**over))


@pytest.mark.parametrize("over", [{}, {"test": "ials"}, {"deterministic": 1}, {"optimizer": "sgd"}, {"lr": 0.0}, {"sampler": "host"},
                                  {"adam_sweep": "replay"}, {"embed_size": 64}, {"embed_size": 128}, {"ials_alpha0": 0.0}, {"ials_nu": 0.0},
                                  {"batch_size": 1}])
def test_what_ials_goes_with_is_let_through(over):
    from pda_amd.model_api import check_ials
    check_ials(make_args(**over))


def test_the_trainer_refuses_before_anything_is_built(monkeypatch):
    from pda_amd import train_new_api as t
    monkeypatch.setattr(t, "data", None, raising=False)
    for over, exc, msg in (({"table_dtype": "bf16"}, NotImplementedError, "--table_dtype"), ({"ials_nu": 2.0}, ValueError, "--ials_nu"),
                           ({"train": "normal", "test": "ials"}, NotImplementedError, "--test ials")):
        monkeypatch.setattr(t, "configure", lambda argv=None, over=over: setattr(t, "args", make_args(**over)))
        monkeypatch.setattr(t, "Ks", [20], raising=False)
        with pytest.raises(exc, match=msg):
            t.main([])


# ---- the binding and the argument checks ---------------------------------------------------------------------------------------------------
def test_the_library_loads_and_the_binding_equals_the_header():
    from pda_amd import _lib, ops
    lib = _lib.load()
    assert declared_in("pda_hip_ials.h") == sorted(_lib.IALS_SIGNATURES) == NAMES
    for d in (_lib.SIGNATURES, _lib.TEMP_POP_SIGNATURES, _lib.PC_SIGNATURES, _lib.DET_SIGNATURES, _lib.DEEP_SIGNATURES, _lib.XQUAD_SIGNATURES,
              _lib.DICE_SIGNATURES, _lib.IPS_SIGNATURES, _lib.MACR_SIGNATURES, _lib.GCN_SIGNATURES, _lib.EXPOSURE_SIGNATURES, _lib.SSM_SIGNATURES,
              _lib.INBATCH_SIGNATURES, _lib.DNS_SIGNATURES):
        assert not set(NAMES) & set(d)
    assert not set(NAMES) & (set(declared_in("pda_hip.h")) | set(declared_in("pda_hip_experimental.h")))
    for n in NAMES:
        assert getattr(lib, n).argtypes == _lib.IALS_SIGNATURES[n][1]
        assert getattr(lib, n).restype is (C.c_size_t if n.endswith("_bytes") else C.c_int)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pda_hip_ials.h")).read(),
                  flags=re.S)
    for n in NAMES:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert len(params.split(",")) == len(_lib.IALS_SIGNATURES[n][1]), n
    assert _lib.IALS_CHUNK == ops.IALS_CHUNK == ir.CHUNK == int(re.search(r"#define PDA_IALS_CHUNK (\d+)", text).group(1))
    assert _lib.IALS_GRAM_ROWS == ops.IALS_GRAM_ROWS == ir.GRAM_ROWS == int(re.search(r"#define PDA_IALS_GRAM_ROWS (\d+)", text).group(1))
    for d in (32, 64, 128):
        assert lib.pda_ials_workspace_bytes(3, d) == 3 * (d * d + d) * 4 and lib.pda_ials_workspace_bytes(0, d) == 0
    assert lib.pda_ials_workspace_bytes(3, 256) == 0 and lib.pda_ials_workspace_bytes(3, 48) == 0


@pytest.fixture(scope="module")
def entry_points():
    """name -> call(**what differs from a sound call); distinct non-null addresses stand for the buffers (never dereferenced)."""
    from pda_amd import _lib
    lib = _lib.load()
    keep = C.create_string_buffer(4096)
    b, c, g = (C.c_void_p(C.addressof(keep) + 64 * k) for k in range(3))
    big = 1 << 30

    def gram(Z=b, n=9, d=32, G=g, ws=c, ws_bytes=big):
        return lib.pda_ials_gram_f32(Z, n, d, G, ws, ws_bytes, NULL)

    def sweep(indptr=b, indices=b, n_rows=9, nnz=20, work=b, n_work=9, long_rows=NULL, n_long=0, n_slots=0, Z=b, n_z=12, G=g, d=32, alpha0=0.1,
              lam_row=b, X_out=c, fail=b, dbg=NULL, ws=NULL, ws_bytes=0):
        return lib.pda_ials_half_sweep_f32(indptr, indices, n_rows, nnz, work, n_work, long_rows, n_long, n_slots, Z, n_z, G, d, alpha0, lam_row, X_out,
                                           fail, dbg, ws, ws_bytes, NULL)

    def loss(indptr=b, indices=b, n_rows=9, nnz=20, X=c, Z=b, n_z=12, G=g, d=32, lam_row=b, out=c):
        return lib.pda_ials_loss_f32(indptr, indices, n_rows, nnz, X, Z, n_z, G, d, lam_row, out, NULL)

    yield {"gram": gram, "sweep": sweep, "loss": loss}, b, c, g
    del keep


def test_every_argument_error_comes_back_before_any_launch(entry_points):
    eps, b, c, g = entry_points
    gram, sweep, loss = eps["gram"], eps["sweep"], eps["loss"]
    for arg in ("Z", "G", "ws"):
        assert gram(**{arg: NULL}) == ERR_ARG, arg
    assert gram(n=0) == ERR_ARG and gram(n=1 << 31) == ERR_ARG
    assert gram(n=257, ws_bytes=2 * (32 * 32 + 32) * 4 - 1) == ERR_ARG                    # two blocks of rows: two slots
    for d in (16, 48, 256, 0):
        assert gram(d=d) == ERR_UNSUPPORTED and sweep(d=d) == ERR_UNSUPPORTED and loss(d=d) == ERR_UNSUPPORTED, d
    assert gram(d=256, n=0) == ERR_ARG and sweep(d=256, n_work=0) == ERR_ARG              # (the argument errors come first)

    for arg in ("indptr", "indices", "work", "Z", "G", "lam_row", "X_out", "fail"):
        assert sweep(**{arg: NULL}) == ERR_ARG, arg
    assert sweep(n_rows=0) == ERR_ARG and sweep(n_z=0) == ERR_ARG and sweep(n_work=0) == ERR_ARG and sweep(n_rows=1 << 31) == ERR_ARG
    assert sweep(alpha0=-0.5) == ERR_ARG and sweep(alpha0=float("nan")) == ERR_ARG and sweep(alpha0=float("inf")) == ERR_ARG
    assert sweep(X_out=b) == ERR_ARG and sweep(X_out=g) == ERR_ARG                          # X_out is neither Z nor G
    assert sweep(n_long=1, n_slots=2) == ERR_ARG                                            # cut rows without their list
    assert sweep(long_rows=b, n_long=1, n_slots=1, ws=c, ws_bytes=1 << 30) == ERR_ARG       # a cut row has at least two chunks
    assert sweep(n_slots=2) == ERR_ARG                                                      # slots without cut rows
    assert sweep(long_rows=b, n_long=1, n_slots=2, n_work=10) == ERR_ARG                    # slots without a workspace
    assert sweep(long_rows=b, n_long=1, n_slots=2, n_work=10, ws=c, ws_bytes=2 * (32 * 32 + 32) * 4 - 1) == ERR_ARG
    assert sweep(long_rows=b, n_long=1, n_slots=12, n_work=9, ws=c, ws_bytes=1 << 30) == ERR_ARG       # fewer entries than chunks
    assert sweep(long_rows=b, n_long=10, n_slots=20, n_work=30, ws=c, ws_bytes=1 << 30) == ERR_ARG     # more cut rows than rows

    for arg in ("indptr", "indices", "X", "Z", "G", "lam_row", "out"):
        assert loss(**{arg: NULL}) == ERR_ARG, arg
    assert loss(n_rows=0) == ERR_ARG and loss(n_z=0) == ERR_ARG and loss(n_z=1 << 31) == ERR_ARG


def test_ops_refuses_bad_calls_before_the_library():
    import torch
    from pda_amd import ops
    with pytest.raises(ValueError, match="HBM"):
        ops.ials_gram(torch.zeros(9, 32))
    for kw, what in ((dict(lam=0.0), "lambda"), (dict(lam=1.0, alpha0=-1.0), "alpha0"), (dict(lam=1.0, nu=1.5), "nu")):
        with pytest.raises(ValueError, match=what):
            ops.check_ials_params(kw["lam"], kw.get("alpha0", 0.1), kw.get("nu", 1.0))
    with pytest.raises(ValueError, match="outside the tables"):
        ops.ials_graph_arrays([0, 1], [0, 7], 2, 7)


# ---- the work lists ------------------------------------------------------------------------------------------------------------------------------
def zipf_pairs(seed=3, nu=70, ni=45, n=2500):
    g = np.random.default_rng(seed)
    u, i = g.integers(0, nu - 1, n), np.minimum(g.zipf(1.4, n) - 1, ni - 2)      # the last user and the last item stay without pairs
    return u, i, nu, ni


@pytest.mark.parametrize("chunk", [1, 7, 16, ir.CHUNK])
def test_the_work_lists_cover_every_row_once_and_every_pair_once(chunk):
    from pda_amd import ops
    u, i, nu, ni = zipf_pairs()
    h = ops.ials_graph_arrays(u, i, nu, ni, chunk)
    eu, ei = ir.dedup_pairs(u, i, ni)
    assert h["nnz"] == len(eu) < len(u)                                                     # (duplicates were there, and count once)
    for side, rows, cols, n in (("user", eu, ei, nu), ("item", ei, eu, ni)):
        s = h[side]
        indptr, indices = ir.csr(rows, cols, n)
        np.testing.assert_array_equal(s["indptr"], indptr)
        np.testing.assert_array_equal(s["indices"], indices)
        assert s["indices"].dtype == np.int32 and s["indptr"].dtype == np.int64 and s["deg"][-1] == 0
        work, long_rows, n_slots = ir.work_list(indptr, chunk)
        np.testing.assert_array_equal(s["work"], work)
        np.testing.assert_array_equal(s["long_rows"], long_rows)
        assert s["n_slots"] == n_slots
        seen = np.zeros(len(indices) + 1, dtype=np.int64)
        for r, a, b, slot in s["work"]:
            assert indptr[r] <= a <= b <= indptr[r + 1] and b - a <= chunk
            seen[a:b] += 1
        assert (seen[:-1] == 1).all()                                                       # every pair exactly once
        finished = np.concatenate([s["work"][s["work"][:, 3] < 0, 0], s["long_rows"][:, 0]])
        np.testing.assert_array_equal(np.sort(finished), np.arange(n))                      # every row finished exactly once
        used = np.sort(s["work"][s["work"][:, 3] >= 0, 3])
        np.testing.assert_array_equal(used, np.arange(n_slots))
        for r, s0, k in s["long_rows"]:
            mine = s["work"][s["work"][:, 0] == r]
            assert len(mine) == k >= 2 and (np.diff(mine[:, 1]) > 0).all() and (mine[:, 3] == s0 + np.arange(k)).all()
        assert (np.diff(s["work"][:, 2] - s["work"][:, 1]) <= 0).all()                      # falling length


def test_lam_row_is_rounded_once_from_float64():
    from pda_amd import ops
    deg = np.array([0, 1, 5, 4096, 20000])
    for lam, a0, nu in ir.PARAMS + ((0.003, 0.7, 0.5),):
        got = ops.ials_lam_row(deg, 8232, lam, a0, nu)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, ir.lam_row(deg, 8232, lam, a0, nu))
        np.testing.assert_array_equal(got, np.array([np.float32(lam * (float(n) + a0 * 8232) ** nu) for n in deg]))


# ---- the restatement's own properties ------------------------------------------------------------------------------------------------------------
def toy(seed=5, nu=6, ni=5, d=4):
    g = np.random.default_rng(seed)
    eu, ei = ir.dedup_pairs(g.integers(0, nu, 14), g.integers(0, ni, 14), ni)
    X, Y = g.standard_normal((nu, d)) * 0.4, g.standard_normal((ni, d)) * 0.4
    up, ui = ir.csr(eu, ei, nu)
    ip, ii = ir.csr(ei, eu, ni)
    return eu, ei, X, Y, up, ui, ip, ii


@pytest.mark.parametrize("a0, lam, nu", [(0.25, 0.05, 1.0), (0.5, 1e-3, 0.0), (0.0, 0.1, 0.5)])
def test_the_row_solution_zeroes_the_float64_gradient(a0, lam, nu):
    import torch
    eu, ei, X, Y, up, ui, ip, ii = toy()
    lu, li = ir.lam_row(np.diff(up), 5, lam, a0, nu), ir.lam_row(np.diff(ip), 6, lam, a0, nu)

    def L(Xt, Yt):
        s = (Xt[eu] * Yt[ei]).sum(1)
        return ((s - 1) ** 2).sum() + ir.alpha32(a0) * ((Xt @ Yt.T) ** 2).sum() + (torch.from_numpy(lu.astype(np.float64)) * (Xt * Xt).sum(1)).sum() \
            + (torch.from_numpy(li.astype(np.float64)) * (Yt * Yt).sum(1)).sum()

    np.testing.assert_allclose(L(torch.from_numpy(X), torch.from_numpy(Y)).item(), ir.objective(X, Y, eu, ei, a0, lu, li)[0], rtol=1e-13)
    X1 = ir.half_sweep(up, ui, Y, a0, lu)
    Xt, Yt = torch.from_numpy(X1).requires_grad_(), torch.from_numpy(Y).requires_grad_()
    gX, = torch.autograd.grad(L(Xt, Yt), Xt)
    assert gX.abs().max().item() < 1e-12                                                    # the user rows sit at their minimiser
    Y1 = ir.half_sweep(ip, ii, X1, a0, li)
    Xt, Yt = torch.from_numpy(X1).requires_grad_(), torch.from_numpy(Y1).requires_grad_()
    gY, = torch.autograd.grad(L(Xt, Yt), Yt)
    assert gY.abs().max().item() < 1e-12


def test_a_half_sweep_never_raises_the_objective_and_empty_rows_become_zero():
    u, i, nu, ni = zipf_pairs()
    eu, ei = ir.dedup_pairs(u, i, ni)
    up, ui = ir.csr(eu, ei, nu)
    ip, ii = ir.csr(ei, eu, ni)
    g = np.random.default_rng(1)
    for a0, lam, nuu in ir.PARAMS:
        X, Y = g.standard_normal((nu, 8)) * 0.3, g.standard_normal((ni, 8)) * 0.3
        lu, li = ir.lam_row(np.diff(up), ni, lam, a0, nuu), ir.lam_row(np.diff(ip), nu, lam, a0, nuu)
        last = ir.objective(X, Y, eu, ei, a0, lu, li)[0]
        for _ in range(4):
            X = ir.half_sweep(up, ui, Y, a0, lu)
            mid = ir.objective(X, Y, eu, ei, a0, lu, li)[0]
            Y = ir.half_sweep(ip, ii, X, a0, li)
            now = ir.objective(X, Y, eu, ei, a0, lu, li)[0]
            assert mid <= last * (1 + 1e-13) and now <= mid * (1 + 1e-13)
            last = now
        assert (X[-1] == 0).all() and (Y[-1] == 0).all()


def test_the_exact_test_s_inputs_are_exact_in_fp32_whatever_the_order():
    """Tables of multiples of 1/8, alpha0 in {0.25, 0.5}, dyadic lam_row: every partial sum of the stated order is a multiple of 1/256 below
    2^24 / 256, so the fp32 chain equals exact arithmetic -- and any other order would give the same bits."""
    rows, cols = ir.length_graph(lengths=(0, 1, 33, 300, 2 * 256 + 5), n_other=600)
    ip, ix = ir.csr(rows, cols, 5)
    Z = ir.eighths_table(600, 32, 2)
    lam = np.array([0.5, 1.25, 3.0, 0.75, 2.5], dtype=np.float32)
    G32 = ir.gram32(Z)
    np.testing.assert_array_equal(G32.astype(np.float64), Z.astype(np.float64).T @ Z.astype(np.float64))
    for a0 in (0.25, 0.5):
        for r in range(5):
            A32, b32 = ir.normal32(ip, ix, Z, G32, a0, lam, r, chunk=256)
            A, b = ir.normal_equations(ip, ix, Z, a0, lam, r)
            np.testing.assert_array_equal(A32.astype(np.float64), A)
            np.testing.assert_array_equal(b32.astype(np.float64), b)
    # the sizes of the GPU test: the largest magnitude any partial sum can reach stays exactly representable
    n, c = ir.N_OTHER, 2 * ir.CHUNK + 5
    assert (c * 0.25 + 0.5 * n * 0.25 + 8.0) * 256 < 2 ** 24         # |z| <= 1/2: |z z'| <= 1/4 in units of 1/64, alpha0 G in units of 1/256, lam <= 8


@pytest.mark.parametrize("d", [32, 64, 128])
def test_the_parity_test_s_inputs_keep_kappa_eta_below_a_tenth(d):
    rows, cols = ir.length_graph()
    ip, ix = ir.csr(rows, cols, len(ir.ROW_LENGTHS))
    for kind in ir.TABLES:
        Z = ir.table(kind, ir.N_OTHER, d)
        for a0, lam, nu in ir.PARAMS:
            o = ir.row_bounds(ip, ix, Z, a0, ir.lam_row(np.diff(ip), ir.N_OTHER, lam, a0, nu), range(len(ir.ROW_LENGTHS)))
            assert (o["kappa"] * o["eta"]).max() < 0.1, (kind, a0, lam, nu, (o["kappa"] * o["eta"]).max())
            assert (o["x"][0] == 0).all() and np.isfinite(o["bound"]).all()
