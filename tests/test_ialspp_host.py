"""CPU suite for iALS++ (`--train ials --ials_solver block`, include/pda_hip_ialspp.h): the flags, the new refusals of check_ials,
the binding against the header, the entry points' argument checks (every call carries a violation, so none reaches a launch), pair_perm, and
the properties of the restatement tests/ialspp_ref.py that the GPU suite leans on: repeated block passes are block Gauss-Seidel on the row
systems and converge to the exact half-sweep, k = d is that half-sweep in one step, an epoch never raises the objective, and the exact test's
inputs are exact in fp32 whatever the order."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ials_ref as ir
import ialspp_ref as pr
from test_abi import declared_in

ERR_ARG, ERR_UNSUPPORTED = -1, -2
NULL = C.c_void_p(None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pda_ialspp_block_pass_f32", "pda_ialspp_gram_f32", "pda_ialspp_loss_f32", "pda_ialspp_predict_f32"]


def make_args(**over):
    from pda_amd.parse import parse_args
    a = parse_args(["--train", "ials", "--embed_size", "64", "--regs", "0.05", "--ials_solver", "block"])
    for k, v in over.items():
        setattr(a, k, v)
    return a


# ---- flags and refusals --------------------------------------------------------------------------------------------------------------------
def test_the_flags_default_to_the_exact_solver_and_block_32():
    from pda_amd import parse
    from pda_amd.model_api import IALS_SOLVERS, check_ials
    a = parse.parse_args([])
    assert (a.ials_solver, a.ials_block) == ("exact", 32) and IALS_SOLVERS == ("exact", "block")
    b = parse.parse_args("--train ials --ials_solver block --ials_block 64 --embed_size 256".split())
    assert (b.ials_solver, b.ials_block, b.embed_size) == ("block", 64, 256)
    check_ials(b)
    ext = {f[0]: f[3] for f in parse._EXTENSION_FLAGS}
    assert {"ials_solver", "ials_block"} <= set(ext) and not set(ext) & set(parse.reference_flag_names())
    assert "initialisation" in ext["ials_solver"] and "256" in ext["ials_solver"] and "divide" in ext["ials_block"]
    for train in ("normal", "s_condition", "ssm"):                                          # nothing to refuse for any other trainer
        check_ials(make_args(train=train, test="normal", ials_solver="nonsense", ials_block=7, embed_size=48))


@pytest.mark.parametrize("d, k", [(32, 32), (64, 32), (64, 64), (128, 32), (128, 64), (128, 128), (256, 32), (256, 64), (256, 128)])
def test_every_supported_pair_is_let_through(d, k):
    from pda_amd.model_api import check_ials
    check_ials(make_args(embed_size=d, ials_block=k))
    check_ials(make_args(embed_size=d, ials_block=k, test="ials", deterministic=1))


NEW_REFUSALS = [({"embed_size": 48}, NotImplementedError, "--embed_size"), ({"embed_size": 512}, NotImplementedError, "--embed_size"),
                ({"embed_size": 16}, NotImplementedError, "--embed_size"), ({"ials_block": 16}, ValueError, "--ials_block"),
                ({"ials_block": 48}, ValueError, "--ials_block"), ({"ials_block": 256, "embed_size": 256}, ValueError, "--ials_block"),
                ({"embed_size": 32, "ials_block": 64}, ValueError, "--ials_block"), ({"embed_size": 64, "ials_block": 128}, ValueError, "--ials_block"),
                ({"ials_solver": "cg"}, ValueError, "--ials_solver")]
STILL_REFUSED = [({"model": "lightgcn"}, "--model"), ({"table_dtype": "bf16"}, "--table_dtype"), ({"gpus": 2}, "--gpus"),
                 ({"neg_sampler": "dns"}, "--neg_sampler"), ({"test": "s_condition"}, "--test"), ({"train": "normal", "test": "ials"}, "--test ials")]


@pytest.mark.parametrize("over, exc, flag", NEW_REFUSALS)
def test_every_new_refusal_names_its_flag(over, exc, flag):
    from pda_amd.model_api import check_ials
    with pytest.raises(exc, match=flag):
        check_ials(make_args(**over))


@pytest.mark.parametrize("over, flag", STILL_REFUSED)
def test_what_the_exact_solver_refuses_stays_refused(over, flag):
    from pda_amd.model_api import check_ials
    with pytest.raises(NotImplementedError, match=flag):
        check_ials(make_args(**over))
    with pytest.raises(ValueError, match="--regs"):
        check_ials(make_args(regs=0.0))


def test_the_exact_solver_still_refuses_256_and_its_state_dict_keys_are_those_of_before():
    from pda_amd import ops
    from pda_amd.model_api import check_ials
    with pytest.raises(NotImplementedError, match="--embed_size"):
        check_ials(make_args(ials_solver="exact", embed_size=256))
    check_ials(make_args(ials_solver="exact", embed_size=64, ials_block=48))                # (--ials_block is not looked at by the exact solver)
    assert ops.IALS_EMBED_SIZES == (32, 64, 128) and ops.IALSPP_EMBED_SIZES == (32, 64, 128, 256) == pr.EMBED_SIZES
    assert ops.IALSPP_BLOCK_SIZES == (32, 64, 128) == pr.BLOCK_SIZES


def test_blocks_are_ascending_and_refuse_what_does_not_divide():
    from pda_amd import ops
    assert ops.ialspp_blocks(256, 64) == [0, 64, 128, 192] and ops.ialspp_blocks(32, 32) == [0] and ops.ialspp_blocks(128, 32) == [0, 32, 64, 96]
    for d, k, what in ((64, 128, "divide"), (48, 32, "embedding size"), (64, 16, "block size")):
        with pytest.raises(ValueError, match=what):
            ops.ialspp_blocks(d, k)


# ---- the binding and the argument checks ---------------------------------------------------------------------------------------------------
def test_the_binding_equals_the_header_and_no_size_function_is_exported():
    from pda_amd import _lib
    lib = _lib.load()
    assert declared_in("pda_hip_ialspp.h") == sorted(_lib.IALSPP_SIGNATURES) == NAMES
    assert not [n for n in NAMES if re.search(r"_workspace_bytes$|_ws_words$|_scratch_bytes$", n)]
    others = [v for k, v in vars(_lib).items() if k.endswith("SIGNATURES") and k != "IALSPP_SIGNATURES"]
    assert len(others) >= 20
    for d in others:
        assert not set(NAMES) & set(d)
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "pda_hip_ialspp.h":
            assert not set(NAMES) & set(declared_in(h)), h
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pda_hip_ialspp.h")).read(), flags=re.S)
    for n in NAMES:
        assert getattr(lib, n).argtypes == _lib.IALSPP_SIGNATURES[n][1] and getattr(lib, n).restype is C.c_int
        params = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert len(params.split(",")) == len(_lib.IALSPP_SIGNATURES[n][1]), n


@pytest.fixture(scope="module")
def entry_points():
    """name -> call(**what differs from a sound call); distinct non-null addresses stand for the buffers (never dereferenced)."""
    from pda_amd import _lib
    lib = _lib.load()
    keep = C.create_string_buffer(4096)
    b, c, g, e = (C.c_void_p(C.addressof(keep) + 64 * k) for k in range(4))
    big = 1 << 30

    def bpass(indptr=b, indices=b, perm=NULL, n_rows=9, nnz=20, work=b, n_work=9, long_rows=NULL, n_long=0, n_slots=0, Z=b, n_z=12, G=g, d=64, k=32,
              p0=32, alpha0=0.1, lam_row=b, X=c, e=e, fail=b, dbg=NULL, slots=NULL, slot_floats=0, delta=NULL, delta_floats=0):
        return lib.pda_ialspp_block_pass_f32(indptr, indices, perm, n_rows, nnz, work, n_work, long_rows, n_long, n_slots, Z, n_z, G, d, k, p0, alpha0,
                                             lam_row, X, e, fail, dbg, slots, slot_floats, delta, delta_floats, NULL)

    def predict(indptr=b, indices=b, n_rows=9, nnz=20, X=c, Z=b, n_z=12, d=64, e=e):
        return lib.pda_ialspp_predict_f32(indptr, indices, n_rows, nnz, X, Z, n_z, d, e, NULL)

    def gram(Z=b, n=9, d=256, G=g, ws=c, ws_floats=big):
        return lib.pda_ialspp_gram_f32(Z, n, d, G, ws, ws_floats, NULL)

    def loss(indptr=b, indices=b, n_rows=9, nnz=20, X=c, Z=b, n_z=12, G=g, d=256, lam_row=b, out=c):
        return lib.pda_ialspp_loss_f32(indptr, indices, n_rows, nnz, X, Z, n_z, G, d, lam_row, out, NULL)

    yield {"pass": bpass, "predict": predict, "gram": gram, "loss": loss}, b, c, g, e
    del keep


def test_every_argument_error_comes_back_before_any_launch(entry_points):
    eps, b, c, g, e = entry_points
    bpass, predict, gram, loss = eps["pass"], eps["predict"], eps["gram"], eps["loss"]
    for arg in ("indptr", "indices", "work", "Z", "G", "lam_row", "X", "e", "fail"):
        assert bpass(**{arg: NULL}) == ERR_ARG, arg
    assert bpass(n_rows=0) == ERR_ARG and bpass(n_z=0) == ERR_ARG and bpass(n_work=0) == ERR_ARG and bpass(n_rows=1 << 31) == ERR_ARG
    assert bpass(alpha0=-0.5) == ERR_ARG and bpass(alpha0=float("nan")) == ERR_ARG and bpass(alpha0=float("inf")) == ERR_ARG
    assert bpass(X=b) == ERR_ARG and bpass(X=g) == ERR_ARG and bpass(e=c) == ERR_ARG and bpass(e=g) == ERR_ARG      # X, Z, G and e are four buffers
    assert bpass(n_long=1, n_slots=2) == ERR_ARG                                            # cut rows without their list
    assert bpass(long_rows=b, n_long=1, n_slots=1, slots=c, slot_floats=1 << 30, delta=c, delta_floats=1 << 30) == ERR_ARG   # at least two chunks
    assert bpass(n_slots=2) == ERR_ARG                                                      # slots without cut rows
    assert bpass(long_rows=b, n_long=1, n_slots=2, n_work=10) == ERR_ARG                    # slots without a workspace
    sound = dict(long_rows=b, n_long=1, n_slots=2, n_work=10, slots=c, delta=g)
    assert bpass(slot_floats=2 * (32 * 32 + 32) - 1, delta_floats=64, **sound) == ERR_ARG   # a slot is k * k + k floats ...
    assert bpass(slot_floats=2 * (32 * 32 + 32), delta_floats=63, **sound) == ERR_ARG       # ... and k floats of delta
    assert bpass(slot_floats=1 << 30, delta_floats=64, **dict(sound, delta=NULL)) == ERR_ARG
    assert bpass(long_rows=b, n_long=1, n_slots=12, n_work=9, slots=c, slot_floats=1 << 30, delta=g, delta_floats=1 << 30) == ERR_ARG
    # the block: unsupported sizes, then what does not divide, then p0
    for d, k in ((48, 32), (16, 16), (512, 64), (64, 16), (256, 256), (128, 48), (0, 32), (64, 0)):
        assert bpass(d=d, k=k, p0=0) == ERR_UNSUPPORTED, (d, k)
    for d, k in ((32, 64), (32, 128), (64, 128)):
        assert bpass(d=d, k=k, p0=0) == ERR_ARG, (d, k)                                    # both supported, but k does not divide d
    assert bpass(p0=-32) == ERR_ARG and bpass(p0=64) == ERR_ARG and bpass(p0=16) == ERR_ARG and bpass(d=256, k=128, p0=256) == ERR_ARG
    assert bpass(d=48, n_work=0) == ERR_ARG and bpass(d=48, Z=NULL) == ERR_ARG and bpass(k=16, alpha0=-1.0) == ERR_ARG      # (the argument errors come first)

    for arg in ("indptr", "indices", "X", "Z", "e"):
        assert predict(**{arg: NULL}) == ERR_ARG, arg
    assert predict(n_rows=0) == ERR_ARG and predict(n_z=0) == ERR_ARG and predict(n_z=1 << 31) == ERR_ARG
    for arg in ("Z", "G", "ws"):
        assert gram(**{arg: NULL}) == ERR_ARG, arg
    assert gram(n=0) == ERR_ARG and gram(n=1 << 31) == ERR_ARG
    assert gram(n=257, ws_floats=2 * (256 * 256 + 256) - 1) == ERR_ARG and gram(n=257, d=64, ws_floats=2 * (64 * 64 + 64) - 1) == ERR_ARG
    for arg in ("indptr", "indices", "X", "Z", "G", "lam_row", "out"):
        assert loss(**{arg: NULL}) == ERR_ARG, arg
    assert loss(n_rows=0) == ERR_ARG and loss(n_z=0) == ERR_ARG
    for d in (16, 48, 512, 0):
        assert predict(d=d) == ERR_UNSUPPORTED and gram(d=d) == ERR_UNSUPPORTED and loss(d=d) == ERR_UNSUPPORTED, d
    assert gram(d=48, n=0) == ERR_ARG and predict(d=48, X=NULL) == ERR_ARG and loss(d=48, out=NULL) == ERR_ARG


def test_ops_refuses_bad_calls_before_the_library():
    import torch
    from pda_amd import ops
    with pytest.raises(ValueError, match="HBM"):
        ops.ialspp_gram(torch.zeros(9, 256))
    with pytest.raises(ValueError, match="same pairs"):
        ops.ials_pair_perm(np.array([0, 1, 2]), np.array([0, 1]), np.array([0, 1, 2]), np.array([1, 0]))


# ---- pair_perm ------------------------------------------------------------------------------------------------------------------------------------
def zipf_pairs(seed=3, nu=70, ni=45, n=2500):
    g = np.random.default_rng(seed)
    return g.integers(0, nu - 1, n), np.minimum(g.zipf(1.4, n) - 1, ni - 2), nu, ni        # duplicates; the last user and item stay without pairs


def test_pair_perm_is_the_inverse_map_with_duplicates_and_empty_rows():
    from pda_amd import ops
    u, i, nu, ni = zipf_pairs()
    h = ops.ials_graph_arrays(u, i, nu, ni)
    assert h["nnz"] < len(u) and h["user"]["deg"][-1] == 0 and h["item"]["deg"][-1] == 0 and (h["user"]["deg"] == 0).sum() >= 1
    up, ui, ip, ii = h["user"]["indptr"], h["user"]["indices"], h["item"]["indptr"], h["item"]["indices"]
    perm = ops.ials_pair_perm(up, ui, ip, ii)
    assert perm.dtype == np.int64 and perm.shape == (h["nnz"],)
    np.testing.assert_array_equal(perm, pr.pair_perm(up, ui, ip, ii))
    np.testing.assert_array_equal(np.sort(perm), np.arange(h["nnz"]))                       # a permutation
    urow = np.repeat(np.arange(nu), np.diff(up))
    irow = np.repeat(np.arange(ni), np.diff(ip))
    np.testing.assert_array_equal(urow[perm], ii)                                          # the pair at item position q is (ii[q], irow[q]) ...
    np.testing.assert_array_equal(ui[perm], irow)                                          # ... and so is the pair at user position perm[q]


# ---- the restatement's own properties ------------------------------------------------------------------------------------------------------------
def small(seed=5, nu=12, ni=9, d=8, n=60):
    g = np.random.default_rng(seed)
    eu, ei = ir.dedup_pairs(g.integers(0, nu - 1, n), g.integers(0, ni, n), ni)
    X, Y = g.standard_normal((nu, d)) * 0.4, g.standard_normal((ni, d)) * 0.4
    up, ui = ir.csr(eu, ei, nu)
    ip, ii = ir.csr(ei, eu, ni)
    return eu, ei, X, Y, up, ui, ip, ii


@pytest.mark.parametrize("a0, lam, nu", [(0.25, 0.05, 1.0), (0.5, 0.05, 0.0), (0.01, 0.1, 0.5)])
def test_repeated_passes_over_all_blocks_converge_to_the_half_sweep(a0, lam, nu):
    """With Y fixed, sweeping the blocks is block Gauss-Seidel on the SPD systems A_r x = b_r: the error falls monotonically in the energy
    norm of A_r and goes to zero, i.e. the passes converge to half_sweep; the cached predictions stay those of the tables."""
    eu, ei, X, Y, up, ui, ip, ii = small()
    lu = ir.lam_row(np.diff(up), Y.shape[0], lam, a0, nu)
    want = ir.half_sweep(up, ui, Y, a0, lu)
    A = [ir.normal_equations(up, ui, Y, a0, lu, r)[0] for r in range(X.shape[0])]
    energy = lambda X: np.array([(X[r] - want[r]) @ A[r] @ (X[r] - want[r]) for r in range(X.shape[0])])       # noqa: E731
    e = pr.predictions(X, Y, up, ui)
    last = energy(X)
    for sweep in range(3000):
        for p0 in (0, 2, 4, 6):
            X, e = pr.block_pass(X, e, up, ui, None, Y, a0, lu, p0, 2)
            now = energy(X)
            assert (now <= last * (1 + 1e-9) + 1e-28).all()
            last = now
        if np.abs(X - want).max() < 1e-12:
            break
    assert np.abs(X - want).max() < 1e-12, (sweep, np.abs(X - want).max())
    np.testing.assert_allclose(e, pr.predictions(X, Y, up, ui), atol=1e-12)
    assert np.abs(X[-1]).max() < 1e-12                                                      # the row without pairs goes to zero


def test_k_equal_to_d_is_the_half_sweep_in_one_step_from_any_start():
    eu, ei, X, Y, up, ui, ip, ii = small()
    a0, lam = 0.25, 0.05
    lu = ir.lam_row(np.diff(up), Y.shape[0], lam, a0, 1.0)
    for scale in (0.0, 1.0, 30.0):
        X1, e1 = pr.block_pass(X * scale, pr.predictions(X * scale, Y, up, ui), up, ui, None, Y, a0, lu, 0, X.shape[1])
        np.testing.assert_allclose(X1, ir.half_sweep(up, ui, Y, a0, lu), atol=1e-11 * max(1.0, scale))
        np.testing.assert_allclose(e1, pr.predictions(X1, Y, up, ui), atol=1e-11 * max(1.0, scale))


def test_an_epoch_never_raises_the_objective_and_keeps_the_cache_true():
    eu, ei, X, Y, up, ui, ip, ii = small()
    a0, lam = 0.1, 0.05
    lu, li = ir.lam_row(np.diff(up), Y.shape[0], lam, a0, 1.0), ir.lam_row(np.diff(ip), X.shape[0], lam, a0, 1.0)
    perm = pr.pair_perm(up, ui, ip, ii)
    last = ir.objective(X, Y, eu, ei, a0, lu, li)[0]
    e = pr.predictions(X, Y, up, ui)
    for _ in range(3):
        for p0 in (0, 4):
            X, e = pr.block_pass(X, e, up, ui, None, Y, a0, lu, p0, 4)
            mid = ir.objective(X, Y, eu, ei, a0, lu, li)[0]
            Y, e = pr.block_pass(Y, e, ip, ii, perm, X, a0, li, p0, 4)
            now = ir.objective(X, Y, eu, ei, a0, lu, li)[0]
            assert mid <= last * (1 + 1e-13) and now <= mid * (1 + 1e-13)
            last = now
        np.testing.assert_allclose(e, pr.predictions(X, Y, up, ui), atol=1e-12)
    X2, Y2, e2 = pr.epoch(X, Y, up, ui, ip, ii, a0, lu, li, 4)
    assert ir.objective(X2, Y2, eu, ei, a0, lu, li)[0] <= last * (1 + 1e-13)


def test_the_exact_test_s_inputs_are_exact_in_fp32_whatever_the_order():
    rows, cols = ir.length_graph(lengths=(0, 1, 33, 300, 2 * 256 + 5), n_other=600)
    ip, ix = ir.csr(rows, cols, 5)
    d, k, p0 = 64, 32, 32
    Z, X, lam, g = pr.exact_inputs(d, 5, 600)
    e = (g.integers(-4, 9, len(ix)) / 4.0).astype(np.float32)
    G32 = ir.gram32(Z)
    G = Z.astype(np.float64).T @ Z.astype(np.float64)
    np.testing.assert_array_equal(G32.astype(np.float64), G)
    for a0 in (0.25, 0.5):
        assert pr.exact_headroom(ip, ix, Z, X, e, a0, lam, p0, k) < 2 ** 24
        for r in range(5):
            H32, g32 = pr.system32(ip, ix, None, Z, G32, X[r], e, a0, lam, r, p0, k, chunk=256)
            H, gg = pr.block_system(X[r], e[ip[r]:ip[r + 1]], Z[ix[ip[r]:ip[r + 1]]], G, a0, lam[r], p0, k)
            np.testing.assert_array_equal(H32.astype(np.float64), H)
            np.testing.assert_array_equal(g32.astype(np.float64), gg)


def test_the_bound_of_a_step_covers_an_fp32_evaluation_of_it():
    """step_bounds on a small system, against the same step carried out in fp32 numpy: the fp32 result lies inside, with room."""
    rows, cols = ir.length_graph(lengths=(0, 1, 33, 90), n_other=120)
    ip, ix = ir.csr(rows, cols, 4)
    d, k, p0, a0 = 64, 32, 32, 0.1
    Z = ir.table("gauss0.3", 120, d)
    X = ir.table("gauss0.3", 4, d, seed=5)
    lam = ir.lam_row(np.diff(ip), 120, 0.05, a0, 1.0)
    e = pr.predictions(X, Z, ip, ix).astype(np.float32)
    o = pr.pass_bounds(X, e, ip, ix, None, Z, a0, lam, p0, k)
    assert np.isfinite(o["dX"]).all() and np.isfinite(o["de"]).all()
    G32 = ir.gram32(Z)
    for r in range(4):
        H32, g32 = pr.system32(ip, ix, None, Z, G32, X[r], e, a0, lam, r, p0, k)
        x1 = X[r].copy()
        x1[p0:p0 + k] = (X[r, p0:p0 + k] - np.linalg.solve(H32.astype(np.float64), g32.astype(np.float64)).astype(np.float32)).astype(np.float32)
        assert np.linalg.norm(x1 - o["X"][r]) <= o["dX"][r]
