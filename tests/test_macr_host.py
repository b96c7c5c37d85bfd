"""CPU suite for MACR (`--train macr`, include/pda_hip_macr.h): the flags, the refusals, the grid over c, the binding against the header, the
entry points' argument checks (all before any HIP call), the checkpoint, the restatement of tests/macr_ref.py against a closed form, the
float32 restatement inside the bounds the GPU suite holds the kernels to, the ranking identity, and the separation of the list inputs."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from macr_ref import (BATCHES, C_GRID, DIMS, KINDS, LIST_CS, LIST_DIMS, LIST_SHAPES, REGS, TOL, WEIGHTS, arg_topk, close_rows, contract_lists, list_case,
                      macr_grads, model_values, parity_case, rounding_bound, tolerance)
from test_abi import declared_in

ERR_ARG, ERR_UNSUPPORTED = -1, -2
CONFIG = {"n_users": 9, "n_items": 12}


def make_args(**over):
    from pda_amd.parse import parse_args
    a = parse_args(["--train", "macr", "--test", "macr", "--embed_size", "64", "--batch_size", "16"])
    for k, v in over.items():
        setattr(a, k, v)
    return a


# ---- flags, refusals, the grid ---------------------------------------------------------------------------------------------------------------
def test_the_seven_flags_keep_their_names_types_and_defaults():
    from pda_amd import parse
    a = parse.parse_args([])
    want = {"alpha": 1e-3, "beta": 1e-3, "c": 10.0, "check_c": 1, "start": -1.0, "end": 1.0, "step": 20}
    for k, v in want.items():
        assert getattr(a, k) == v and type(getattr(a, k)) is type(v), k
    assert set(want) <= set(parse.reference_flag_names())            # reference flags, not extensions
    table = {f[0]: f for f in parse._REFERENCE_FLAGS}
    for k, v in want.items():                                          # only the help text changed: it now says what MACR does with the flag
        assert table[k][1] is type(v) and table[k][2] == v and "MACR" in table[k][3] and "(unused)" not in table[k][3], k
    ext = [f[0] for f in parse._EXTENSION_FLAGS]
    assert not set(want) & set(ext)
    b = parse.parse_args("--train macr --test macr --alpha 0.5 --beta 0.25 --c 0.3 --check_c 0 --start -2 --end 2 --step 5".split())
    assert (b.train, b.test, b.alpha, b.beta, b.c, b.check_c, b.start, b.end, b.step) == ("macr", "macr", 0.5, 0.25, 0.3, 0, -2.0, 2.0, 5)


def test_the_grid_over_c():
    from pda_amd.model_api import macr_c_grid
    g = macr_c_grid(make_args())
    assert g == list(C_GRID) == [float(c) for c in np.linspace(-1, 1, 20)] and len(g) == 20 and g[0] == -1.0 and g[-1] == 1.0 and 0.0 not in g
    assert macr_c_grid(make_args(check_c=0, c=0.3)) == [0.3]            # --check_c 0: the single --c
    assert macr_c_grid(make_args(start=0.0, end=2.0, step=5)) == [0.0, 0.5, 1.0, 1.5, 2.0]


def test_every_evaluation_starts_with_c_zero():
    """The trainer's evaluation: c = 0 first (printed as "MACR without c"), then the grid; the best c by recall@Ks[0] ends in the model."""
    from pda_amd import train_new_api as t
    src = open(t.__file__).read()
    block = src[src.index('elif args.test == "macr":'):src.index('elif args.test == "normal":')]
    assert block.index("rec.update_c(0.0)") < block.index('print("MACR without c")') < block.index("for c in macr_c_grid(args):")
    assert 'ret_c["recall"][0] > best_ret["recall"][0]' in block and "rec.best_c = best_c" in block


@pytest.mark.parametrize("over, flag", [({"deterministic": 1}, "--deterministic"), ({"table_dtype": "bf16"}, "--table_dtype"),
                                        ({"optimizer": "sgd"}, "--optimizer"), ({"optimizer": "lazy_adam"}, "--optimizer"),
                                        ({"adam_sweep": "replay"}, "--adam_sweep"), ({"adam_sweep": "replay_fast"}, "--adam_sweep"),
                                        ({"gpus": 2}, "--gpus"), ({"topk_max": 55}, "--topk_max"), ({"topk_max": 1024}, "--topk_max"),
                                        ({"embed_size": 32}, "--embed_size"), ({"embed_size": 48}, "--embed_size"), ({"embed_size": 512}, "--embed_size")])
def test_refused_options_name_their_flag(over, flag):
    from pda_amd.model_api import MACRBPRMF
    with pytest.raises(NotImplementedError, match=flag):
        MACRBPRMF(make_args(**over), CONFIG, device="cpu")


@pytest.mark.parametrize("over, flag", [({"alpha": float("nan")}, "--alpha"), ({"beta": float("inf")}, "--beta"), ({"c": float("nan")}, "--c"),
                                        ({"check_c": 2}, "--check_c"), ({"step": 0}, "--step")])
def test_bad_values_are_value_errors_that_name_their_flag(over, flag):
    from pda_amd.model_api import MACRBPRMF
    with pytest.raises(ValueError, match=flag):
        MACRBPRMF(make_args(**over), CONFIG, device="cpu")


def test_the_trainer_refuses_every_other_test_mode(monkeypatch):
    from pda_amd import train_new_api as t
    for test in ("normal", "s_condition", "temp_pop", "dice", "ips"):
        monkeypatch.setattr(t, "configure", lambda argv=None, test=test: setattr(t, "args", make_args(test=test)))
        with pytest.raises(NotImplementedError, match="--train macr goes with --test macr"):
            t.main([])
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(train="normal")))
    with pytest.raises(NotImplementedError, match="--test macr needs a MACR model"):
        t.main([])
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(optimizer="sgd")))
    with pytest.raises(NotImplementedError, match="--optimizer"):
        t.main([])
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(topk_max=60)))
    with pytest.raises(NotImplementedError, match="--topk_max"):
        t.main([])


def test_lists_are_refused_outside_the_bias_head():
    from pda_amd import ops
    ops.check_macr_lists(64, 54)
    with pytest.raises(ValueError, match="embedding width"):
        ops.check_macr_lists(32, 50)
    with pytest.raises(ValueError, match="K must lie in 1 .. 54"):
        ops.check_macr_lists(64, 55)


# ---- the binding and the argument checks ---------------------------------------------------------------------------------------------------
def test_binding_equals_the_header():
    from pda_amd import _lib
    names = ["pda_macr_adam_step_f32", "pda_macr_item_bias_f32", "pda_macr_item_prep_f32", "pda_macr_step_f32"]
    assert declared_in("pda_hip_macr.h") == sorted(_lib.MACR_SIGNATURES) == names
    for d in (_lib.SIGNATURES, _lib.TEMP_POP_SIGNATURES, _lib.PC_SIGNATURES, _lib.DET_SIGNATURES, _lib.DEEP_SIGNATURES, _lib.XQUAD_SIGNATURES,
              _lib.DICE_SIGNATURES, _lib.IPS_SIGNATURES):
        assert not set(names) & set(d)
    assert not set(names) & (set(declared_in("pda_hip.h")) | set(declared_in("pda_hip_experimental.h")))
    lib = _lib.load()
    for n in names:
        assert getattr(lib, n).argtypes == _lib.MACR_SIGNATURES[n][1]


def test_entry_points_check_arguments_without_gpu():
    from pda_amd import _lib
    lib = _lib.load()
    keep = C.create_string_buffer(4096)
    b, null = C.c_void_p(C.addressof(keep)), C.c_void_p(None)

    def step(U=b, wi=b, users=b, gW=b, tagI=b, B=8, d=32, alpha=1e-3, reg_div=8.0, tag=1, flags=0x100, nu=9, ni=12):
        return lib.pda_macr_step_f32(U, b, wi, b, nu, ni, users, b, b, B, d, alpha, 1e-3, 1e-3, reg_div, b, b, gW, b, tagI, tag, flags, null, null)

    assert step(U=null) == ERR_ARG and step(wi=null) == ERR_ARG and step(users=null) == ERR_ARG and step(gW=null) == ERR_ARG and step(tagI=null) == ERR_ARG
    assert step(B=0) == ERR_ARG and step(reg_div=0.0) == ERR_ARG and step(reg_div=float("nan")) == ERR_ARG and step(tag=0) == ERR_ARG
    assert step(alpha=float("nan")) == ERR_ARG and step(alpha=float("inf")) == ERR_ARG
    assert step(nu=0) == ERR_ARG and step(ni=0) == ERR_ARG and step(ni=1 << 31) == ERR_ARG and step(flags=0x400) == ERR_ARG and step(flags=2) == ERR_ARG
    assert step(d=16) == ERR_UNSUPPORTED and step(d=48) == ERR_UNSUPPORTED and step(d=512) == ERR_UNSUPPORTED

    def adam(m=b, mW=b, wu=b, policy=0, d=64, flags=0x300, B=8):
        return lib.pda_macr_adam_step_f32(b, m, b, b, b, 9, b, b, b, b, b, 12, b, wu, mW, b, b, b, b, b, B, d, 1e-3, 1e-3, 1e-3, 8.0, 1, 1e-3, 0.9, 0.999,
                                          1e-8, flags, policy, null, null)

    assert adam(m=null) == ERR_ARG and adam(mW=null) == ERR_ARG and adam(wu=null) == ERR_ARG and adam(policy=5) == ERR_ARG and adam(policy=-1) == ERR_ARG
    assert adam(flags=1) == ERR_ARG and adam(B=-3) == ERR_ARG and adam(d=8) == ERR_UNSUPPORTED

    def prep(I=b, w=b, sig=b, J=b, n=12, d=64):
        return lib.pda_macr_item_prep_f32(I, w, n, d, sig, J, null)

    assert prep(I=null) == ERR_ARG and prep(w=null) == ERR_ARG and prep(sig=null) == ERR_ARG and prep(J=null) == ERR_ARG and prep(n=0) == ERR_ARG
    assert prep(n=1 << 31) == ERR_ARG and prep(d=16) == ERR_UNSUPPORTED and prep(d=96) == ERR_UNSUPPORTED
    bias = lib.pda_macr_item_bias_f32
    assert bias(null, 0.5, b, 12, null) == ERR_ARG and bias(b, 0.5, null, 12, null) == ERR_ARG and bias(b, 0.5, b, 0, null) == ERR_ARG
    assert bias(b, float("nan"), b, 12, null) == ERR_ARG and bias(b, float("inf"), b, 12, null) == ERR_ARG
    del keep


def test_ops_refuses_bad_batches_before_the_library():
    from pda_amd import ops
    U, I = torch.zeros(9, 32), torch.zeros(12, 32)
    i4 = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="HBM"):
        ops.macr_grads(U, I, torch.zeros(32), torch.zeros(32), i4, i4, i4, None, alpha=0, beta=0, regs=1e-3, reg_div=4, step=1)
    with pytest.raises(ValueError, match="HBM"):
        ops.macr_item_prep(I, torch.zeros(32))
    with pytest.raises(ValueError, match="HBM"):
        ops.macr_item_bias(torch.zeros(12), 0.5)


# ---- the model and its checkpoint ----------------------------------------------------------------------------------------------------------------
def test_model_parameters_checkpoint_round_trip_and_a_bprmf_refuses_it():
    from pda_amd.model_api import BPRMF, MACRBPRMF
    a = MACRBPRMF(make_args(alpha=0.5, beta=0.25), CONFIG, device="cpu", seed=1)
    assert isinstance(a, BPRMF) and [f.name for f in (a.opt, a.loss, a.mf_loss, a.reg_loss, a.batch_ratings)] == ["opt", "loss", "mf_loss", "reg_loss",
                                                                                                                   "batch_ratings"]
    assert (a.alpha, a.beta, a.c, a.best_c) == (0.5, 0.25, 0.0, 0.0)
    lim = np.sqrt(6.0 / (64 + 1))                                       # Xavier for [d, 1]: fan_in = d, fan_out = 1
    for k in ("w_item", "w_user"):
        w = a.weights[k]
        assert w.shape == (64, 1) and w.dtype == torch.float32 and float(w.abs().max()) <= lim and float(w.abs().max()) > 0.7 * lim
    assert not torch.equal(a.weights["w_item"], a.weights["w_user"])
    a.update_c(0.37)
    assert a.c == 0.37
    with pytest.raises(ValueError, match="finite"):
        a.update_c(float("nan"))
    a.best_c = 0.37
    # the trainer's three terms of a row of five
    np.testing.assert_allclose(a.trainer_terms(torch.tensor([3.0, 1.0, 2.0, 4.0, 0.5])).numpy(), [3.0, 2.5, 0.5])
    # a state with moments, without a GPU: the attributes ops.MacrState holds
    st = a._macr = type("S", (), {})()
    g = torch.Generator().manual_seed(4)
    for k, ref in (("mU", a.weights["user_embedding"]), ("vU", a.weights["user_embedding"]), ("mI", a.weights["item_embedding"]),
                   ("vI", a.weights["item_embedding"]), ("mW", torch.zeros(2, 64)), ("vW", torch.zeros(2, 64))):
        setattr(st, k, torch.rand(ref.shape, generator=g))
    a._t = 17
    buf = io.BytesIO()
    torch.save(a.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf)
    assert sd["format"] == "pda_amd/2" and sd["model"] == "macr" and (sd["macr_c"], sd["macr_alpha"], sd["macr_beta"], sd["adam_t"]) == (0.37, 0.5, 0.25, 17)
    assert {"w_item", "w_user", "mW", "vW", "mU", "vU", "mI", "vI", "user_embedding", "item_embedding"} <= set(sd)
    with pytest.raises(ValueError, match="checkpoint of a macr model cannot be loaded into BPRMF"):
        BPRMF(make_args(train="normal", test="normal"), CONFIG, device="cpu", seed=2).load_state_dict(sd)
    plain = BPRMF(make_args(train="normal", test="normal"), CONFIG, device="cpu", seed=2)
    with pytest.raises(ValueError, match="checkpoint of a mf model cannot be loaded into MACRBPRMF"):
        a.load_state_dict(plain.state_dict())
    with pytest.raises(ValueError, match="embed_size"):
        MACRBPRMF(make_args(embed_size=128), CONFIG, device="cpu").load_state_dict(sd)
    # the restore itself builds an ops.MacrState: needs only torch
    m = MACRBPRMF(make_args(), CONFIG, device="cpu", seed=3)
    assert not torch.equal(a.weights["w_item"], m.weights["w_item"])
    m.load_state_dict(sd)
    for k in ("user_embedding", "item_embedding", "w_item", "w_user"):
        assert torch.equal(a.weights[k], m.weights[k])
    for k in ("mU", "vU", "mI", "vI", "mW", "vW"):
        assert torch.equal(getattr(st, k), getattr(m._macr, k))
    assert m._t == 17 and m.c == m.best_c == 0.37 and float(m._macr.gW.abs().max()) == 0.0


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------------
def test_restated_gradients_match_the_closed_form():
    """macr_grads (autograd) against the chain rule written out in float64, triplet by triplet."""
    rng = np.random.default_rng(3)
    nU, nI, d, B = 7, 9, 4, 16
    U, I = rng.standard_normal((nU, d)) * 0.6, rng.standard_normal((nI, d)) * 0.6
    wi, wu = rng.standard_normal(d), rng.standard_normal(d)
    users, pos, neg = rng.integers(0, nU, B), rng.integers(0, nI, B), rng.integers(0, nI, B)
    al, be, regs = 0.5, 0.25, 1e-2
    terms, gU, gI, gW = macr_grads(U, I, wi, wu, users, pos, neg, alpha=al, beta=be, regs=regs, reg_div=B)
    sg = lambda x: 1 / (1 + np.exp(-x))                                # noqa: E731
    e = 1e-10
    eU, eI, eW, c = np.zeros_like(U), np.zeros_like(I), np.zeros((2, d)), regs / B
    lo = li = lu = 0.0
    for u, p, n in zip(users, pos, neg):
        yp, yn, sp, sn, su = U[u] @ I[p], U[u] @ I[n], sg(I[p] @ wi), sg(I[n] @ wi), sg(U[u] @ wu)
        zp, zn = sg(yp * sp * su), sg(yn * sn * su)
        lo += (-np.log(zp + e) - np.log(1 - zn + e)) / B
        li += (-np.log(sp + e) - np.log(1 - sn + e)) / B
        lu += (-np.log(su + e) - np.log(1 - su + e)) / B
        gap, gan = -zp * (1 - zp) / (zp + e) / B, zn * (1 - zn) / (1 - zn + e) / B
        hp = (gap * yp * su - al / B / (sp + e)) * sp * (1 - sp)
        hn = (gan * yn * su + al / B / (1 - sn + e)) * sn * (1 - sn)
        hu = (gap * yp * sp + gan * yn * sn + be / B * (-1 / (su + e) + 1 / (1 - su + e))) * su * (1 - su)
        eU[u] += gap * sp * su * I[p] + gan * sn * su * I[n] + hu * wu + c * U[u]
        eI[p] += gap * sp * su * U[u] + hp * wi + c * I[p]
        eI[n] += gan * sn * su * U[u] + hn * wi + c * I[n]
        eW[0] += hp * I[p] + hn * I[n]
        eW[1] += hu * U[u]
    np.testing.assert_allclose(gU, eU, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(gI, eI, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(gW, eW, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(terms[1:4], [lo, li, lu], rtol=1e-12)
    assert terms[0] == pytest.approx(lo + al * li + be * lu + terms[4], rel=1e-14)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("d", DIMS)
def test_the_float32_restatement_stays_inside_the_gpu_bounds(d, B, kind):
    """tests/test_gpu_macr.py holds the kernels to 1e-5 on these very inputs: the restatement itself, computed in float32, stays inside a quarter
    of that on every loss term and on all four gradients -- gW, which sums B terms, included -- so the bounds ask nothing float32 arithmetic
    cannot give."""
    U, I, wi, wu, b = parity_case(d, B, kind)
    for alpha, beta in WEIGHTS:
        kw = dict(alpha=alpha, beta=beta, regs=REGS, reg_div=B)
        r64 = macr_grads(U, I, wi, wu, *b, **kw)
        r32 = macr_grads(U, I, wi, wu, *b, dtype=torch.float32, **kw)
        for what, x, y in zip(("loss", "gU", "gI", "gW"), r64, r32):
            assert tolerance(what) == TOL == 1e-5
            assert np.abs(x - y).max() <= tolerance(what) / 4, (what, np.abs(x - y).max())
    if kind == "spread":
        s = lambda x: 1 / (1 + np.exp(-x))                             # noqa: E731
        for v in (s(I.astype(np.float64) @ wi), s(U.astype(np.float64) @ wu)):
            assert 0.05 - 1e-6 <= v.min() and v.max() <= 0.95 + 1e-6 and v.max() - v.min() > 0.6
    if B == 2048:       # every row is hot, and gW sums 2 048 terms
        assert np.bincount(b[0], minlength=64).min() >= 15 and np.bincount(np.concatenate([b[1], b[2]]), minlength=40).min() >= 60


# ---- the ranking -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", LIST_DIMS)
@pytest.mark.parametrize("shape", LIST_SHAPES)
def test_the_ranking_identity_on_the_list_inputs(shape, d):
    """s_u > 0: the float64 lists of (y - c) s_i s_u and of (y - c) s_i are identical for every c of the grid (negative c included) and of the
    GPU list test."""
    U, I, w, users, hist = list_case(*shape, d)
    w_user = 12.5 * w.astype(np.float64)                                # along the users' common direction: s_u from 0.05 to 0.95
    s_u = 1.0 / (1.0 + np.exp(-(U.astype(np.float64) @ w_user)))
    assert s_u.min() > 0 and s_u.max() - s_u.min() > 0.6
    for c in C_GRID + LIST_CS:
        a, b = model_values(U, I, w, users, c), model_values(U, I, w, users, c, s_u=s_u)
        for r, items in enumerate(hist):
            a[r, items] = b[r, items] = -np.inf
        np.testing.assert_array_equal(arg_topk(a, 54), arg_topk(b, 54))


@pytest.mark.parametrize("d", LIST_DIMS)
@pytest.mark.parametrize("shape", LIST_SHAPES)
def test_the_list_inputs_are_separated_by_more_than_the_rounding_bound(shape, d):
    """The condition of the GPU list test: in at most 1 % of the rows do two adjacent values of the float64 list lie closer than the bound the
    test grants (2 max_i E of the row), for every c it ranks with -- a wrong list cannot hide inside the bound."""
    U, I, w, users, hist = list_case(*shape, d)
    assert shape[1] - len(hist[0]) == 40 and max(len(h) for h in hist[1:]) <= 30
    for c in LIST_CS:
        v, E = model_values(U, I, w, users, c), rounding_bound(U, I, w, users, c)
        bad = close_rows(v, E, 54, hist)
        assert len(bad) <= 0.01 * shape[0], (c, bad)
        assert 2 * E.max() < 2e-4                                       # (and the bound itself stays far below a value step of 2.6e-3)


def test_the_contract_restatement_breaks_ties_by_the_lower_id_and_masks():
    s = np.float32([[1, 3, 3, 2, 3], [5, 5, 5, 5, 5]])
    ids, h = contract_lists(s, np.float32([0.5] * 5), 0.0, 3, [np.array([1]), np.array([0, 1, 2, 3])])
    np.testing.assert_array_equal(ids, [[2, 4, 3], [4, 0, 1]])         # masked items fill a short list, lowest id first
    ids, h = contract_lists(s, np.float32([0, 0, 0, 4, 0]), -1.0, 2, [[], []])
    np.testing.assert_array_equal(ids, [[3, 1], [3, 0]])               # beta = +sig: item 3 moves to the front
    assert h.dtype == np.float32 and h[0, 3] == 6.0
