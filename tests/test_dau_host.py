"""CPU suite for the DirectAU loss (`--train dau`, include/pda_hip_dau.h): the flags, the refusals, the run-directory suffix, the binding against
the header, the entry points' argument checks (all before any HIP call), the checkpoint, the closed form of the contract against autograd, the
float32 restatement inside the bound the GPU suite holds the kernels to, and the mutants that suite must be able to tell from the contract."""
import ctypes as C
import functools
import io
import os
import re

import numpy as np
import pytest
import torch

import dau_ref as dr
from dau_ref import CASES, MUTANTS, REGS, T, case_id, case_reference, parity_case, tolerance, worst
from test_abi import declared_in

ERR_ARG, ERR_UNSUPPORTED = -1, -2
CONFIG = {"n_users": 9, "n_items": 12}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_args(**over):
    from pda_amd.parse import parse_args
    a = parse_args(["--train", "dau", "--embed_size", "32", "--batch_size", "16"])
    for k, v in over.items():
        setattr(a, k, v)
    return a


# ---- flags and refusals --------------------------------------------------------------------------------------------------------------------
def test_flags_parse_and_the_reference_flags_stay():
    from pda_amd import parse
    a = parse.parse_args([])
    assert (a.dau_gamma, a.dau_t, a.dau_same, a.dau_rank) == (1.0, 2.0, "keep", "raw")
    assert isinstance(a.dau_gamma, float) and isinstance(a.dau_t, float)
    b = parse.parse_args("--train dau --test dau --dau_gamma 0.5 --dau_t 4 --dau_same drop --dau_rank cosine".split())
    assert (b.train, b.test, b.dau_gamma, b.dau_t, b.dau_same, b.dau_rank) == ("dau", "dau", 0.5, 4.0, "drop", "cosine")
    ext = [f[0] for f in parse._EXTENSION_FLAGS]
    at = ext.index("dau_gamma")
    assert ext[at:at + 4] == ["dau_gamma", "dau_t", "dau_same", "dau_rank"]
    assert not set(ext) & set(parse.reference_flag_names()) and parse.reference_flag_names()[:5] == ["data_path", "dataset", "source", "train", "test"]
    assert "untuned" in {f[0]: f[3] for f in parse._EXTENSION_FLAGS}["dau_gamma"].lower()


@pytest.mark.parametrize("over, flag", [({"deterministic": 1}, "--deterministic"), ({"table_dtype": "bf16"}, "--table_dtype"),
                                        ({"optimizer": "sgd"}, "--optimizer"), ({"optimizer": "lazy_adam"}, "--optimizer"),
                                        ({"adam_sweep": "replay"}, "--adam_sweep"), ({"adam_sweep": "replay_fast"}, "--adam_sweep"),
                                        ({"sampler": "host"}, "--sampler"), ({"gpus": 2}, "--gpus"), ({"model": "lightgcn"}, "--model lightgcn"),
                                        ({"neg_sampler": "dns"}, "--neg_sampler")])
def test_refused_options_name_their_flag(over, flag):
    from pda_amd.model_api import DAUMF, check_dau
    with pytest.raises(NotImplementedError, match=flag):
        check_dau(make_args(**over))
    with pytest.raises(NotImplementedError, match=flag):
        DAUMF(make_args(**over), CONFIG, device="cpu")


@pytest.mark.parametrize("over, flag", [({"dau_gamma": -1.0}, "--dau_gamma"), ({"dau_gamma": float("nan")}, "--dau_gamma"),
                                        ({"dau_t": 0.0}, "--dau_t"), ({"dau_t": 20.5}, "--dau_t"), ({"dau_t": float("nan")}, "--dau_t"),
                                        ({"dau_same": "both"}, "--dau_same"), ({"dau_rank": "l2"}, "--dau_rank"),
                                        ({"batch_size": 1}, "--batch_size"), ({"batch_size": 16385}, "--batch_size")])
def test_bad_values_are_value_errors_that_name_their_flag(over, flag):
    from pda_amd.model_api import DAUMF
    with pytest.raises(ValueError, match=flag):
        DAUMF(make_args(**over), CONFIG, device="cpu")


def test_the_batch_size_limits_and_dns_under_train_dau():
    from pda_amd.model_api import check_dau, check_dns
    check_dau(make_args(batch_size=2))
    check_dau(make_args(batch_size=16384, dau_t=20.0, dau_gamma=0.0))
    with pytest.raises(NotImplementedError, match="--neg_sampler dns"):
        check_dns(make_args(neg_sampler="dns"))


def test_the_trainer_refuses_a_test_mode_dau_does_not_have(monkeypatch):
    from pda_amd import train_new_api as t
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(test="s_condition")))
    with pytest.raises(NotImplementedError, match="--train dau goes with --test normal"):
        t.main([])
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(test="normal", optimizer="sgd")))
    with pytest.raises(NotImplementedError, match="--optimizer"):
        t.main([])
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(test="dau", dau_same="both")))
    with pytest.raises(ValueError, match="--dau_same"):
        t.main([])


def test_the_tools_name_the_checkpoint_that_train_dau_writes(tmp_path):
    """export_topk, bpr_pc and xquad accept --train dau and look for the run directory with the `dau` suffix train_new_api.main gives it."""
    import inspect

    from pda_amd import bpr_pc, export_topk, synthetic, xquad
    from pda_amd import train_new_api as t
    src = inspect.getsource(t.main)
    assert 'if args.train == "dau":' in src and 'args.saveID += "dau"' in src and "||--- dau align=" in src
    toy = str(tmp_path / "data") + "/"
    synthetic.write_dataset(toy + "toy", n_users=60, n_items=40, mean_hist=6)
    save = str(tmp_path / "save") + "/"
    argv = ["--data_path", toy, "--dataset", "toy", "--train", "dau", "--save_dir", save, "--regs", "0.01", "--lr", "0.002", "--saveID", "x",
            "--pop_exp", "0.22", "--Ks", "[20,50]"]
    want = save + "mf_toy_checkpoint/wd_0.01_lr_0.002_a_0.001_xpop_exp-0.22dau_train_dau/best_ckpt.ckpt"
    for tool, extra in ((bpr_pc, []), (xquad, []), (export_topk, ["--export_out", str(tmp_path / "x.npz"), "--dau_rank", "cosine"])):
        with pytest.raises(FileNotFoundError) as e:
            tool.main(argv + extra)
        assert want in str(e.value), tool.__name__


# ---- the binding and the argument checks ---------------------------------------------------------------------------------------------------
NAMES = ["pda_dau_adam_step_f32", "pda_dau_col_splits", "pda_dau_step_f32", "pda_dau_workspace_bytes"]


def test_binding_equals_the_header():
    from pda_amd import _lib, ops
    assert declared_in("pda_hip_dau.h") == sorted(_lib.DAU_SIGNATURES) == NAMES
    for name in dir(_lib):
        if name.endswith("SIGNATURES") and name != "DAU_SIGNATURES":
            assert not set(NAMES) & set(getattr(_lib, name)), name
    assert not set(NAMES) & (set(declared_in("pda_hip.h")) | set(declared_in("pda_hip_experimental.h")) | set(declared_in("pda_hip_inbatch.h")))
    lib = _lib.load()
    for n in NAMES:
        assert getattr(lib, n).argtypes == _lib.DAU_SIGNATURES[n][1]
    raw = open(os.path.join(ROOT, "include", "pda_hip_dau.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for n in NAMES:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert len(params.split(",")) == len(_lib.DAU_SIGNATURES[n][1]), n
    define = lambda name: float(re.search(r"#define %s ([\d.]+)" % name, text).group(1))      # noqa: E731
    assert _lib.DAU_MAX_B == ops.DAU_MAX_B == define("PDA_DAU_MAX_B") == 16384 and ops.DAU_MAX_T == define("PDA_DAU_MAX_T") == 20.0
    assert T == ops.DAU_TILE == define("PDA_DAU_TILE") and ops.DAU_STAT_WORDS == define("PDA_DAU_STAT_WORDS") == 4
    assert ops.DAU_SAME == {"keep": define("PDA_DAU_SAME_KEEP"), "drop": define("PDA_DAU_SAME_DROP")} == {"keep": 0, "drop": 1}
    assert "restated from memory" in raw.lower()


def test_the_splits_and_the_workspace_are_functions_of_the_shape_alone():
    from pda_amd import _lib, ops
    lib = _lib.load()
    assert lib.pda_dau_col_splits(0) == 0 and lib.pda_dau_col_splits(16385) == 0
    assert ops.dau_col_splits(1) == ops.dau_col_splits(T) == 1 and ops.dau_col_splits(T + 3) > 1
    for B in (1, 2, T, T + 3, 2 * T + 5, 2048, 16384):
        assert 1 <= ops.dau_col_splits(B) <= -(-B // ops.DAU_TILE)
    for case in CASES:
        assert ops.dau_col_splits(case[1]) > 1 or case[1] <= T
    assert lib.pda_dau_workspace_bytes(0, 64) == 0 and lib.pda_dau_workspace_bytes(16385, 64) == 0 and lib.pda_dau_workspace_bytes(8, 48) == 0
    # linear in B: the image and the per-split slices of G, r and n, with splits x B <= B + 16 384 -- far below the B^2 words of a Gram matrix
    for d in (32, 256):
        for B in (1024, 2048, 4096, 16384):
            assert lib.pda_dau_workspace_bytes(B, d) <= 4 * (2 * B * d + 2 * (B + 16384 + 32 * 32) * (d + 2) + 10 * (B + 32)) + 1024
    with pytest.raises(ValueError, match="batch size"):
        ops.dau_col_splits(0)
    with pytest.raises(ValueError, match="batch size"):
        ops.dau_workspace(16385, 64, "cpu")
    with pytest.raises(ValueError, match="width"):
        ops.dau_workspace(8, 48, "cpu")


def test_entry_points_check_arguments_without_gpu():
    from pda_amd import _lib
    lib = _lib.load()
    keep = C.create_string_buffer(1 << 16)
    base = (C.addressof(keep) + 15) & ~15
    b, null, odd = C.c_void_p(base), C.c_void_p(None), C.c_void_p(base + 4)
    big = 1 << 30

    def step(U=b, users=b, pos=b, gU=b, tagI=b, ws=b, B=8, d=32, t=2.0, gamma=1.0, same=0, reg_div=8.0, tag=1, flags=0x100, nu=9, ni=12, wsb=big):
        return lib.pda_dau_step_f32(U, b, nu, ni, users, pos, B, d, t, gamma, same, 1e-3, reg_div, gU, b, b, tagI, tag, flags, ws, wsb, null, null, null)

    assert step(U=null) == ERR_ARG and step(users=null) == ERR_ARG and step(pos=null) == ERR_ARG and step(gU=null) == ERR_ARG
    assert step(tagI=null) == ERR_ARG and step(ws=null) == ERR_ARG and step(ws=odd) == ERR_ARG
    assert step(B=0) == ERR_ARG and step(B=-1) == ERR_ARG and step(B=16385) == ERR_ARG
    assert step(t=0.0) == ERR_ARG and step(t=-1.0) == ERR_ARG and step(t=float("nan")) == ERR_ARG and step(t=float("inf")) == ERR_ARG
    assert step(t=20.5) == ERR_ARG
    assert step(gamma=-0.5) == ERR_ARG and step(gamma=float("nan")) == ERR_ARG and step(gamma=float("inf")) == ERR_ARG
    assert step(same=2) == ERR_ARG and step(same=-1) == ERR_ARG
    assert step(reg_div=0.0) == ERR_ARG and step(reg_div=float("nan")) == ERR_ARG and step(tag=0) == ERR_ARG
    assert step(nu=0) == ERR_ARG and step(ni=0) == ERR_ARG and step(ni=1 << 31) == ERR_ARG and step(flags=0x400) == ERR_ARG and step(flags=2) == ERR_ARG
    assert step(wsb=0) == ERR_ARG and step(wsb=lib.pda_dau_workspace_bytes(8, 32) - 1) == ERR_ARG
    assert step(d=16) == ERR_UNSUPPORTED and step(d=48) == ERR_UNSUPPORTED and step(d=512) == ERR_UNSUPPORTED
    assert step(d=48, B=0) == ERR_ARG                                   # (the argument errors come first)

    def adam(m=b, pos=b, ws=b, policy=0, d=64, flags=0x300, B=8, t=2.0, gamma=1.0, same=1, wsb=big):
        return lib.pda_dau_adam_step_f32(b, m, b, b, b, 9, b, b, b, b, b, 12, b, pos, B, d, t, gamma, same, 1e-3, 8.0, 1, 1e-3, 0.9, 0.999, 1e-8,
                                         flags, policy, ws, wsb, null, null, null)

    assert adam(m=null) == ERR_ARG and adam(pos=null) == ERR_ARG and adam(ws=null) == ERR_ARG and adam(policy=5) == ERR_ARG and adam(policy=-1) == ERR_ARG
    assert adam(flags=1) == ERR_ARG and adam(B=-3) == ERR_ARG and adam(B=16385) == ERR_ARG and adam(t=0.0) == ERR_ARG and adam(t=21.0) == ERR_ARG
    assert adam(gamma=-1.0) == ERR_ARG and adam(same=2) == ERR_ARG and adam(wsb=16) == ERR_ARG and adam(d=8) == ERR_UNSUPPORTED
    assert lib.pda_dau_workspace_bytes(8, 32) > 0 and lib.pda_dau_workspace_bytes(8, 16) == 0 and lib.pda_dau_workspace_bytes(-1, 32) == 0
    del keep


def test_ops_refuses_bad_batches_before_the_library():
    from pda_amd import ops
    U, I = torch.zeros(9, 32), torch.zeros(12, 32)
    i4 = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="HBM"):
        ops.dau_step(U, I, i4, i4, U.clone(), I.clone(), torch.zeros(9, dtype=torch.int32), torch.zeros(12, dtype=torch.int32),
                     torch.zeros(64, dtype=torch.uint8), t=2.0, gamma=1.0, regs=1e-3, reg_div=4, step=1)


# ---- the model and its checkpoint ----------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_and_a_bprmf_loads_it():
    from pda_amd.model_api import BPRMF, DAUMF
    a = DAUMF(make_args(dau_gamma=0.5, dau_t=4.0, dau_same="drop", dau_rank="cosine"), CONFIG, device="cpu", seed=1)
    assert isinstance(a, BPRMF)
    a._t = 17
    buf = io.BytesIO()
    torch.save(a.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf)
    plain = BPRMF(make_args(train="normal"), CONFIG, device="cpu", seed=2)
    assert set(sd) - {"mU", "vU", "mI", "vI"} == (set(plain.state_dict()) - {"mU", "vU", "mI", "vI"}) | {"dau_gamma", "dau_t", "dau_same", "dau_rank"}
    assert (sd["dau_gamma"], sd["dau_t"], sd["dau_same"], sd["dau_rank"], sd["adam_t"], sd["embed_size"]) == (0.5, 4.0, "drop", "cosine", 17, 32)
    for m in (plain, DAUMF(make_args(), CONFIG, device="cpu", seed=3)):
        assert not torch.equal(a.weights["user_embedding"], m.weights["user_embedding"])
        m.load_state_dict(sd)
        for k in ("user_embedding", "item_embedding"):
            assert torch.equal(a.weights[k], m.weights[k])
        assert m._t == 17
    a.load_state_dict(plain.state_dict())                                        # and the other way round
    raw = DAUMF(make_args(), CONFIG, device="cpu", seed=3)
    U, I = raw.score_tables()                                                    # --dau_rank raw: the tables themselves
    assert U is raw.weights["user_embedding"] and I is raw.weights["item_embedding"]
    assert raw.take_dau() == (0.0, 0.0, 0.0)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("same", ["keep", "drop"])
def test_the_closed_form_of_the_contract_equals_autograd_on_the_definition(same):
    """The r_a / G_a form of include/pda_hip_dau.h written out in numpy float64 against dau_grads (autograd on the definition), with repeated
    users and items in the batch."""
    rng = np.random.default_rng(3)
    nU, nI, d, B, t, gamma = 7, 5, 4, 9, 1.7, 0.8
    U, I = rng.standard_normal((nU, d)) * 0.4, rng.standard_normal((nI, d)) * 0.4
    users, pos = rng.integers(0, nU, B), rng.integers(0, nI, B)
    assert len(np.unique(users)) < B and len(np.unique(pos)) < B
    c_reg = 1e-2 / B
    terms, gU, gI, stat = dr.dau_grads(U, I, users, pos, t=t, gamma=gamma, same=same, regs=1e-2, reg_div=B)
    nu, ni = np.maximum(np.sqrt((U[users] ** 2).sum(1)), 1e-12), np.maximum(np.sqrt((I[pos] ** 2).sum(1)), 1e-12)
    uh, ih = U[users] / nu[:, None], I[pos] / ni[:, None]

    def side(x, ids):
        adm = ~np.eye(B, dtype=bool)
        if same == "drop":
            adm &= ids[:, None] != ids[None, :]
        sq = (x * x).sum(1)
        e = np.where(adm, np.exp(-t * (sq[:, None] + sq[None, :] - 2 * x @ x.T)), 0.0)
        r, G = e.sum(1), e @ x
        S, P = r.sum() / 2, adm.sum() / 2
        return np.log(S / P), (-2 * t / S) * (r[:, None] * x - G)

    uni_u, du = side(uh, users)
    uni_i, di = side(ih, pos)
    g = (2 / B) * (uh - ih) + (gamma / 2) * du
    h = -(2 / B) * (uh - ih) + (gamma / 2) * di
    eU, eI = np.zeros_like(U), np.zeros_like(I)
    for r in range(B):
        eU[users[r]] += (g[r] - (uh[r] @ g[r]) * uh[r]) / nu[r] + c_reg * U[users[r]]
        eI[pos[r]] += (h[r] - (ih[r] @ h[r]) * ih[r]) / ni[r] + c_reg * I[pos[r]]
    np.testing.assert_allclose(gU, eU, rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(gI, eI, rtol=1e-10, atol=1e-13)
    align = ((uh - ih) ** 2).sum() / B
    np.testing.assert_allclose(stat, [align, uni_u, uni_i], rtol=1e-12)
    assert terms[1] == pytest.approx(align + gamma * (uni_u + uni_i) / 2, rel=1e-12)
    assert terms[2] == pytest.approx(1e-2 * 0.5 * ((U[users] ** 2).sum() + (I[pos] ** 2).sum()) / B, rel=1e-12)
    assert terms[0] == pytest.approx(terms[1] + terms[2], rel=1e-14)


def test_degenerate_batches_of_the_restatement():
    rng = np.random.default_rng(5)
    U, I = rng.standard_normal((6, 4)), rng.standard_normal((6, 4))
    one = dr.dau_grads(U, I, [2], [3], t=2.0, gamma=1.0, same="keep", regs=0.0, reg_div=1)
    assert one[3][1] == 0.0 and one[3][2] == 0.0 and one[0][1] == pytest.approx(one[3][0])          # B = 1: alignment alone
    users, pos = np.arange(4), np.full(4, 1)
    drop = dr.dau_grads(U, I, users, pos, t=2.0, gamma=1.0, same="drop", regs=0.0, reg_div=4)
    keep = dr.dau_grads(U, I, users, pos, t=2.0, gamma=1.0, same="keep", regs=0.0, reg_div=4)
    assert drop[3][2] == 0.0 and abs(keep[3][2]) < 1e-15 and np.isfinite(drop[1]).all() and np.isfinite(keep[2]).all()
    np.testing.assert_allclose(drop[2], keep[2], atol=1e-14)            # e = 1 at distance 0: no uniformity gradient on the item side either way


@functools.lru_cache(maxsize=None)
def reference(case):
    return case_reference(case)


def test_the_cases_cover_every_value_of_every_axis_with_every_d():
    assert len(CASES) == 24
    for d in (32, 64, 128, 256):
        mine = [c for c in CASES if c[0] == d]
        assert {c[1] for c in mine} == {1, 2, T + 3, 2 * T + 5}
        for axis, values in ((2, {2.0, 10.0}), (3, {1.0, 5.0}), (4, {"keep", "drop"}), (5, {True, False}), (6, {True, False})):
            assert {c[axis] for c in mine} == values
    for case in CASES:
        d, B, t, gamma, same, grouped, distinct = case
        c = parity_case(*case)
        assert c["users"].shape == c["pos"].shape == (B,) and c["U"].shape[1] == d and c["I"].shape[0] == 40
        norms = np.linalg.norm(c["U"], axis=1)
        assert 0.69 < norms.min() and norms.max() < 1.31                # norm near 1
        if distinct:
            assert len(np.unique(c["users"])) == B                      # the precondition of PDA_UPD_USERS_DISTINCT
        elif B > 20:
            assert len(np.unique(c["users"])) < B
        if grouped:
            assert (np.diff(c["pos"]) >= 0).all()
        if B > T:
            assert len(np.unique(c["pos"])) < B                         # items repeat inside the batch


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_float32_restatement_stays_inside_the_gpu_bound(case):
    """tests/test_gpu_dau.py holds the kernels to tolerance(t, gamma) on these very inputs: the restatement itself, computed in float32, stays
    inside a quarter of it, so the bound asks nothing float32 arithmetic cannot give."""
    tol = tolerance(case[2], case[3])
    assert tol == 1e-5 * max(1.0, 2 * case[2] * case[3]) and 4e-5 <= tol <= 1e-3
    w = worst(reference(case), case_reference(case, dtype=torch.float32))
    print("DirectAU float32 restatement %s: worst error %.3g (bound %.3g)" % (case_id(case), w, tol))
    assert w <= tol / 4, (w, tol)


def test_three_adam_steps_in_float32_stay_inside_the_gpu_bound():
    r64, _ = dr.adam_reference()
    r32, _ = dr.adam_reference(dtype=torch.float32)
    w = max(np.abs(r64[k] - r32[k]).max() for k in r64)
    print("DirectAU three steps in float32: worst error %.3g (bound %.3g)" % (w, 1e-5))
    assert w <= 1e-5 / 4, w


def takes_part(mutant, case):
    d, B, t, gamma, same, grouped, distinct = case
    c = parity_case(*case)
    dup = B > 1 and (len(np.unique(c["pos"])) < B or len(np.unique(c["users"])) < B)
    if mutant in ("no_proj", "align_unnormalised"):
        return True                                                     # (the alignment term is there at B = 1)
    if mutant == "uni_per_row":
        return B > 2                                                    # (two rows: each row's mean is the global one)
    if mutant == "same_dropped":
        return same == "keep" and dup
    if mutant == "same_kept":
        return same == "drop" and dup
    return B > 1 and gamma > 0                                          # diag_kept, half_gamma_missing, t_not_in_grad, reg_per_occurrence


@pytest.mark.parametrize("mutant", MUTANTS)
def test_a_broken_contract_is_outside_the_bound_on_the_gpu_inputs(mutant):
    """The GPU comparison has power: each restatement with one clause broken differs from the contract by more than the bound, in a loss term
    or a gradient element, on EVERY case of the GPU tests its clause takes part in (a batch of one row has no pair: only its alignment and
    its regulariser are left)."""
    n, smallest = 0, np.inf
    for case in CASES:
        if not takes_part(mutant, case):
            continue
        tol = tolerance(case[2], case[3])
        w = worst(reference(case), case_reference(case, mutant=mutant))
        print("DirectAU mutant %s on %s: differs by %.3g (bound %.3g)" % (mutant, case_id(case), w, tol))
        assert w > tol, (mutant, case, w)
        smallest = min(smallest, w / tol)
        n += 1
    print("DirectAU mutant %s: %d cases, smallest difference %.3g x the bound" % (mutant, n, smallest))
    assert n >= {"no_proj": 24, "align_unnormalised": 24, "uni_per_row": 16, "same_dropped": 8, "same_kept": 8}.get(mutant, 20)
