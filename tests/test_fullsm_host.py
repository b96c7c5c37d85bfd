"""CPU suite for the full-catalogue softmax (`--train ssm --ssm_source all`, include/pda_hip_fullsm.h): the flags and the refusals, the binding
against the header, the entry points' argument checks (all before any HIP call), the checkpoint, the restatement against the formulas of the
header, the float32 restatement inside the bound the GPU suite holds the kernels to, and the mutants that suite must be able to tell from the
contract."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import fullsm_ref as fr
from fullsm_ref import CASES, MUTANTS, REGS, T, case_id, case_reference, parity_case, tolerance, worst
from test_abi import declared_in

ERR_ARG, ERR_UNSUPPORTED = -1, -2
CONFIG = {"n_users": 9, "n_items": 12}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_args(**over):
    from pda_amd.parse import parse_args
    a = parse_args(["--train", "ssm", "--ssm_source", "all", "--embed_size", "32", "--batch_size", "16"])
    for k, v in over.items():
        setattr(a, k, v)
    return a


# ---- flags and refusals --------------------------------------------------------------------------------------------------------------------
def test_all_is_a_third_source_and_no_flag_is_new():
    from pda_amd import parse
    from pda_amd.model_api import check_ssm
    a = parse.parse_args("--train ssm --ssm_source all --ssm_mask_train 0".split())
    assert (a.train, a.ssm_source, a.ssm_mask_train) == ("ssm", "all", 0)
    check_ssm(a)
    for B in (1, 2, 2048, 16384):
        check_ssm(make_args(batch_size=B))
    ext = [f[0] for f in parse._EXTENSION_FLAGS]
    assert [f for f in ext if f.startswith("ssm_")] == ["ssm_source", "ssm_logq", "ssm_mask_train", "ssm_negs", "ssm_tau", "ssm_norm"]
    helps = {f[0]: f[3] for f in parse._EXTENSION_FLAGS}
    for flag in ("ssm_source", "ssm_mask_train", "ssm_logq", "ssm_negs"):
        assert "all" in helps[flag], flag
    assert "unused with --ssm_source all" in helps["ssm_logq"] and "with --ssm_source all" in helps["ssm_negs"]


REFUSED = [({"deterministic": 1}, "--deterministic"), ({"table_dtype": "bf16"}, "--table_dtype"), ({"optimizer": "sgd"}, "--optimizer"),
           ({"adam_sweep": "replay"}, "--adam_sweep"), ({"adam_sweep": "replay_fast"}, "--adam_sweep"), ({"gpus": 2}, "--gpus"),
           ({"sampler": "host"}, "--sampler")]
BAD_VALUES = [({"ssm_source": "memory"}, "--ssm_source"), ({"ssm_mask_train": 2}, "--ssm_mask_train"), ({"batch_size": 0}, "--batch_size"),
              ({"batch_size": 16385}, "--batch_size"), ({"ssm_tau": 0.0}, "--ssm_tau"), ({"ssm_norm": 2}, "--ssm_norm")]


@pytest.mark.parametrize("over, flag", REFUSED)
def test_every_refusal_of_train_ssm_stays(over, flag):
    from pda_amd.model_api import SSMBPRMF, check_ssm
    with pytest.raises(NotImplementedError, match=flag):
        check_ssm(make_args(**over))
    with pytest.raises(NotImplementedError, match=flag):
        SSMBPRMF(make_args(**over), CONFIG, device="cpu")


@pytest.mark.parametrize("over, flag", BAD_VALUES)
def test_bad_values_are_value_errors_that_name_their_flag(over, flag):
    from pda_amd.model_api import SSMBPRMF
    with pytest.raises(ValueError, match=flag):
        SSMBPRMF(make_args(**over), CONFIG, device="cpu")


def test_the_backbone_stays_refused_and_the_other_sources_keep_their_batch_sizes():
    from pda_amd.model_api import check_lightgcn, check_ssm
    with pytest.raises(NotImplementedError, match="--model lightgcn --train ssm"):
        check_lightgcn(make_args(model="lightgcn"))
    check_ssm(make_args(ssm_source="sampled", batch_size=1))
    with pytest.raises(ValueError, match="--batch_size"):
        check_ssm(make_args(ssm_source="batch", batch_size=1))


# ---- the binding and the argument checks ---------------------------------------------------------------------------------------------------
NAMES = ["pda_fullsm_adam_step_f32", "pda_fullsm_col_splits", "pda_fullsm_step_f32", "pda_fullsm_workspace_bytes"]


def test_binding_equals_the_header():
    from pda_amd import _lib, ops
    assert declared_in("pda_hip_fullsm.h") == sorted(_lib.FULLSM_SIGNATURES) == NAMES
    others = [v for k, v in vars(_lib).items() if k.endswith("SIGNATURES") and k != "FULLSM_SIGNATURES"]
    assert len(others) >= 15
    for d in others:
        assert not set(NAMES) & set(d)
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "pda_hip_fullsm.h":
            assert not set(NAMES) & set(declared_in(h)), h
    lib = _lib.load()
    for n in NAMES:
        assert getattr(lib, n).argtypes == _lib.FULLSM_SIGNATURES[n][1]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pda_hip_fullsm.h")).read(), flags=re.S)
    for n in NAMES:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert len(params.split(",")) == len(_lib.FULLSM_SIGNATURES[n][1]), n
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))      # noqa: E731
    assert _lib.FULLSM_MAX_B == ops.FULLSM_MAX_B == define("PDA_FULLSM_MAX_B") == 16384
    assert ops.FULLSM_ROW_TILE == define("PDA_FULLSM_ROW_TILE") and ops.FULLSM_COL_TILE == define("PDA_FULLSM_COL_TILE")
    assert T == max(ops.FULLSM_ROW_TILE, ops.FULLSM_COL_TILE)


def test_the_splits_and_the_workspace_are_functions_of_the_shape_alone():
    from pda_amd import _lib, ops
    lib = _lib.load()
    assert lib.pda_fullsm_col_splits(100, 0) == 0 and lib.pda_fullsm_col_splits(100, 16385) == 0 and lib.pda_fullsm_col_splits(0, 8) == 0
    assert lib.pda_fullsm_col_splits(1 << 31, 8) == 0
    assert ops.fullsm_col_splits(1, 1) == ops.fullsm_col_splits(T, 16384) == 1
    for nI, B in ((20, 1), (70, 33), (257, 69), (5000, 1), (5000, 69), (20000, 2048), (200000, 2048), (200000, 16384), (2 ** 31 - 1, 16384)):
        s = ops.fullsm_col_splits(nI, B)
        assert 1 <= s <= -(-nI // ops.FULLSM_COL_TILE), (nI, B, s)
    assert ops.fullsm_col_splits(5000, 69) > 1 and ops.fullsm_col_splits(20000, 2048) > 1
    assert lib.pda_fullsm_workspace_bytes(0, 100, 64) == 0 and lib.pda_fullsm_workspace_bytes(16385, 100, 64) == 0
    assert lib.pda_fullsm_workspace_bytes(8, 0, 64) == 0 and lib.pda_fullsm_workspace_bytes(8, 100, 48) == 0
    # below the B x n_items words of the logit matrix (a third of it at worst: d = 256 on the small catalogue, where the per-split partial g_r weigh
    # most): the bit mask is a 32nd of it, the rest is linear in B x d x splits and in n_items
    for d in (32, 256):
        for B, nI in ((2048, 20000), (2048, 200000), (16384, 200000)):
            got = lib.pda_fullsm_workspace_bytes(B, nI, d)
            assert 0 < got <= 4 * B * -(-nI // 32) + 4 * nI + 4 * (B + 31) * (d * (ops.fullsm_col_splits(nI, B) + 1) + 2 * ops.fullsm_col_splits(nI, B) + 16) + 4096
            assert got < 4 * B * nI // 3
    with pytest.raises(ValueError, match="batch size"):
        ops.fullsm_col_splits(100, 0)
    with pytest.raises(ValueError, match="batch size"):
        ops.fullsm_workspace(16385, 100, 64, "cpu")
    with pytest.raises(ValueError, match="n_items"):
        ops.fullsm_workspace(8, 0, 64, "cpu")
    with pytest.raises(ValueError, match="width"):
        ops.fullsm_workspace(8, 100, 48, "cpu")


def test_entry_points_check_arguments_without_gpu():
    """Every argument error comes back before a launch: the pointers are stand-in host addresses no kernel could read."""
    from pda_amd import _lib
    lib = _lib.load()
    keep = C.create_string_buffer(1 << 16)
    base = (C.addressof(keep) + 15) & ~15
    b, null, odd = C.c_void_p(base), C.c_void_p(None), C.c_void_p(base + 4)
    big = 1 << 30

    def step(U=b, users=b, pos=b, gU=b, tagI=b, ws=b, B=8, d=32, tau=0.1, norm=1, reg_div=8.0, tag=1, flags=0x100, nu=9, ni=12, wsb=big,
             indptr=null, indices=null):
        return lib.pda_fullsm_step_f32(U, b, nu, ni, users, pos, B, d, tau, norm, indptr, indices, 1e-3, reg_div, gU, b, b, tagI, tag, flags, ws, wsb,
                                       null, null, null)

    assert step(U=null) == ERR_ARG and step(users=null) == ERR_ARG and step(pos=null) == ERR_ARG and step(gU=null) == ERR_ARG
    assert step(tagI=null) == ERR_ARG and step(ws=null) == ERR_ARG and step(ws=odd) == ERR_ARG
    assert step(indptr=b) == ERR_ARG and step(indices=b) == ERR_ARG                      # the CSR: both or neither
    assert step(B=0) == ERR_ARG and step(B=-1) == ERR_ARG and step(B=16385) == ERR_ARG
    assert step(tau=0.0) == ERR_ARG and step(tau=-1.0) == ERR_ARG and step(tau=float("nan")) == ERR_ARG and step(tau=float("inf")) == ERR_ARG
    assert step(norm=2) == ERR_ARG and step(norm=-1) == ERR_ARG
    assert step(reg_div=0.0) == ERR_ARG and step(reg_div=float("nan")) == ERR_ARG and step(tag=0) == ERR_ARG
    assert step(nu=0) == ERR_ARG and step(ni=0) == ERR_ARG and step(ni=1 << 31) == ERR_ARG and step(flags=0x400) == ERR_ARG and step(flags=2) == ERR_ARG
    assert step(wsb=0) == ERR_ARG and step(wsb=lib.pda_fullsm_workspace_bytes(8, 12, 32) - 1) == ERR_ARG
    assert step(d=16) == ERR_UNSUPPORTED and step(d=48) == ERR_UNSUPPORTED and step(d=512) == ERR_UNSUPPORTED
    assert step(d=48, B=0) == ERR_ARG                                   # (the argument errors come first)

    def adam(m=b, pos=b, ws=b, policy=0, d=64, flags=0x300, B=8, tau=0.1, norm=0, wsb=big, indices=null):
        return lib.pda_fullsm_adam_step_f32(b, m, b, b, b, 9, b, b, b, b, b, 12, b, pos, B, d, tau, norm, null, indices, 1e-3, 8.0, 1, 1e-3, 0.9,
                                            0.999, 1e-8, flags, policy, ws, wsb, null, null, null)

    assert adam(m=null) == ERR_ARG and adam(pos=null) == ERR_ARG and adam(ws=null) == ERR_ARG and adam(policy=5) == ERR_ARG and adam(policy=-1) == ERR_ARG
    assert adam(flags=1) == ERR_ARG and adam(B=-3) == ERR_ARG and adam(B=16385) == ERR_ARG and adam(tau=0.0) == ERR_ARG and adam(norm=2) == ERR_ARG
    assert adam(wsb=16) == ERR_ARG and adam(d=8) == ERR_UNSUPPORTED and adam(indices=b) == ERR_ARG
    assert lib.pda_fullsm_workspace_bytes(8, 12, 32) > 0 and lib.pda_fullsm_workspace_bytes(8, 12, 16) == 0 and lib.pda_fullsm_workspace_bytes(-1, 12, 32) == 0
    del keep


def test_ops_refuses_bad_batches_before_the_library():
    from pda_amd import ops
    U, I = torch.zeros(9, 32), torch.zeros(12, 32)
    i4 = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="HBM"):
        ops.fullsm_step(U, I, i4, i4, U.clone(), I.clone(), torch.zeros(9, dtype=torch.int32), torch.zeros(12, dtype=torch.int32),
                        torch.zeros(64, dtype=torch.uint8), tau=0.1, norm=1, regs=1e-3, reg_div=4, step=1)


# ---- the model and its checkpoint ----------------------------------------------------------------------------------------------------------------
def test_checkpoint_carries_the_source_and_the_mask_flag():
    from pda_amd.model_api import SSMBPRMF
    a = SSMBPRMF(make_args(ssm_mask_train=0, ssm_tau=0.25), CONFIG, device="cpu", seed=1)
    old = SSMBPRMF(make_args(ssm_source="sampled"), CONFIG, device="cpu", seed=2)
    sd, sd_old = a.state_dict(), old.state_dict()
    assert set(sd) == set(sd_old) | {"ssm_source", "ssm_mask_train"}
    assert (sd["ssm_source"], sd["ssm_mask_train"], sd["ssm_tau"]) == ("all", 0, 0.25)
    a.load_state_dict(sd_old)                                          # a sampled run's checkpoint, without the two keys
    assert torch.equal(a.weights["user_embedding"], old.weights["user_embedding"])
    old.load_state_dict(sd)
    assert torch.equal(old.weights["item_embedding"], a.weights["item_embedding"])


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
def test_restated_gradients_match_the_closed_form_of_the_contract():
    """fullsm_grads (autograd) against the formulas of include/pda_hip_fullsm.h written out in numpy float64, for both values of norm."""
    rng = np.random.default_rng(3)
    nU, nI, d, B, tau = 7, 9, 4, 6, 0.3
    U, I = rng.standard_normal((nU, d)) * 0.4, rng.standard_normal((nI, d)) * 0.4
    users, pos = rng.integers(0, nU, B), rng.integers(0, nI, B)
    member = rng.random((B, nI)) < 0.3
    member[np.arange(B), pos] = True                                    # a row's positive is a train item of its user
    c_reg = 1e-2 / B
    for norm in (0, 1):
        terms, gU, gI, l, stats = fr.fullsm_grads(U, I, users, pos, tau=tau, norm=norm, regs=1e-2, reg_div=B, member=member)
        nu = np.maximum(np.sqrt((U[users] ** 2).sum(1)), 1e-12) if norm else np.ones(B)
        ni = np.maximum(np.sqrt((I ** 2).sum(1)), 1e-12) if norm else np.ones(nI)
        uh, ih = U[users] / nu[:, None], I / ni[:, None]
        S = uh @ ih.T / tau
        E = ~member
        E[np.arange(B), pos] = True
        Cm, mf = np.zeros((B, nI)), 0.0
        for r in range(B):
            cols = np.flatnonzero(E[r])
            m = S[r, cols].max()
            se = np.exp(S[r, cols] - m).sum()
            assert stats[r, 0] == pytest.approx(m, rel=1e-12) and stats[r, 1] == pytest.approx(np.log(se), abs=1e-12)
            mf += ((m - S[r, pos[r]]) + np.log(se)) / B
            Cm[r, cols] = np.exp(S[r, cols] - m) / se
            Cm[r, pos[r]] -= 1.0
        Cm /= tau * B
        g, h = Cm @ ih, Cm.T @ uh
        eU, eI = np.zeros_like(U), np.zeros_like(I)
        for r in range(B):
            eU[users[r]] += ((g[r] - (uh[r] @ g[r]) * uh[r]) / nu[r] if norm else g[r]) + c_reg * U[users[r]]
            eI[pos[r]] += c_reg * I[pos[r]]
        for c in range(nI):
            eI[c] += (h[c] - (ih[c] @ h[c]) * ih[c]) / ni[c] if norm else h[c]
        reg = 1e-2 * 0.5 * ((U[users] ** 2).sum() + (I[pos] ** 2).sum()) / B
        np.testing.assert_allclose(gU, eU, rtol=1e-10, atol=1e-14)
        np.testing.assert_allclose(gI, eI, rtol=1e-10, atol=1e-14)
        assert terms[1] == pytest.approx(mf, rel=1e-12) and terms[2] == pytest.approx(reg, rel=1e-12)
        assert terms[0] == pytest.approx(terms[1] + terms[2], rel=1e-14)


def test_a_row_with_every_other_item_excluded_takes_only_the_regulariser():
    rng = np.random.default_rng(5)
    U, I = rng.standard_normal((6, 4)), rng.standard_normal((7, 4))
    users, pos = np.arange(4), np.array([0, 3, 5, 6])
    member = np.zeros((4, 7), dtype=bool)
    member[2, :] = True
    terms, gU, gI, l, stats = fr.fullsm_grads(U, I, users, pos, tau=0.5, norm=1, regs=0.0, reg_div=4, member=member)
    assert l[2] == 0.0 and np.abs(gU[2]).max() == 0.0 and stats[2, 1] == 0.0 and np.isfinite(terms).all()


@functools.lru_cache(maxsize=None)
def reference(case):
    return case_reference(case)


def test_the_cases_cover_every_value_of_every_axis_with_every_d():
    from pda_amd import ops
    assert len(CASES) == 24
    for d in (32, 64, 128, 256):
        mine = [c for c in CASES if c[0] == d]
        for axis, values in ((1, {1, 33, 69}), (2, {20, 70, 257, 5000}), (3, {0, 1}), (4, {1.0, 0.1}), (5, {0, 1}), (6, {True, False}),
                             (7, {True, False})):
            assert {c[axis] for c in mine} == values
    for case in CASES:
        d, B, nI, norm, tau, use_mask, distinct, drop = case
        c, member = parity_case(*case)
        assert c["users"].shape == c["pos"].shape == (B,) and c["U"].shape[1] == d and c["I"].shape == (nI, d)
        ok = fr.valid_rows(c["users"], c["pos"], c["nU"], nI)
        assert (~ok).sum() == (5 if drop else 0)
        if distinct:
            assert len(np.unique(c["users"])) == B                      # the precondition of PDA_UPD_USERS_DISTINCT
        elif B > 20:
            assert np.bincount(c["users"][ok]).max() > 2                # users that occur more than twice
        if B > T and nI < 1000:
            assert len(np.unique(c["pos"][ok])) < ok.sum()              # equal positives occur
        if nI == 5000:
            assert ops.fullsm_col_splits(nI, B) > 1
        if use_mask:
            share = member[ok].mean()
            assert 0.1 <= share <= 0.5, (case, share)                   # neither an empty nor a full mask
            assert member[ok][np.arange(ok.sum()), c["pos"][ok]].all()  # a row's positive is a train item of its user


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_float32_restatement_stays_inside_the_gpu_bound(case):
    """tests/test_gpu_fullsm.py holds the kernels to tolerance(tau) on these very inputs: the restatement itself, computed in float32, stays
    inside it, so the bound asks nothing float32 arithmetic cannot give."""
    tol = tolerance(case[4])
    assert tol == (1e-5 if case[4] == 1.0 else 1e-4)
    r64, r32 = reference(case), case_reference(case, dtype=torch.float32)
    w = max(worst(r64, r32), np.abs(r64[4] - r32[4]).max())
    print("full softmax float32 restatement %s: worst error %.3g (bound %.3g)" % (case_id(case), w, tol))
    assert w <= tol, (w, tol)


@pytest.mark.parametrize("norm", [0, 1])
def test_three_adam_steps_in_float32_stay_inside_the_gpu_bound(norm):
    r64, _ = fr.adam_reference(norm)
    r32, _ = fr.adam_reference(norm, dtype=torch.float32)
    w = max(np.abs(r64[k] - r32[k]).max() for k in r64)
    print("full softmax three steps in float32, norm=%d: worst error %.3g (bound %.3g)" % (norm, w, 1e-5))
    assert w <= 1e-5, w


def takes_part(mutant, case):
    d, B, nI, norm, tau, use_mask, distinct, drop = case
    if mutant in ("no_mask", "pos_masked"):
        return bool(use_mask)
    if mutant == "no_proj":
        return bool(norm)
    if mutant == "no_tau_grad":
        return tau != 1.0
    if mutant == "mean_over_valid":
        return bool(drop)
    if mutant == "last_tile_dropped":
        return nI % T != 0
    return True                                                          # reg_per_column


@pytest.mark.parametrize("mutant", MUTANTS)
def test_a_broken_contract_is_outside_the_bound_on_the_gpu_inputs(mutant):
    """The GPU comparison has power: each restatement with one clause broken differs from the contract by more than twice the bound, in a loss
    term or a gradient element, on EVERY case of the GPU tests its clause takes part in, and that is at least one case with every d."""
    hit = set()
    for case in CASES:
        if not takes_part(mutant, case):
            continue
        w = worst(reference(case), case_reference(case, mutant=mutant))
        print("full softmax mutant %s on %s: differs by %.3g (2 x bound %.3g)" % (mutant, case_id(case), w, 2 * tolerance(case[4])))
        assert w > 2 * tolerance(case[4]), (mutant, case, w)
        hit.add(case[0])
    assert hit == {32, 64, 128, 256}, (mutant, hit)
