"""CPU suite for the in-batch softmax with logQ correction (`--train ssm --ssm_source batch`, include/pda_hip_inbatch.h): the flags and their
place, the refusals, the binding against the header, the entry points' argument checks (all before any HIP call), the logQ table, the
checkpoint, the float32 restatement inside the bound the GPU suite holds the kernels to, and the mutants that suite must be able to tell from
the contract."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import inbatch_ref as ir
from inbatch_ref import CASES, MUTANTS, REGS, T, case_reference, parity_case, tolerance, worst
from test_abi import declared_in

ERR_ARG, ERR_UNSUPPORTED = -1, -2
CONFIG = {"n_users": 9, "n_items": 12}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_args(**over):
    from pda_amd.parse import parse_args
    a = parse_args(["--train", "ssm", "--ssm_source", "batch", "--embed_size", "32", "--batch_size", "16"])
    for k, v in over.items():
        setattr(a, k, v)
    return a


# ---- flags and refusals --------------------------------------------------------------------------------------------------------------------
def test_flags_parse_with_their_defaults_in_front_of_ssm_negs():
    from pda_amd import parse
    a = parse.parse_args([])
    assert (a.ssm_source, a.ssm_logq, a.ssm_mask_train) == ("sampled", 1, 1)
    assert isinstance(a.ssm_logq, int) and isinstance(a.ssm_mask_train, int)
    b = parse.parse_args("--train ssm --ssm_source batch --ssm_logq 0 --ssm_mask_train 0".split())
    assert (b.train, b.ssm_source, b.ssm_logq, b.ssm_mask_train) == ("ssm", "batch", 0, 0)
    ext = [f[0] for f in parse._EXTENSION_FLAGS]
    at = ext.index("ssm_negs")
    assert ext[at - 3:at] == ["ssm_source", "ssm_logq", "ssm_mask_train"] and ext[at:at + 3] == ["ssm_negs", "ssm_tau", "ssm_norm"]
    ref = parse.reference_flag_names()
    assert len(ref) == 54 and not set(ext) & set(ref)
    helps = {f[0]: f[3] for f in parse._EXTENSION_FLAGS}
    assert "unused with --ssm_source batch" in helps["ssm_negs"]


REFUSED = [({"deterministic": 1}, "--deterministic"), ({"table_dtype": "bf16"}, "--table_dtype"), ({"optimizer": "sgd"}, "--optimizer"),
           ({"adam_sweep": "replay"}, "--adam_sweep"), ({"gpus": 2}, "--gpus"), ({"sampler": "host"}, "--sampler")]
BAD_VALUES = [({"ssm_source": "memory"}, "--ssm_source"), ({"ssm_logq": 2}, "--ssm_logq"), ({"ssm_logq": -1}, "--ssm_logq"),
              ({"ssm_mask_train": 2}, "--ssm_mask_train"), ({"batch_size": 1}, "--batch_size"), ({"batch_size": 16385}, "--batch_size"),
              ({"ssm_tau": 0.0}, "--ssm_tau"), ({"ssm_norm": 2}, "--ssm_norm")]


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


def test_the_sampled_source_takes_any_batch_size_and_the_backbone_stays_refused():
    from pda_amd.model_api import check_lightgcn, check_ssm
    check_ssm(make_args(ssm_source="sampled", batch_size=1))
    check_ssm(make_args(batch_size=2))
    check_ssm(make_args(batch_size=16384))
    with pytest.raises(NotImplementedError, match="--model lightgcn --train ssm"):
        check_lightgcn(make_args(model="lightgcn"))


# ---- the binding and the argument checks ---------------------------------------------------------------------------------------------------
NAMES = ["pda_inbatch_adam_step_f32", "pda_inbatch_col_splits", "pda_inbatch_mask", "pda_inbatch_step_f32", "pda_inbatch_workspace_bytes"]


def test_binding_equals_the_header():
    from pda_amd import _lib, ops
    assert declared_in("pda_hip_inbatch.h") == sorted(_lib.INBATCH_SIGNATURES) == NAMES
    for d in (_lib.SIGNATURES, _lib.TEMP_POP_SIGNATURES, _lib.PC_SIGNATURES, _lib.DET_SIGNATURES, _lib.DEEP_SIGNATURES, _lib.XQUAD_SIGNATURES,
              _lib.DICE_SIGNATURES, _lib.IPS_SIGNATURES, _lib.MACR_SIGNATURES, _lib.GCN_SIGNATURES, _lib.EXPOSURE_SIGNATURES, _lib.SSM_SIGNATURES):
        assert not set(NAMES) & set(d)
    assert not set(NAMES) & (set(declared_in("pda_hip.h")) | set(declared_in("pda_hip_experimental.h")) | set(declared_in("pda_hip_ssm.h")))
    lib = _lib.load()
    for n in NAMES:
        assert getattr(lib, n).argtypes == _lib.INBATCH_SIGNATURES[n][1]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pda_hip_inbatch.h")).read(), flags=re.S)
    for n in NAMES:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert len(params.split(",")) == len(_lib.INBATCH_SIGNATURES[n][1]), n
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))      # noqa: E731
    assert _lib.INBATCH_MAX_B == ops.INBATCH_MAX_B == define("PDA_INBATCH_MAX_B") == 16384
    assert ops.INBATCH_ROW_TILE == define("PDA_INBATCH_ROW_TILE") and ops.INBATCH_COL_TILE == define("PDA_INBATCH_COL_TILE")
    assert T == max(ops.INBATCH_ROW_TILE, ops.INBATCH_COL_TILE)


def test_the_splits_and_the_workspace_are_functions_of_the_shape_alone():
    from pda_amd import _lib, ops
    lib = _lib.load()
    assert lib.pda_inbatch_col_splits(0) == 0 and lib.pda_inbatch_col_splits(16385) == 0
    assert ops.inbatch_col_splits(1) == ops.inbatch_col_splits(T) == 1 and ops.inbatch_col_splits(T + 3) > 1
    for B in (1, 2, T, T + 3, 2 * T + 5, 2048, 16384):
        s = ops.inbatch_col_splits(B)
        assert 1 <= s <= -(-B // ops.INBATCH_COL_TILE)
    assert lib.pda_inbatch_workspace_bytes(0, 64) == 0 and lib.pda_inbatch_workspace_bytes(16385, 64) == 0 and lib.pda_inbatch_workspace_bytes(8, 48) == 0
    # linear in B: O(B d + B x column splits), far below the B^2 words of the logit matrix
    for d in (32, 256):
        per_row = [lib.pda_inbatch_workspace_bytes(B, d) / B for B in (2048, 4096, 16384)]
        assert max(per_row) <= 4 * (4 * d + 16 + 2 * 64) and max(per_row) < 4 * 2048
    with pytest.raises(ValueError, match="batch size"):
        ops.inbatch_col_splits(0)
    with pytest.raises(ValueError, match="batch size"):
        ops.inbatch_workspace(16385, 64, "cpu")
    with pytest.raises(ValueError, match="width"):
        ops.inbatch_workspace(8, 48, "cpu")


def test_entry_points_check_arguments_without_gpu():
    from pda_amd import _lib
    lib = _lib.load()
    keep = C.create_string_buffer(1 << 16)
    base = (C.addressof(keep) + 15) & ~15
    b, null, odd = C.c_void_p(base), C.c_void_p(None), C.c_void_p(base + 4)
    big = 1 << 30

    def step(U=b, users=b, pos=b, gU=b, tagI=b, ws=b, B=8, d=32, tau=0.1, norm=1, reg_div=8.0, tag=1, flags=0x100, nu=9, ni=12, wsb=big, logq=null,
             mask=null):
        return lib.pda_inbatch_step_f32(U, b, nu, ni, users, pos, B, d, tau, norm, logq, mask, 1e-3, reg_div, gU, b, b, tagI, tag, flags, ws, wsb,
                                        null, null)

    assert step(U=null) == ERR_ARG and step(users=null) == ERR_ARG and step(pos=null) == ERR_ARG and step(gU=null) == ERR_ARG
    assert step(tagI=null) == ERR_ARG and step(ws=null) == ERR_ARG and step(ws=odd) == ERR_ARG
    assert step(B=0) == ERR_ARG and step(B=-1) == ERR_ARG and step(B=16385) == ERR_ARG
    assert step(tau=0.0) == ERR_ARG and step(tau=-1.0) == ERR_ARG and step(tau=float("nan")) == ERR_ARG and step(tau=float("inf")) == ERR_ARG
    assert step(norm=2) == ERR_ARG and step(norm=-1) == ERR_ARG
    assert step(reg_div=0.0) == ERR_ARG and step(reg_div=float("nan")) == ERR_ARG and step(tag=0) == ERR_ARG
    assert step(nu=0) == ERR_ARG and step(ni=0) == ERR_ARG and step(ni=1 << 31) == ERR_ARG and step(flags=0x400) == ERR_ARG and step(flags=2) == ERR_ARG
    assert step(wsb=0) == ERR_ARG and step(wsb=lib.pda_inbatch_workspace_bytes(8, 32) - 1) == ERR_ARG
    assert step(d=16) == ERR_UNSUPPORTED and step(d=48) == ERR_UNSUPPORTED and step(d=512) == ERR_UNSUPPORTED
    assert step(d=48, B=0) == ERR_ARG                                   # (the argument errors come first)

    def adam(m=b, pos=b, ws=b, policy=0, d=64, flags=0x300, B=8, tau=0.1, norm=0, wsb=big):
        return lib.pda_inbatch_adam_step_f32(b, m, b, b, b, 9, b, b, b, b, b, 12, b, pos, B, d, tau, norm, null, null, 1e-3, 8.0, 1, 1e-3, 0.9,
                                             0.999, 1e-8, flags, policy, ws, wsb, null, null)

    assert adam(m=null) == ERR_ARG and adam(pos=null) == ERR_ARG and adam(ws=null) == ERR_ARG and adam(policy=5) == ERR_ARG and adam(policy=-1) == ERR_ARG
    assert adam(flags=1) == ERR_ARG and adam(B=-3) == ERR_ARG and adam(B=16385) == ERR_ARG and adam(tau=0.0) == ERR_ARG and adam(norm=2) == ERR_ARG
    assert adam(wsb=16) == ERR_ARG and adam(d=8) == ERR_UNSUPPORTED

    def mask(users=b, pos=b, indptr=b, indices=b, out=b, B=8, nu=9, ni=12):
        return lib.pda_inbatch_mask(users, pos, B, indptr, indices, nu, ni, out, null)

    assert mask(users=null) == ERR_ARG and mask(pos=null) == ERR_ARG and mask(indptr=null) == ERR_ARG and mask(indices=null) == ERR_ARG
    assert mask(out=null) == ERR_ARG and mask(B=0) == ERR_ARG and mask(B=16385) == ERR_ARG and mask(nu=0) == ERR_ARG and mask(ni=0) == ERR_ARG
    assert lib.pda_inbatch_workspace_bytes(8, 32) > 0 and lib.pda_inbatch_workspace_bytes(8, 16) == 0 and lib.pda_inbatch_workspace_bytes(-1, 32) == 0
    del keep


def test_ops_refuses_bad_batches_before_the_library():
    from pda_amd import ops
    U, I = torch.zeros(9, 32), torch.zeros(12, 32)
    i4 = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="HBM"):
        ops.inbatch_step(U, I, i4, i4, U.clone(), I.clone(), torch.zeros(9, dtype=torch.int32), torch.zeros(12, dtype=torch.int32),
                         torch.zeros(64, dtype=torch.uint8), tau=0.1, norm=1, regs=1e-3, reg_div=4, step=1)
    with pytest.raises(ValueError, match="HBM"):
        ops.inbatch_mask(i4, i4, torch.zeros(10, dtype=torch.int64), i4, 9, 12)


# ---- logq ---------------------------------------------------------------------------------------------------------------------------------------
def test_logq_against_the_closed_form_on_a_toy_graph():
    """Five users over six items; user 4 is outside the pool in the second half.  q by hand, as fractions."""
    from pda_amd import ops
    rows = [[0, 1], [0], [0, 2, 3], [1, 3], [4]]
    indptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    q = np.array([1 / 2 + 1 + 1 / 3, 1 / 2 + 1 / 2, 1 / 3, 1 / 3 + 1 / 2, 1.0, 0.0]) / 5
    got = ops.inbatch_logq(indptr, indices, 6)
    assert got.dtype == np.float32 and got.shape == (6,)
    np.testing.assert_allclose(np.exp(got[:5].astype(np.float64)), q[:5], rtol=1e-6)
    assert np.exp(got[:5].astype(np.float64)).sum() == pytest.approx(1.0, abs=1e-6)      # over the items that occur
    assert got[5] == got[:5].min() == np.float32(np.log(q[:5].min()))                       # q = 0: the smallest positive q
    pool = np.array([0, 1, 2, 3], dtype=np.int32)
    q4 = np.array([1 / 2 + 1 + 1 / 3, 1 / 2 + 1 / 2, 1 / 3, 1 / 3 + 1 / 2]) / 4
    got4 = ops.inbatch_logq(torch.from_numpy(indptr), torch.from_numpy(indices), 6, torch.from_numpy(pool))
    np.testing.assert_allclose(np.exp(got4[:4].astype(np.float64)), q4, rtol=1e-6)
    assert got4[4] == got4[5] == got4[:4].min() and np.exp(got4[:4].astype(np.float64)).sum() == pytest.approx(1.0, abs=1e-6)
    train = {u: set(r) for u, r in enumerate(rows)}
    np.testing.assert_array_equal(got, ir.logq_ref(train, 6, range(5)))                     # the restatement the GPU tests use
    np.testing.assert_array_equal(got4, ir.logq_ref(train, 6, pool))


def test_the_mask_words_round_trip():
    rng = np.random.default_rng(2)
    for B in (1, 31, 32, 33, 69):
        excl = rng.random((B, B)) < 0.3
        w = ir.pack_mask(excl)
        assert w.shape == (B, (B + 31) // 32) and w.dtype == np.int32
        np.testing.assert_array_equal(ir.unpack_mask(w, B), excl)
        for r, c in ((0, 0), (B - 1, B - 1), (B // 2, B - 1)):
            assert bool((int(w.view(np.uint32)[r, c // 32]) >> (c % 32)) & 1) == bool(excl[r, c])


# ---- the model and its checkpoint ----------------------------------------------------------------------------------------------------------------
def test_checkpoint_adds_the_three_flags_and_an_older_ssm_checkpoint_loads():
    from pda_amd.model_api import SSMBPRMF
    a = SSMBPRMF(make_args(ssm_logq=0, ssm_tau=0.25), CONFIG, device="cpu", seed=1)
    old = SSMBPRMF(make_args(ssm_source="sampled"), CONFIG, device="cpu", seed=2)
    sd, sd_old = a.state_dict(), old.state_dict()
    assert set(sd) == set(sd_old) | {"ssm_source", "ssm_logq", "ssm_mask_train"}
    assert (sd["ssm_source"], sd["ssm_logq"], sd["ssm_mask_train"], sd["ssm_tau"]) == ("batch", 0, 1, 0.25)
    a.load_state_dict(sd_old)                                          # today's --train ssm checkpoint, without the three keys
    assert torch.equal(a.weights["user_embedding"], old.weights["user_embedding"])
    old.load_state_dict(sd)
    assert torch.equal(old.weights["item_embedding"], a.weights["item_embedding"])


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
def test_restated_gradients_match_the_closed_form_of_the_contract():
    """inbatch_grads (autograd) against the formulas of include/pda_hip_inbatch.h written out in numpy float64, for both values of norm."""
    rng = np.random.default_rng(3)
    nU, nI, d, B, tau = 7, 5, 4, 6, 0.3
    U, I = rng.standard_normal((nU, d)) * 0.4, rng.standard_normal((nI, d)) * 0.4
    users, pos = rng.integers(0, nU, B), rng.integers(0, nI, B)
    logq = np.log(rng.random(nI) + 0.1)
    excl = rng.random((B, B)) < 0.3
    c_reg = 1e-2 / B
    for norm in (0, 1):
        terms, gU, gI, l = ir.inbatch_grads(U, I, users, pos, tau=tau, norm=norm, regs=1e-2, reg_div=B, logq=logq, excl=excl)
        nu = np.maximum(np.sqrt((U[users] ** 2).sum(1)), 1e-12) if norm else np.ones(B)
        ni = np.maximum(np.sqrt((I[pos] ** 2).sum(1)), 1e-12) if norm else np.ones(B)
        uh, ih = U[users] / nu[:, None], I[pos] / ni[:, None]
        S = uh @ ih.T / tau - logq[pos][None, :]
        E = ~(excl | (pos[:, None] == pos[None, :])) | np.eye(B, dtype=bool)
        Cm, mf = np.zeros((B, B)), 0.0
        for r in range(B):
            cols = np.flatnonzero(E[r])
            m = S[r, cols].max()
            lse = m + np.log(np.exp(S[r, cols] - m).sum())
            mf += (lse - S[r, r]) / B
            Cm[r, cols] = np.exp(S[r, cols] - lse)
            Cm[r, r] -= 1.0
        Cm /= tau * B
        g, h = Cm @ ih, Cm.T @ uh
        eU, eI = np.zeros_like(U), np.zeros_like(I)
        for r in range(B):
            eU[users[r]] += ((g[r] - (uh[r] @ g[r]) * uh[r]) / nu[r] if norm else g[r]) + c_reg * U[users[r]]
            eI[pos[r]] += ((h[r] - (ih[r] @ h[r]) * ih[r]) / ni[r] if norm else h[r]) + c_reg * I[pos[r]]
        reg = 1e-2 * 0.5 * ((U[users] ** 2).sum() + (I[pos] ** 2).sum()) / B
        np.testing.assert_allclose(gU, eU, rtol=1e-10, atol=1e-14)
        np.testing.assert_allclose(gI, eI, rtol=1e-10, atol=1e-14)
        assert terms[1] == pytest.approx(mf, rel=1e-12) and terms[2] == pytest.approx(reg, rel=1e-12)
        assert terms[0] == pytest.approx(terms[1] + terms[2], rel=1e-14)


def test_a_row_with_every_other_column_excluded_takes_only_the_regulariser():
    rng = np.random.default_rng(5)
    U, I = rng.standard_normal((6, 4)), rng.standard_normal((6, 4))
    users, pos = np.arange(4), np.arange(4)
    excl = np.zeros((4, 4), dtype=bool)
    excl[2, :] = True
    terms, gU, gI, l = ir.inbatch_grads(U, I, users, pos, tau=0.5, norm=1, regs=0.0, reg_div=4, excl=excl)
    assert l[2] == 0.0 and np.abs(gU[2]).max() == 0.0 and np.isfinite(terms).all()


@functools.lru_cache(maxsize=None)
def reference(case):
    return case_reference(case)


def test_the_cases_cover_every_value_of_every_axis_with_every_d():
    assert len(CASES) == 24
    for d in (32, 64, 128, 256):
        mine = [c for c in CASES if c[0] == d]
        assert {c[1] for c in mine} == {1, 2, T + 3, 2 * T + 5}
        for axis, values in ((2, {0, 1}), (3, {1.0, 0.1}), (4, {0, 1}), (5, {0, 1}), (6, {True, False}), (7, {True, False})):
            assert {c[axis] for c in mine} == values
    for case in CASES:
        d, B, norm, tau, use_logq, use_mask, grouped, distinct = case
        c, logq, excl = parity_case(*case)
        assert c["users"].shape == c["pos"].shape == (B,) and c["U"].shape[1] == d
        if distinct:
            assert len(np.unique(c["users"])) == B                      # the precondition of PDA_UPD_USERS_DISTINCT
        elif B > 20:
            assert len(np.unique(c["users"])) < B
        if grouped:
            assert (np.diff(c["pos"]) >= 0).all()
        if B > T:
            assert len(np.unique(c["pos"])) < B                         # equal positives occur
        if use_mask and B > 2:
            share = ir.excluded_share(c["users"], c["pos"], excl)
            print("in-batch case %s: %.1f %% of the off-diagonal pairs excluded" % (case, 100 * share))
            assert 0.05 <= share <= 0.5, (case, share)                  # neither an empty nor a full mask


@pytest.mark.parametrize("case", CASES, ids=lambda c: "d%d-B%d-norm%d-tau%g-logq%d-mask%d-%s-%s" % (c[0], c[1], c[2], c[3], c[4], c[5],
                                                                                                   "grouped" if c[6] else "any",
                                                                                                   "distinct" if c[7] else "rep"))
def test_the_float32_restatement_stays_inside_the_gpu_bound(case):
    """tests/test_gpu_inbatch.py holds the kernels to tolerance(tau) on these very inputs: the restatement itself, computed in float32, stays
    inside a quarter of it, so the bound asks nothing float32 arithmetic cannot give."""
    tol = tolerance(case[3])
    assert tol == (1e-5 if case[3] == 1.0 else 1e-4)
    w = worst(reference(case), case_reference(case, dtype=torch.float32))
    print("in-batch float32 restatement %s: worst error %.3g (bound %.3g)" % (case, w, tol))
    assert w <= tol / 4, (w, tol)


@pytest.mark.parametrize("norm", [0, 1])
def test_three_adam_steps_in_float32_stay_inside_the_gpu_bound(norm):
    r64, _ = ir.adam_reference(norm)
    r32, _ = ir.adam_reference(norm, dtype=torch.float32)
    w = max(np.abs(r64[k] - r32[k]).max() for k in r64)
    print("in-batch three steps in float32, norm=%d: worst error %.3g (bound %.3g)" % (norm, w, 1e-5))
    assert w <= 1e-5 / 4, w


def takes_part(mutant, case):
    d, B, norm, tau, use_logq, use_mask, grouped, distinct = case
    c, logq, excl = parity_case(*case)
    pos = c["pos"]
    dup = B > 1 and len(np.unique(pos)) < B
    if mutant in ("no_logq", "logq_negs_only"):
        return bool(use_logq) and B > 1
    if mutant == "no_mask":
        return bool(use_mask) and B > 2 and bool((excl & (pos[:, None] != pos[None, :])).any())
    if mutant == "equal_pos_kept":       # (a row's positive is a train item of its user: where the mask is given it excludes these pairs as well)
        return dup and not use_mask
    if mutant in ("no_diag", "reg_per_column"):
        return B > 1
    if mutant == "no_tau_grad":
        return tau != 1.0 and B > 1
    return bool(norm) and B > 1                                          # no_proj


@pytest.mark.parametrize("mutant", MUTANTS)
def test_a_broken_contract_is_outside_the_bound_on_the_gpu_inputs(mutant):
    """The GPU comparison has power: each restatement with one clause broken differs from the contract by more than the bound, in a loss term
    or a gradient element, on EVERY case of the GPU tests its clause takes part in (a batch of one row has no other column: only its
    regulariser is left, and no clause of the softmax takes part)."""
    n, smallest = 0, np.inf
    for case in CASES:
        if not takes_part(mutant, case):
            continue
        w = worst(reference(case), case_reference(case, mutant=mutant))
        print("in-batch mutant %s on %s: differs by %.3g (bound %.3g)" % (mutant, case, w, tolerance(case[3])))
        assert w > tolerance(case[3]), (mutant, case, w)
        smallest = min(smallest, w / tolerance(case[3]))
        n += 1
    print("in-batch mutant %s: %d cases, smallest difference %.3g x the bound" % (mutant, n, smallest))
    assert n >= {"no_logq": 12, "logq_negs_only": 12, "no_mask": 8, "equal_pos_kept": 4, "no_diag": 20, "reg_per_column": 20, "no_tau_grad": 8,
                 "no_proj": 8}[mutant]
