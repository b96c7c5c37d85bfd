"""CPU suite for the IPS baselines (`--train ips`, include/pda_hip_ips.h): the flags, the refusals, the weights against numpy, the binding against
the header, the entry points' argument checks (all before any HIP call), the checkpoint, the restatement of tests/ips_ref.py against a closed
form, and the float32 restatement inside the bounds the GPU suite holds the kernels to."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from ips_ref import BATCHES, COUNTS, DIMS, VARIANTS, ips_grads, ips_weights, parity_case, tolerance
from test_abi import declared_in

ERR_ARG, ERR_UNSUPPORTED = -1, -2
CONFIG = {"n_users": 9, "n_items": 12}


def make_args(**over):
    from pda_amd.parse import parse_args
    a = parse_args(["--train", "ips", "--embed_size", "32", "--batch_size", "16"])
    for k, v in over.items():
        setattr(a, k, v)
    return a


# ---- flags and refusals --------------------------------------------------------------------------------------------------------------------
def test_flags_parse_and_the_reference_flags_stay():
    from pda_amd import parse
    a = parse.parse_args([])
    assert (a.ips_clip, a.ips_norm) == (0.0, 0) and isinstance(a.ips_clip, float) and isinstance(a.ips_norm, int)
    b = parse.parse_args("--train ips --test ips --ips_clip 8 --ips_norm 1".split())
    assert (b.train, b.test, b.ips_clip, b.ips_norm) == ("ips", "ips", 8.0, 1)
    ext = [f[0] for f in parse._EXTENSION_FLAGS]
    assert ext[-9:-7] == ["ips_clip", "ips_norm"] and ext[-7] == "dice_int_weight"          # in front of the DICE block
    assert not set(ext) & set(parse.reference_flag_names()) and parse.reference_flag_names()[:5] == ["data_path", "dataset", "source", "train", "test"]


@pytest.mark.parametrize("over, flag", [({"deterministic": 1}, "--deterministic"), ({"table_dtype": "bf16"}, "--table_dtype"),
                                        ({"optimizer": "sgd"}, "--optimizer"), ({"optimizer": "lazy_adam"}, "--optimizer"),
                                        ({"adam_sweep": "replay"}, "--adam_sweep"), ({"adam_sweep": "replay_fast"}, "--adam_sweep"),
                                        ({"gpus": 2}, "--gpus")])
def test_refused_options_name_their_flag(over, flag):
    from pda_amd.model_api import IPSBPRMF
    with pytest.raises(NotImplementedError, match=flag):
        IPSBPRMF(make_args(**over), CONFIG, device="cpu")


@pytest.mark.parametrize("over, flag", [({"ips_clip": -1.0}, "--ips_clip"), ({"ips_clip": float("nan")}, "--ips_clip"), ({"ips_norm": 2}, "--ips_norm"),
                                        ({"ips_norm": -1}, "--ips_norm")])
def test_bad_values_are_value_errors_that_name_their_flag(over, flag):
    from pda_amd.model_api import IPSBPRMF
    with pytest.raises(ValueError, match=flag):
        IPSBPRMF(make_args(**over), CONFIG, device="cpu")


def test_the_trainer_refuses_a_test_mode_ips_does_not_have(monkeypatch):
    from pda_amd import train_new_api as t
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(test="s_condition")))
    with pytest.raises(NotImplementedError, match="--train ips goes with --test normal"):
        t.main([])
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(test="normal", optimizer="sgd")))
    with pytest.raises(NotImplementedError, match="--optimizer"):
        t.main([])
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(test="ips", ips_norm=3)))
    with pytest.raises(ValueError, match="--ips_norm"):
        t.main([])


# ---- the weights -----------------------------------------------------------------------------------------------------------------------------
TOY = np.array([7, 0, 1, 3, 21, 2], dtype=np.int64)         # a zero-count item; 21 / 7 = 3 and 21 / 3 = 7 exactly, 21 / 2 = 10.5


def test_weights_equal_numpy_on_a_toy_count_vector():
    from pda_amd import ops
    w = ops.IpsWeights.from_counts(TOY)
    assert w.ipw.dtype == torch.float32 and w.n_items == 6
    np.testing.assert_array_equal(w.ipw.numpy(), np.array([3, 21, 21, 7, 1, 10.5], dtype=np.float32))       # the zero-count item counts as one
    np.testing.assert_array_equal(w.ipw.numpy(), ips_weights(TOY)[1])
    c = ops.IpsWeights.from_counts(TOY, clip=8.0)
    np.testing.assert_array_equal(c.ipw.numpy(), np.array([3, 8, 8, 7, 1, 8], dtype=np.float32))
    np.testing.assert_array_equal(c.ipw.numpy(), ips_weights(TOY, 8.0)[1])
    # from the train CSR's column ids: the same counts
    idx = torch.from_numpy(np.repeat(np.arange(6), TOY).astype(np.int32))
    np.testing.assert_array_equal(ops.IpsWeights(idx, 6, clip=8.0).ipw.numpy(), c.ipw.numpy())
    with pytest.raises(ValueError, match="ips_clip"):
        ops.IpsWeights.from_counts(TOY, clip=-2.0)
    with pytest.raises(ValueError, match="outside the catalogue"):
        ops.IpsWeights(idx, 5)


def test_weights_are_float64_then_cast():
    """max_j n_j = 3 and n_i = 1 ... : 1 / (n / 3) in float64, rounded to float32 ONCE -- not the float32 quotient of float32 operands, and a clip
    that float32 cannot hold is applied in float64."""
    from pda_amd import ops
    counts = np.array([3, 1, 2, 49, 7, 10], dtype=np.int64)
    got = ops.IpsWeights.from_counts(counts).ipw.numpy()
    want = (1.0 / (counts.astype(np.float64) / 49.0)).astype(np.float32)
    np.testing.assert_array_equal(got, want)
    f32_path = np.float32(1) / (counts.astype(np.float32) / np.float32(49))
    assert (f32_path != want).any()                                     # the two rules do differ on these counts
    clip = 4.9000000001
    np.testing.assert_array_equal(ops.IpsWeights.from_counts(counts, clip=clip).ipw.numpy(), np.minimum(1.0 / (counts / 49.0), clip).astype(np.float32))
    # the counts of the gradient tests: the unclipped weights span [1, 16] exactly
    assert sorted(set(ips_weights(COUNTS)[1])) == [1, 2, 4, 8, 16] and sorted(set(ips_weights(COUNTS, 4.0)[1])) == [1, 2, 4]


def test_item_counts_from_the_loader_lists():
    from pda_amd.model_api import ips_item_counts
    lists = {0: [1, 3], 1: [], 2: [3, 4, 5], 7: [3]}
    np.testing.assert_array_equal(ips_item_counts(lists, 7), [0, 1, 0, 3, 1, 1, 0])


# ---- the binding and the argument checks ---------------------------------------------------------------------------------------------------
def test_binding_equals_the_header():
    from pda_amd import _lib
    names = ["pda_ips_adam_step_f32", "pda_ips_step_f32", "pda_ips_weight_sum"]
    assert declared_in("pda_hip_ips.h") == sorted(_lib.IPS_SIGNATURES) == names
    for d in (_lib.SIGNATURES, _lib.TEMP_POP_SIGNATURES, _lib.PC_SIGNATURES, _lib.DET_SIGNATURES, _lib.DEEP_SIGNATURES, _lib.XQUAD_SIGNATURES,
              _lib.DICE_SIGNATURES):
        assert not set(names) & set(d)
    assert not set(names) & (set(declared_in("pda_hip.h")) | set(declared_in("pda_hip_experimental.h")))
    lib = _lib.load()
    for n in names:
        assert getattr(lib, n).argtypes == _lib.IPS_SIGNATURES[n][1]


def test_entry_points_check_arguments_without_gpu():
    from pda_amd import _lib
    lib = _lib.load()
    keep = C.create_string_buffer(4096)
    b, null = C.c_void_p(C.addressof(keep)), C.c_void_p(None)

    def wsum(ipw=b, users=b, out=b, B=8, nu=9, ni=12):
        return lib.pda_ips_weight_sum(ipw, nu, ni, users, b, b, B, out, null)

    assert wsum(ipw=null) == ERR_ARG and wsum(users=null) == ERR_ARG and wsum(out=null) == ERR_ARG and wsum(B=0) == ERR_ARG
    assert wsum(nu=0) == ERR_ARG and wsum(ni=0) == ERR_ARG and wsum(ni=1 << 31) == ERR_ARG

    def step(U=b, users=b, ipw=b, gU=b, tagI=b, B=8, d=32, reg_div=8.0, tag=1, flags=0x100, nu=9, ni=12):
        return lib.pda_ips_step_f32(U, b, nu, ni, users, b, b, ipw, null, B, d, 1e-3, reg_div, gU, b, b, tagI, tag, flags, null, null)

    assert step(U=null) == ERR_ARG and step(users=null) == ERR_ARG and step(ipw=null) == ERR_ARG and step(gU=null) == ERR_ARG and step(tagI=null) == ERR_ARG
    assert step(B=0) == ERR_ARG and step(reg_div=0.0) == ERR_ARG and step(reg_div=float("nan")) == ERR_ARG and step(tag=0) == ERR_ARG
    assert step(nu=0) == ERR_ARG and step(ni=0) == ERR_ARG and step(flags=0x400) == ERR_ARG and step(flags=2) == ERR_ARG
    assert step(d=16) == ERR_UNSUPPORTED and step(d=48) == ERR_UNSUPPORTED and step(d=512) == ERR_UNSUPPORTED

    def adam(m=b, ipw=b, policy=0, d=64, flags=0x300, B=8):
        return lib.pda_ips_adam_step_f32(b, m, b, b, b, 9, b, b, b, b, b, 12, b, b, b, ipw, b, B, d, 1e-3, 8.0, 1, 1e-3, 0.9, 0.999, 1e-8, flags, policy,
                                         null, null)

    assert adam(m=null) == ERR_ARG and adam(ipw=null) == ERR_ARG and adam(policy=5) == ERR_ARG and adam(policy=-1) == ERR_ARG and adam(flags=1) == ERR_ARG
    assert adam(B=-3) == ERR_ARG and adam(d=8) == ERR_UNSUPPORTED
    del keep


def test_ops_refuses_bad_batches_before_the_library():
    from pda_amd import ops
    U, I = torch.zeros(9, 32), torch.zeros(12, 32)
    i4 = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="HBM"):
        ops.ips_grads(U, I, i4, i4, i4, torch.ones(12), U.clone(), I.clone(), torch.zeros(9, dtype=torch.int32), torch.zeros(12, dtype=torch.int32),
                      regs=1e-3, reg_div=4, step=1)
    with pytest.raises(ValueError, match="HBM"):
        ops.ips_weight_sum(torch.ones(12), i4, i4, i4, 9)


# ---- the model and its checkpoint ----------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_and_a_bprmf_loads_it():
    from pda_amd.model_api import BPRMF, IPSBPRMF
    a = IPSBPRMF(make_args(ips_clip=8.0, ips_norm=1), dict(CONFIG, ips_item_counts=np.arange(12)), device="cpu", seed=1)
    np.testing.assert_array_equal(a.ips.ipw.numpy(), ips_weights(np.arange(12), 8.0)[1])
    assert isinstance(a, BPRMF) and [f.name for f in (a.opt, a.loss, a.mf_loss, a.reg_loss, a.batch_ratings)] == ["opt", "loss", "mf_loss", "reg_loss",
                                                                                                                   "batch_ratings"]
    st = a._opt_state()
    g = torch.Generator().manual_seed(4)
    for k in ("mU", "vU", "mI", "vI"):
        st[k].copy_(torch.rand(st[k].shape, generator=g))
    a._t = 17
    buf = io.BytesIO()
    torch.save(a.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf)
    plain = BPRMF(make_args(train="normal"), CONFIG, device="cpu", seed=2)
    keys = set(plain.state_dict()) | {"mU", "vU", "mI", "vI"}
    assert set(sd) == keys | {"ips_clip", "ips_norm"} and sd["format"] == "pda_amd/2" and "model" not in sd
    assert (sd["ips_clip"], sd["ips_norm"], sd["adam_t"], sd["embed_size"]) == (8.0, 1, 17, 32)
    for m in (plain, IPSBPRMF(make_args(), CONFIG, device="cpu", seed=3)):        # (a model that only evaluates needs no item counts)
        assert not torch.equal(a.weights["user_embedding"], m.weights["user_embedding"])
        m.load_state_dict(sd)
        for k in ("user_embedding", "item_embedding"):
            assert torch.equal(a.weights[k], m.weights[k])
        for k in ("mU", "vU", "mI", "vI"):
            assert torch.equal(st[k], m._state[k])
        assert m._t == 17
    a.load_state_dict(plain.state_dict())                                        # and the other way round
    with pytest.raises(ValueError, match="embed_size"):
        IPSBPRMF(make_args(embed_size=64), CONFIG, device="cpu").load_state_dict(sd)
    with pytest.raises(ValueError, match="one number per item"):
        IPSBPRMF(make_args(), dict(CONFIG, ips_item_counts=np.arange(11)), device="cpu")
    with pytest.raises(ValueError, match="train interactions per item"):
        IPSBPRMF(make_args(), CONFIG, device="cpu").train_step(None, None, None)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [False, True])
def test_restated_gradients_match_the_closed_form(norm):
    """ips_grads (autograd) against the closed form of the contract in float64: the coefficient of every triplet's log-sigmoid is w_t / B or
    w_t / S, and the L2 term is unweighted."""
    rng = np.random.default_rng(3)
    nU, nI, d, B = 7, 9, 4, 16
    U, I = rng.standard_normal((nU, d)) * 0.4, rng.standard_normal((nI, d)) * 0.4
    users, pos, neg = rng.integers(0, nU, B), rng.integers(0, nI, B), rng.integers(0, nI, B)
    ipw = ips_weights(rng.integers(0, 30, nI), 6.0)[1]
    terms, gU, gI = ips_grads(U, I, users, pos, neg, ipw, norm=norm, regs=1e-2, reg_div=B)
    sg = lambda x: 1 / (1 + np.exp(-x))                                # noqa: E731
    dl = lambda x: sg(x) * (1 - sg(x)) / (sg(x) + 1e-10)               # noqa: E731  d log(sigmoid(x) + 1e-10) / dx
    den = float(ipw[pos].astype(np.float64).sum()) if norm else B
    eU, eI, mf, c = np.zeros_like(U), np.zeros_like(I), 0.0, 1e-2 / B
    for u, p, n in zip(users, pos, neg):
        x = U[u] @ I[p] - U[u] @ I[n]
        gx = -float(ipw[p]) / den * dl(x)
        mf -= float(ipw[p]) / den * np.log(sg(x) + 1e-10)
        eU[u] += gx * (I[p] - I[n]) + c * U[u]
        eI[p] += gx * U[u] + c * I[p]
        eI[n] += -gx * U[u] + c * I[n]
    np.testing.assert_allclose(gU, eU, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(gI, eI, rtol=1e-10, atol=1e-14)
    assert terms[1] == pytest.approx(mf, rel=1e-12) and terms[0] == pytest.approx(terms[1] + terms[2], rel=1e-14)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("d", DIMS)
def test_the_float32_restatement_stays_inside_the_gpu_bounds(d, B, variant):
    """tests/test_gpu_ips.py holds the kernels to tolerance() on these very inputs: the restatement itself, computed in float32, stays inside
    them with a factor of four to spare, so the bounds ask nothing float32 arithmetic cannot give."""
    U, I, b, ipw, norm = parity_case(d, B, variant)
    kw = dict(norm=norm, regs=1e-2, reg_div=B)
    t64, gU64, gI64 = ips_grads(U, I, *b, ipw, **kw)
    t32, gU32, gI32 = ips_grads(U, I, *b, ipw, dtype=torch.float32, **kw)
    tol = tolerance(ipw, b[1], norm)
    assert tol == (1e-5 if norm else 1e-5 * float(ipw[b[1]].max())) and tol <= 16e-5
    worst = max(np.abs(t64 - t32).max(), np.abs(gU64 - gU32).max(), np.abs(gI64 - gI32).max())
    assert worst <= tol / 4, (worst, tol)
