"""CPU suite for the popularity-correlation regulariser (`--train pcc`, include/pda_hip_pcc.h): the closed form of the penalty's gradient against
autograd, the float32 restatement inside the bounds the GPU suite holds the kernels to, the sign of the step, the flags, the refusals, the
directory suffix, the binding against the header and the entry points' argument checks (all before any HIP call), and the checkpoint."""
import ctypes as C
import io
import math

import numpy as np
import pytest
import torch

from pcc_ref import BATCHES, COUNTS, DIMS, ONS, parity_case, pcc_grads, pcc_moments, pcc_pop, pcc_scores, tolerance
from test_abi import declared_in

ERR_ARG, ERR_UNSUPPORTED = -1, -2
CONFIG = {"n_users": 9, "n_items": 12}


def make_args(**over):
    from pda_amd.parse import parse_args
    a = parse_args(["--train", "pcc", "--embed_size", "32", "--batch_size", "16"])
    for k, v in over.items():
        setattr(a, k, v)
    return a


# ---- the objective ---------------------------------------------------------------------------------------------------------------------------
def closed_form(z, q, gamma):
    """d (gamma r^2) / d z_t of the contract, float64 numpy."""
    zb, qb = z.mean(), q.mean()
    Szz, Sqq, Szq = ((z - zb) ** 2).sum(), ((q - qb) ** 2).sum(), ((z - zb) * (q - qb)).sum()
    r = Szq / math.sqrt(Szz * Sqq)
    return 2 * gamma * r / math.sqrt(Szz * Sqq) * ((q - qb) - Szq / Szz * (z - zb))


@pytest.mark.parametrize("B", [2, 3, 7, 67, 2048])
def test_closed_form_of_the_penalty_gradient_equals_autograd(B):
    rng = np.random.default_rng(B)
    z, q = rng.standard_normal(B) * 0.7, pcc_pop(COUNTS)[rng.integers(0, len(COUNTS), B)].astype(np.float64)
    if B == 2:
        q = np.array([1.0, 4.0])         # (two equal popularities would be the degenerate case)
    gamma = 3.0
    zt = torch.tensor(z, requires_grad=True)
    st = pcc_moments(zt, torch.tensor(q))
    assert not st["by_rule"]
    (gamma * st["r"] ** 2).backward()
    want, got = zt.grad.numpy(), closed_form(z, q, gamma)
    # relative to the size of the coefficient's terms: its two terms cancel (entirely for B = 2, where r^2 = 1 whatever z is), and what is left of
    # them is rounding of that size
    r, Szz, Sqq = (float(st[k].detach()) for k in ("r", "Szz", "Sqq"))
    scale = 2 * gamma * abs(r) / math.sqrt(Szz * Sqq) * np.abs(q - q.mean()).max()
    assert np.abs(got - want).max() <= 1e-12 * scale, (np.abs(got - want).max(), scale)
    if B > 2:
        assert np.abs(want).max() > 1e-3 * scale


def test_degenerate_moments_are_exact():
    q = torch.full((5,), float(np.float32(3.7)), dtype=torch.float64)
    st = pcc_moments(torch.arange(5, dtype=torch.float64), q)
    assert float(st["Sqq"]) == 0.0 and st["by_rule"] and float(st["r"]) == 0.0
    st = pcc_moments(torch.tensor([0.3]), torch.tensor([2.0]))
    assert float(st["Szz"]) == 0.0 and st["by_rule"] and float(st["r"]) == 0.0


@pytest.mark.parametrize("gamma", [1.0, 10.0])
@pytest.mark.parametrize("on", ONS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("d", DIMS)
def test_the_float32_restatement_stays_inside_the_gpu_bounds(d, B, on, gamma):
    """tests/test_gpu_pcc.py holds the kernels to tolerance() on these very inputs: the restatement itself, computed in float32, stays inside
    them with a factor of four to spare, so the bounds ask nothing float32 arithmetic cannot give."""
    U, I, b, pop = parity_case(d, B)
    kw = dict(gamma=gamma, on=on, regs=1e-2, reg_div=B)
    t64, gU64, gI64, st = pcc_grads(U, I, *b, pop, **kw)
    t32, gU32, gI32, _ = pcc_grads(U, I, *b, pop, dtype=torch.float32, **kw)
    tol = tolerance(gamma, st)
    if st[4] > 0:
        assert st[6] != 0.0 and tol == 1e-5 * max(1.0, 4 * gamma / math.sqrt(st[3]))
    else:                                # (B = 2 at d = 32 and 128: both positives are equally popular, r = 0 by rule)
        assert B == 2 and st[6] == 0.0 and tol == 1e-5
    worst = max(np.abs(t64 - t32).max(), np.abs(gU64 - gU32).max(), np.abs(gI64 - gI32).max())
    assert worst <= tol / 4, (worst, tol)


@pytest.mark.parametrize("on", ONS)
def test_steps_on_the_penalty_alone_lower_r_squared(on):
    """Forty plain gradient steps on gamma r^2 alone (float64, d = 32, B = 67): r^2 never rises and ends below half of where it started -- the
    sign of the coefficient, and on which rows it lands.  The step: |d r^2 / d z| <= 4 / sqrt(Szz) and the rows' norms are O(1), so a step of
    0.05 moves z by a small fraction of its spread."""
    U, I, b, pop = parity_case(32, 67)
    U, I = U.astype(np.float64), I.astype(np.float64)
    lr, trace = 0.05, []
    for _ in range(41):
        terms, gU, gI, st = pcc_grads(U, I, *b, pop, gamma=1.0, on=on, regs=0.0, reg_div=67)
        trace.append(st[6] ** 2)
        # the gradient of the penalty alone: the whole gradient minus the BPR one (gamma = 0)
        _, bU, bI, _ = pcc_grads(U, I, *b, pop, gamma=0.0, on=on, regs=0.0, reg_div=67)
        U, I = U - lr * (gU - bU), I - lr * (gI - bI)
    assert trace[0] > 1e-4
    assert all(b2 <= a2 for a2, b2 in zip(trace, trace[1:])), trace
    assert trace[-1] < 0.5 * trace[0], (trace[0], trace[-1])


def test_the_restatement_adds_the_coefficient_where_the_contract_says():
    """pos: the negative's row takes the BPR gradient alone; margin: the coefficient reaches it negated."""
    U, I, b, pop = parity_case(32, 7)
    U, I = U.astype(np.float64), I.astype(np.float64)
    users, pos, neg = (torch.as_tensor(np.asarray(a, dtype=np.int64)) for a in b)
    Ut, It = torch.tensor(U, dtype=torch.float64), torch.tensor(I, dtype=torch.float64)
    for on in ONS:
        sp, sn, z = pcc_scores(Ut, It, users, pos, neg, on)
        assert torch.equal(z, sp if on == "pos" else sp - sn)
        c = closed_form(z.numpy(), pop[b[1]].astype(np.float64), 2.0)
        _, gU, gI, _ = pcc_grads(U, I, *b, pop, gamma=2.0, on=on, regs=0.0, reg_div=7)
        _, bU, bI, _ = pcc_grads(U, I, *b, pop, gamma=0.0, on=on, regs=0.0, reg_div=7)
        eU, eI = np.zeros_like(gU), np.zeros_like(gI)
        for t, (u, p, n) in enumerate(zip(*b)):
            eU[u] += c[t] * (I[p] - (I[n] if on == "margin" else 0))
            eI[p] += c[t] * U[u]
            if on == "margin":
                eI[n] -= c[t] * U[u]
        np.testing.assert_allclose(gU - bU, eU, rtol=1e-9, atol=1e-13)
        np.testing.assert_allclose(gI - bI, eI, rtol=1e-9, atol=1e-13)


# ---- flags and refusals --------------------------------------------------------------------------------------------------------------------
def test_flags_parse_and_the_reference_flags_stay():
    from pda_amd import parse
    a = parse.parse_args([])
    assert (a.pcc_gamma, a.pcc_on, a.pcc_pop) == (1.0, "pos", "count") and isinstance(a.pcc_gamma, float)
    b = parse.parse_args("--train pcc --test pcc --pcc_gamma 2.5 --pcc_on margin --pcc_pop log".split())
    assert (b.train, b.test, b.pcc_gamma, b.pcc_on, b.pcc_pop) == ("pcc", "pcc", 2.5, "margin", "log")
    ext = [f[0] for f in parse._EXTENSION_FLAGS]
    at = ext.index("pcc_gamma")
    assert ext[at:at + 3] == ["pcc_gamma", "pcc_on", "pcc_pop"]
    assert not set(ext) & set(parse.reference_flag_names()) and parse.reference_flag_names()[:5] == ["data_path", "dataset", "source", "train", "test"]
    assert "untuned" in {f[0]: f[3] for f in parse._EXTENSION_FLAGS}["pcc_gamma"].lower()


@pytest.mark.parametrize("over, flag", [({"deterministic": 1}, "--deterministic"), ({"table_dtype": "bf16"}, "--table_dtype"),
                                        ({"optimizer": "sgd"}, "--optimizer"), ({"optimizer": "lazy_adam"}, "--optimizer"),
                                        ({"adam_sweep": "replay"}, "--adam_sweep"), ({"adam_sweep": "replay_fast"}, "--adam_sweep"),
                                        ({"gpus": 2}, "--gpus"), ({"model": "lightgcn"}, "--model lightgcn")])
def test_refused_options_name_their_flag(over, flag):
    from pda_amd.model_api import PCCBPRMF, check_pcc
    with pytest.raises(NotImplementedError, match=flag):
        check_pcc(make_args(**over))
    with pytest.raises(NotImplementedError, match=flag):
        PCCBPRMF(make_args(**over), CONFIG, device="cpu")


@pytest.mark.parametrize("over, flag", [({"pcc_gamma": -1.0}, "--pcc_gamma"), ({"pcc_gamma": float("nan")}, "--pcc_gamma"),
                                        ({"pcc_on": "neg"}, "--pcc_on"), ({"pcc_pop": "share"}, "--pcc_pop")])
def test_bad_values_are_value_errors_that_name_their_flag(over, flag):
    from pda_amd.model_api import PCCBPRMF
    with pytest.raises(ValueError, match=flag):
        PCCBPRMF(make_args(**over), CONFIG, device="cpu")


def test_dns_stays_refused_under_train_pcc():
    from pda_amd.model_api import check_dns
    with pytest.raises(NotImplementedError, match="--neg_sampler dns"):
        check_dns(make_args(neg_sampler="dns"))


def test_the_trainer_refuses_a_test_mode_pcc_does_not_have(monkeypatch):
    from pda_amd import train_new_api as t
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(test="s_condition")))
    with pytest.raises(NotImplementedError, match="--train pcc goes with --test normal"):
        t.main([])
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(test="normal", optimizer="sgd")))
    with pytest.raises(NotImplementedError, match="--optimizer"):
        t.main([])
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(test="pcc", pcc_on="both")))
    with pytest.raises(ValueError, match="--pcc_on"):
        t.main([])


def test_the_tools_name_the_checkpoint_that_train_pcc_writes(tmp_path):
    """export_topk, bpr_pc and xquad accept --train pcc and look for the run directory with the `pcc` suffix train_new_api.main gives it."""
    import inspect

    from pda_amd import bpr_pc, export_topk, synthetic, xquad
    from pda_amd import train_new_api as t
    src = inspect.getsource(t.main)
    assert 'if args.train == "pcc":' in src and 'args.saveID += "pcc"' in src
    toy = str(tmp_path / "data") + "/"
    synthetic.write_dataset(toy + "toy", n_users=60, n_items=40, mean_hist=6)
    save = str(tmp_path / "save") + "/"
    argv = ["--data_path", toy, "--dataset", "toy", "--train", "pcc", "--save_dir", save, "--regs", "0.01", "--lr", "0.002", "--saveID", "x",
            "--pop_exp", "0.22", "--Ks", "[20,50]"]
    want = save + "mf_toy_checkpoint/wd_0.01_lr_0.002_a_0.001_xpop_exp-0.22pcc_train_pcc/best_ckpt.ckpt"
    for tool, extra in ((bpr_pc, []), (xquad, []), (export_topk, ["--export_out", str(tmp_path / "x.npz")])):
        with pytest.raises(FileNotFoundError) as e:
            tool.main(argv + extra)
        assert want in str(e.value), tool.__name__


# ---- the popularities ------------------------------------------------------------------------------------------------------------------------
def test_popularities_equal_numpy_on_a_toy_count_vector():
    from pda_amd import ops
    toy = np.array([7, 0, 1, 3, 21, 2], dtype=np.int64)
    p = ops.PccPop.from_counts(toy)
    assert p.pop.dtype == torch.float32 and p.n_items == 6 and p.mode == "count"
    np.testing.assert_array_equal(p.pop.numpy(), toy.astype(np.float32))
    np.testing.assert_array_equal(p.pop.numpy(), pcc_pop(toy))
    lg = ops.PccPop.from_counts(toy, "log")
    np.testing.assert_array_equal(lg.pop.numpy(), np.log1p(toy.astype(np.float64)).astype(np.float32))
    np.testing.assert_array_equal(lg.pop.numpy(), pcc_pop(toy, "log"))
    with pytest.raises(ValueError, match="--pcc_pop"):
        ops.PccPop.from_counts(toy, "share")
    with pytest.raises(ValueError, match="non-negative"):
        ops.PccPop.from_counts(np.array([1, -1]))


# ---- the binding and the argument checks ---------------------------------------------------------------------------------------------------
def test_binding_equals_the_header():
    import os
    import re

    from pda_amd import _lib, ops
    names = ["pda_pcc_adam_step_f32", "pda_pcc_stats_f32", "pda_pcc_step_f32"]
    assert declared_in("pda_hip_pcc.h") == sorted(_lib.PCC_SIGNATURES) == names
    for name in dir(_lib):
        if name.endswith("SIGNATURES") and name != "PCC_SIGNATURES":
            assert not set(names) & set(getattr(_lib, name)), name
    assert not set(names) & (set(declared_in("pda_hip.h")) | set(declared_in("pda_hip_experimental.h")) | set(declared_in("pda_hip_ips.h")))
    lib = _lib.load()
    for n in names:
        assert getattr(lib, n).argtypes == _lib.PCC_SIGNATURES[n][1] and getattr(lib, n).restype is C.c_int
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pda_hip_pcc.h")).read()
    for macro, val in (("PDA_PCC_ON_POS", _lib.PCC_ON_POS), ("PDA_PCC_ON_MARGIN", _lib.PCC_ON_MARGIN), ("PDA_PCC_STAT_WORDS", _lib.PCC_STAT_WORDS)):
        assert int(re.search(r"#define %s (\d+)" % macro, text).group(1)) == val
    assert ops.PCC_ON == {"pos": 0, "margin": 1}
    assert "restated from memory" in text.lower()


def test_entry_points_check_arguments_without_gpu():
    from pda_amd import _lib
    lib = _lib.load()
    keep = C.create_string_buffer(4096)
    b, null = C.c_void_p(C.addressof(keep)), C.c_void_p(None)

    def stats(U=b, users=b, pop=b, z=b, stat=b, B=8, d=32, on=0, nu=9, ni=12):
        return lib.pda_pcc_stats_f32(U, b, nu, ni, users, b, b, pop, B, d, on, z, stat, null)

    assert stats(U=null) == ERR_ARG and stats(users=null) == ERR_ARG and stats(pop=null) == ERR_ARG and stats(z=null) == ERR_ARG
    assert stats(stat=null) == ERR_ARG and stats(B=0) == ERR_ARG and stats(B=-2) == ERR_ARG and stats(on=2) == ERR_ARG and stats(on=-1) == ERR_ARG
    assert stats(nu=0) == ERR_ARG and stats(ni=0) == ERR_ARG and stats(ni=1 << 31) == ERR_ARG
    assert stats(d=16) == ERR_UNSUPPORTED and stats(d=48) == ERR_UNSUPPORTED and stats(d=512) == ERR_UNSUPPORTED

    def step(U=b, users=b, pop=b, z=b, stat=b, gU=b, tagI=b, B=8, d=32, gamma=1.0, on=0, reg_div=8.0, tag=1, flags=0x100, nu=9, ni=12):
        return lib.pda_pcc_step_f32(U, b, nu, ni, users, b, b, pop, z, stat, B, d, gamma, on, 1e-3, reg_div, gU, b, b, tagI, tag, flags, null, null, null)

    assert step(U=null) == ERR_ARG and step(users=null) == ERR_ARG and step(pop=null) == ERR_ARG and step(z=null) == ERR_ARG
    assert step(stat=null) == ERR_ARG and step(gU=null) == ERR_ARG and step(tagI=null) == ERR_ARG
    assert step(B=0) == ERR_ARG and step(gamma=-0.5) == ERR_ARG and step(gamma=float("nan")) == ERR_ARG and step(on=3) == ERR_ARG
    assert step(reg_div=0.0) == ERR_ARG and step(reg_div=float("nan")) == ERR_ARG and step(tag=0) == ERR_ARG
    assert step(nu=0) == ERR_ARG and step(ni=0) == ERR_ARG and step(flags=0x400) == ERR_ARG and step(flags=2) == ERR_ARG
    assert step(d=16) == ERR_UNSUPPORTED and step(d=48) == ERR_UNSUPPORTED and step(d=512) == ERR_UNSUPPORTED

    def adam(m=b, pop=b, z=b, stat=b, policy=0, d=64, gamma=1.0, on=1, flags=0x300, B=8):
        return lib.pda_pcc_adam_step_f32(b, m, b, b, b, 9, b, b, b, b, b, 12, b, b, b, pop, z, stat, B, d, gamma, on, 1e-3, 8.0, 1, 1e-3, 0.9, 0.999,
                                         1e-8, flags, policy, null, null, null)

    assert adam(m=null) == ERR_ARG and adam(pop=null) == ERR_ARG and adam(z=null) == ERR_ARG and adam(stat=null) == ERR_ARG
    assert adam(policy=5) == ERR_ARG and adam(policy=-1) == ERR_ARG and adam(flags=1) == ERR_ARG and adam(gamma=-1.0) == ERR_ARG and adam(on=2) == ERR_ARG
    assert adam(B=-3) == ERR_ARG and adam(d=8) == ERR_UNSUPPORTED and adam(d=48) == ERR_UNSUPPORTED
    del keep


def test_ops_refuses_bad_batches_before_the_library():
    from pda_amd import ops
    U, I = torch.zeros(9, 32), torch.zeros(12, 32)
    i4 = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="HBM"):
        ops.pcc_grads(U, I, i4, i4, i4, torch.ones(12), U.clone(), I.clone(), torch.zeros(9, dtype=torch.int32), torch.zeros(12, dtype=torch.int32),
                      gamma=1.0, regs=1e-3, reg_div=4, step=1)
    with pytest.raises(ValueError, match="HBM"):
        ops.pcc_stats(U, I, i4, i4, i4, torch.ones(12))


# ---- the model and its checkpoint ----------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_and_a_bprmf_loads_it():
    from pda_amd.model_api import BPRMF, PCCBPRMF
    a = PCCBPRMF(make_args(pcc_gamma=2.0, pcc_on="margin", pcc_pop="log"), dict(CONFIG, ips_item_counts=np.arange(12)), device="cpu", seed=1)
    np.testing.assert_array_equal(a.pcc.pop.numpy(), pcc_pop(np.arange(12), "log"))
    assert isinstance(a, BPRMF)
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
    assert set(sd) == keys | {"pcc_gamma", "pcc_on", "pcc_pop"} and sd["format"] == "pda_amd/2" and "model" not in sd
    assert (sd["pcc_gamma"], sd["pcc_on"], sd["pcc_pop"], sd["adam_t"], sd["embed_size"]) == (2.0, "margin", "log", 17, 32)
    for m in (plain, PCCBPRMF(make_args(), CONFIG, device="cpu", seed=3)):        # (a model that only evaluates needs no item counts)
        assert not torch.equal(a.weights["user_embedding"], m.weights["user_embedding"])
        m.load_state_dict(sd)
        for k in ("user_embedding", "item_embedding"):
            assert torch.equal(a.weights[k], m.weights[k])
        assert m._t == 17
    a.load_state_dict(plain.state_dict())                                        # and the other way round
    with pytest.raises(ValueError, match="one number per item"):
        PCCBPRMF(make_args(), dict(CONFIG, ips_item_counts=np.arange(11)), device="cpu")
    with pytest.raises(ValueError, match="train interactions per item"):
        PCCBPRMF(make_args(), CONFIG, device="cpu").train_step(None, None, None)
