"""CPU suite for the WARP loss (`--train warp`, include/pda_hip_warp.h): the weight table against a direct float64 sum, the vectorised first-violator
search against the plain loop that IS the definition, the step's closed-form float64 gradients against torch.autograd on the stated loss, the
refusals of check_warp, the flags, the binding against the header, the entry points' argument checks (every call carries a violation, so none
reaches a launch), that `--train warp` reaches WARPBPRMF, and the conditions on the inputs that the GPU suite leans on (the chosen margin of the
exact-table sweep, the share of rows the a-priori bound leaves undecided)."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import dns_ref as dr
import warp_ref as wr
from test_abi import declared_in

ERR_ARG, ERR_UNSUPPORTED = -1, -2
NULL = C.c_void_p(None)
NAMES = ["pda_warp_adam_step_f32", "pda_warp_sample_f32", "pda_warp_sample_f32_dev", "pda_warp_step_f32"]
SEED = 2020
INDPTR, INDICES, SLOTS = dr.graph()
POOL = np.arange(dr.NU, dtype=np.int32)[::-1].copy()


def make_args(**over):
    from pda_amd.parse import parse_args
    a = parse_args(["--train", "warp", "--embed_size", "32", "--batch_size", "16"])
    for k, v in over.items():
        setattr(a, k, v)
    return a


# ---- the weight table ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", wr.KINDS)
@pytest.mark.parametrize("n, T", [(200, 64), (200, 256), (2, 3), (1, 1), (37, 7), (100000, 256)])
def test_the_weight_table_is_the_direct_sum(kind, n, T):
    from pda_amd import ops
    w = ops.WarpWeights.build(n, T, kind, "cpu")
    want = wr.weight_table(n, T, kind)
    assert w.table64.shape == (T + 1,) and w.table64[0] == 0.0 and w.wtab[0].item() == 0.0
    np.testing.assert_allclose(w.table64, want, rtol=1e-13, atol=0)      # (a cumulative sum against a sum per entry: a few float64 roundings)
    np.testing.assert_array_equal(w.wtab.numpy(), w.table64.astype(np.float32))      # rounded once
    assert w.wtab.dtype == torch.float32 and w.T == T and w.max_weight == float(w.wtab.max())
    rank = (n - 1) // np.arange(1, T + 1)
    if kind == "log":
        assert (w.table64[1:][rank <= 1] == 0.0).all()                    # 0 at rank 1 (and at rank 0)
        if n == 200 and T >= 100:
            assert w.table64[100] == 0.0 and w.table64[99] > 0.0          # rank(100) = 1, rank(99) = 2
    if kind == "none":
        assert (w.table64[1:] == 1.0).all()
    if kind == "harmonic" and n == 200:
        assert w.table64[1] == sum(1.0 / k for k in range(1, 200)) and (np.diff(w.table64[1:]) <= 0).all()


def test_the_weight_table_refuses_what_it_cannot_build():
    from pda_amd import ops
    for kw, what in ((dict(n_eligible=0, T=4), "n_eligible"), (dict(n_eligible=10, T=0), "T"), (dict(n_eligible=10, T=257), "T"),
                     (dict(n_eligible=10, T=4, kind="sqrt"), "kind")):
        with pytest.raises(ValueError, match=what):
            ops.WarpWeights.build(**kw)


# ---- the first violator ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("margin", [1.0, 0.0, -3.0, math.inf, -math.inf, 0.125])
def test_the_vectorised_search_is_the_plain_loop(margin):
    rng = np.random.default_rng(5)
    B, T = 200, 33
    s = np.round(rng.standard_normal((B, T)) * 2, 1)                      # one decimal: ties between candidates, and with the positive
    sp = np.round(rng.standard_normal(B) * 2, 1)
    s[rng.random((B, T)) < 0.1] = np.nan
    sp[::17] = np.nan
    s[5] = sp[5]                                                          # x == 0 in every column
    s[6, :] = np.inf
    s[7, :] = -np.inf
    sp[8] = np.inf
    want = wr.first_violator_loop(sp, s, margin)
    np.testing.assert_array_equal(wr.first_violator(sp, s, margin), want)
    assert (want[::17] == 0).all()                                        # a NaN positive: no violator
    if margin == math.inf:
        ok = ~np.isnan(sp) & (sp != np.inf) & (np.arange(B) != 7)         # (row 7: x = +inf, inf - inf is a NaN -- no violator there)
        first_number = np.where((~np.isnan(s)).any(1), (~np.isnan(s)).argmax(1) + 1, 0)
        np.testing.assert_array_equal(want[ok], first_number[ok])         # every number violates, a NaN never
        assert want[8] == 0 and want[7] == 0                              # inf - inf
    if margin == -math.inf:
        assert (want[np.arange(B) != 7] == 0).all()
    if margin == 1.0:
        assert 0 < (want == 0).sum() < B and (want > 1).sum() > B // 5


def test_the_masked_outputs_follow_n():
    cand = np.arange(12, dtype=np.int32).reshape(3, 4)
    score = cand.astype(np.float64) + 0.5
    out = wr.outputs_for(np.array([0, 1, 3]), cand, score, np.array([0, 10, 20, 30, 40], dtype=np.float32))
    np.testing.assert_array_equal(out["neg"], [3, 4, 10])
    np.testing.assert_array_equal(out["coef"], [0, 10, 30])
    np.testing.assert_array_equal(out["cand_out"], [[0, 1, 2, 3], [4, -1, -1, -1], [8, 9, 10, -1]])
    np.testing.assert_array_equal(out["score_out"], [[0.5, 1.5, 2.5, 3.5], [4.5, 0, 0, 0], [8.5, 9.5, 10.5, 0]])
    np.testing.assert_array_equal(out["stat"], [4, 1])


# ---- the step --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, B", [(32, 1), (32, 64), (64, 256)])
def test_the_closed_form_gradients_are_autograd_of_the_stated_loss(d, B):
    rng = np.random.default_rng(d + B)
    U, I = (rng.standard_normal((dr.NU, d)) * 0.3), (rng.standard_normal((dr.NI, d)) * 0.3)
    users, pos, neg = (rng.integers(0, n, B) for n in (dr.NU, dr.NI, dr.NI))
    if B > 8:
        pos[: B // 3] = 7                                                 # a hot positive
        neg[3] = pos[3]                                                   # x == 0: active for margin > 0
    coef = rng.choice([0.0, 0.5, 1.0, 5.87], B)
    margin, regs = 0.25, 1e-2
    terms, gU, gI, h = wr.step_grads(U, I, users, pos, neg, coef, margin=margin, regs=regs, reg_div=B)
    Ut, It = torch.tensor(U, requires_grad=True), torch.tensor(I, requires_grad=True)
    t = wr.step_terms_torch(Ut, It, *(torch.as_tensor(a) for a in (users, pos, neg)), torch.as_tensor(coef), margin=margin, regs=regs, reg_div=B)
    t["loss"].backward()
    np.testing.assert_allclose(terms, [float(t[k].detach()) for k in ("loss", "mf", "reg")], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(gU, Ut.grad.numpy(), rtol=0, atol=1e-14)
    np.testing.assert_allclose(gI, It.grad.numpy(), rtol=0, atol=1e-14)
    if B > 8:
        act = (coef > 0) & (h > 0)
        assert 0 < act.sum() < B and ((coef == 0) & (h > 0)).any()        # both kinds of inactive triplet occur
        # an inactive triplet moves its rows by the regulariser alone
        _, rU, rI, _ = wr.step_grads(U, I, users, pos, neg, np.zeros(B), margin=margin, regs=regs, reg_div=B)
        lone = [k for k in range(B) if not act[k] and (users == users[k]).sum() == 1]
        assert lone
        np.testing.assert_array_equal(gU[users[lone]], rU[users[lone]])


# ---- flags and refusals ----------------------------------------------------------------------------------------------------------------------------
def test_flags_parse_and_the_defaults():
    from pda_amd import parse
    from pda_amd.model_api import check_warp
    a = parse.parse_args([])
    assert (a.warp_max_trials, a.warp_margin, a.warp_weight) == (64, 1.0, "harmonic")
    assert isinstance(a.warp_max_trials, int) and isinstance(a.warp_margin, float) and a.train == "normal"
    b = parse.parse_args("--train warp --warp_max_trials 16 --warp_margin 0.5 --warp_weight log".split())
    assert (b.train, b.warp_max_trials, b.warp_margin, b.warp_weight) == ("warp", 16, 0.5, "log")
    check_warp(b)
    ext = [f[0] for f in parse._EXTENSION_FLAGS]
    assert {"warp_max_trials", "warp_margin", "warp_weight"} <= set(ext) and not set(ext) & set(parse.reference_flag_names())


REFUSED = [({"deterministic": 1}, "--deterministic"), ({"table_dtype": "bf16"}, "--table_dtype"), ({"optimizer": "sgd"}, "--optimizer"),
           ({"optimizer": "lazy_adam"}, "--optimizer"), ({"optimizer": "sgd_fused"}, "--optimizer"), ({"adam_sweep": "replay"}, "--adam_sweep"),
           ({"adam_sweep": "replay_fast"}, "--adam_sweep"), ({"adam_exact_lazy": True}, "adam_exact_lazy"), ({"sampler": "host"}, "--sampler"),
           ({"gpus": 2}, "--gpus"), ({"model": "lightgcn"}, "--model"), ({"neg_sampler": "dns"}, "--neg_sampler"),
           ({"neg_sampler": "pop"}, "--neg_sampler"), ({"test": "s_condition"}, "--test"), ({"test": "ips"}, "--test"), ({"test": "macr"}, "--test")]
BAD_VALUES = [({"warp_margin": math.inf}, "--warp_margin"), ({"warp_margin": -math.inf}, "--warp_margin"), ({"warp_margin": math.nan}, "--warp_margin"),
              ({"warp_max_trials": 0}, "--warp_max_trials"), ({"warp_max_trials": 257}, "--warp_max_trials"),
              ({"warp_max_trials": 2.5}, "--warp_max_trials"), ({"warp_weight": "sqrt"}, "--warp_weight"), ({"warp_weight": ""}, "--warp_weight")]


@pytest.mark.parametrize("over, flag", REFUSED)
def test_refused_options_name_their_flag(over, flag):
    from pda_amd.model_api import check_warp
    with pytest.raises(NotImplementedError, match=flag):
        check_warp(make_args(**over))


@pytest.mark.parametrize("over, flag", BAD_VALUES)
def test_bad_values_are_value_errors_that_name_their_flag(over, flag):
    from pda_amd.model_api import check_warp
    with pytest.raises(ValueError, match=flag):
        check_warp(make_args(**over))


@pytest.mark.parametrize("over", [{}, {"test": "warp"}, {"adam_sweep": "sweep"}, {"warp_max_trials": 1}, {"warp_max_trials": 256},
                                  {"warp_margin": -2.0}, {"warp_weight": "log"}, {"warp_weight": "none"}])
def test_what_warp_goes_with_is_let_through(over):
    from pda_amd.model_api import check_warp
    check_warp(make_args(**over))


def test_the_trainer_refuses_before_anything_is_built(monkeypatch):
    from pda_amd import train_new_api as t
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(table_dtype="bf16")))
    with pytest.raises(NotImplementedError, match="--table_dtype"):
        t.main([])
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(test="s_condition")))
    with pytest.raises(NotImplementedError, match="--test"):
        t.main([])
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(warp_max_trials=300)))
    with pytest.raises(ValueError, match="--warp_max_trials"):
        t.main([])


def test_train_warp_reaches_the_model_and_hands_the_sampler_the_live_tables(monkeypatch):
    from pda_amd import train_new_api as t
    built = []

    def fake(args, config, **kw):
        rec = types.SimpleNamespace(weights={"user_embedding": "U", "item_embedding": "I"})
        built.append((args.train, rec))
        return rec

    monkeypatch.setattr(t, "WARPBPRMF", fake)
    got = {}
    sampler = types.SimpleNamespace(distinct_users=True, with_plan=False, mode="warp", set_tables=lambda fn: got.update(fn=fn))
    model = t.DatasetApi_Model(make_args(), {"n_users": 10, "n_items": 10}, 16, sampler, device="cuda")
    assert [b[0] for b in built] == ["warp"] and model.Recommender is built[0][1] and model.input_type == "without_pop"
    assert got["fn"]() == ("U", "I") and model.Recommender.users_distinct is True and sampler.with_plan is False
    built[0][1].weights["user_embedding"] = "U2"                         # the tables AS THEY STAND when the batch is drawn
    assert got["fn"]() == ("U2", "I")


def test_the_model_class_is_a_bprmf_that_checks_its_flags():
    from pda_amd import model_api
    assert issubclass(model_api.WARPBPRMF, model_api.BPRMF)
    with pytest.raises(NotImplementedError, match="--gpus"):
        model_api.WARPBPRMF(make_args(gpus=2), {"n_users": 10, "n_items": 10})


def test_the_device_sampler_refuses_bad_sizes_before_touching_the_device():
    from pda_amd import ops
    from pda_amd.sampler import DeviceSampler
    w = ops.WarpWeights.build(10, 4, "none", "cpu")
    for kw, what in ((dict(max_trials=0, wtab=w), "max_trials"), (dict(max_trials=257, wtab=w), "max_trials"),
                     (dict(max_trials=4, margin=math.nan, wtab=w), "margin"), (dict(max_trials=4, margin=1.0), "wtab"),
                     (dict(max_trials=8, margin=1.0, wtab=w), "wtab")):
        with pytest.raises(ValueError, match=what):
            DeviceSampler(None, "cpu", False, mode="warp", **kw)
    with pytest.raises(ValueError, match="popularity"):
        DeviceSampler(None, "cpu", True, mode="warp", max_trials=4, margin=1.0, wtab=w)


# ---- the binding and the argument checks -----------------------------------------------------------------------------------------------------------
def test_the_library_loads_and_the_binding_equals_the_header():
    import os
    import re
    from pda_amd import _lib
    lib = _lib.load()
    assert declared_in("pda_hip_warp.h") == sorted(_lib.WARP_SIGNATURES) == NAMES
    assert _lib.WARP_MAX_TRIALS == 256
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pda_hip_warp.h")).read()
    assert re.search(r"#define\s+PDA_WARP_MAX_TRIALS\s+256\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NAMES:
        assert getattr(lib, n).argtypes == _lib.WARP_SIGNATURES[n][1] and getattr(lib, n).restype is C.c_int
        params = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % n, text).group(1)
        assert len(params.split(",")) == len(_lib.WARP_SIGNATURES[n][1]), n


def test_every_argument_check_comes_before_a_launch():
    """Every call below carries a violation (or the library would touch a GPU this suite does not have): the code comes back without a launch."""
    from pda_amd import _lib
    lib = _lib.load()
    x = C.c_void_p(4096)                                                  # a non-NULL pointer that is never followed

    def sample(dev=False, U=x, users=x, wtab=x, trials=x, coef=x, pos=x, gen=1, n_pool=5, B=8, nu=10, ni=10, d=64, pop=NULL, n_slots=0, lo=0, hi=10,
               T=4, margin=1.0, pp=NULL, pn=NULL, step_dev=x, step_next=NULL):
        head = (U, x, nu, ni, d, users, gen, NULL, n_pool, B, x, x, NULL, pop, n_slots, lo, hi, T, margin, wtab, 1)
        tail = (pos, x, trials, coef, pp, pn, NULL, NULL, NULL, NULL, NULL)
        if dev:
            return lib.pda_warp_sample_f32_dev(*head, step_dev, step_next, *tail)
        return lib.pda_warp_sample_f32(*head, 1, *tail)

    for dev in (False, True):
        for kw in (dict(U=NULL), dict(users=NULL), dict(wtab=NULL), dict(trials=NULL), dict(coef=NULL), dict(pos=NULL), dict(n_pool=0), dict(B=0),
                   dict(B=(1 << 22) + 1), dict(nu=0), dict(ni=0), dict(T=0), dict(T=257), dict(margin=math.nan), dict(lo=5, hi=5), dict(lo=-1),
                   dict(hi=11), dict(pop=x, n_slots=0), dict(pp=x), dict(pp=x, pn=x), dict(pn=x, pop=x, n_slots=2)):
            assert sample(dev, **kw) == ERR_ARG, (dev, kw)
        assert sample(dev, d=48) == ERR_UNSUPPORTED
    assert sample(True, step_dev=NULL) == ERR_ARG and sample(True, step_dev=x, step_next=x) == ERR_ARG

    def step(adam=False, U=x, coef=x, gU=x, tagI=x, B=8, nu=10, ni=10, d=64, reg_div=8.0, tag=1, flags=0, margin=1.0, mU=x, cache=0):
        if adam:
            return lib.pda_warp_adam_step_f32(U, mU, x, gU, x, nu, x, x, x, x, tagI, ni, x, x, x, coef, margin, B, d, 0.01, reg_div, tag, 1e-3, 0.9,
                                              0.999, 1e-8, flags, cache, NULL, NULL)
        return lib.pda_warp_step_f32(U, x, nu, ni, x, x, x, coef, margin, B, d, 0.01, reg_div, gU, x, x, tagI, tag, flags, NULL, NULL)

    for adam in (False, True):
        for kw in (dict(U=NULL), dict(coef=NULL), dict(gU=NULL), dict(tagI=NULL), dict(B=0), dict(nu=0), dict(ni=0), dict(reg_div=0.0), dict(tag=0),
                   dict(flags=1 << 20), dict(margin=math.nan)):
            assert step(adam, **kw) == ERR_ARG, (adam, kw)
        assert step(adam, d=48) == ERR_UNSUPPORTED
    assert step(True, mU=NULL) == ERR_ARG and step(True, cache=99) == ERR_ARG


# ---- what the GPU suite leans on -------------------------------------------------------------------------------------------------------------------
def exact_scores(d, T, B, users):
    U, I = dr.exact_tables(d)
    ref = wr.sample(SEED, 1, B, T, 1.0, wr.weight_table(dr.NI, T, "harmonic").astype(np.float32), U, I, INDPTR, INDICES, user_pool=POOL,
                    n_pool=dr.NU, users=users, neg_range=(0, dr.NI))
    return ref


def given_users(B):
    """The users of the exact-data batches (those of tests/test_gpu_dns.py): a lone ordinary row; else FULL_USER, EMPTY_USER, and draws with
    replacement."""
    if B == 1:
        return np.array([7], dtype=np.int32)
    u = np.random.default_rng(B).integers(0, dr.NU, B).astype(np.int32)
    u[0], u[1], u[B - 1] = dr.FULL_USER, dr.EMPTY_USER, dr.FULL_USER
    return u


@pytest.mark.parametrize("d", [32, 64, 128, 256])
@pytest.mark.parametrize("T", [7, 64, 256])
def test_the_chosen_margin_spreads_the_rows_over_the_rounds(d, T):
    """The exact-table sweep of the GPU suite at B = 300: the margin chosen from the float64 scores is a multiple of 1/8, leaves at least 20 %
    of the rows on each side of the first round (1 <= N <= 4 against N > 4 or N == 0) and at least one row without a violator."""
    ref = exact_scores(d, T, 300, given_users(300))
    s, sp = ref["score"], ref["pos_score"]
    assert (s == s.astype(np.float32)).all() and (np.abs(s) < 256).all() and (s * 64 == np.round(s * 64)).all()     # exact in fp32, in any order
    m = wr.spread_margin(sp, s)
    assert m * 8 == round(m * 8) and abs(m) < 256
    N = wr.first_violator(sp, s, m)
    early = ((N >= 1) & (N <= 4)).mean()
    print("d=%d T=%d: margin %.3f, %.3f of the rows close in round 0, %d have no violator, largest N %d" % (d, T, m, early, (N == 0).sum(), N.max()))
    assert early >= 0.2 and 1 - early >= 0.2 and (N == 0).sum() >= 1 and N.max() > 4
    big, small = wr.first_violator(sp, s, 1024.0), wr.first_violator(sp, s, -1024.0)
    assert (big == 1).all() and (small == 0).all()                        # the two ends of the sweep


@pytest.mark.parametrize("d", [64, 256])
def test_the_bound_leaves_few_rows_undecided_on_gaussian_tables(d):
    """The Gaussian case of the GPU suite (T = 64, B = 300, margin 1): at most 1 % of the rows hold an undecided candidate before their first
    sure violator."""
    U, I = dr.gaussian_tables(d)
    T, B, margin = 64, 300, 1.0
    ref = wr.sample(SEED, 1, B, T, margin, wr.weight_table(dr.NI, T, "harmonic").astype(np.float32), U, I, INDPTR, INDICES, user_pool=POOL,
                    n_pool=dr.NU, neg_range=(0, dr.NI))
    ok, blurred = wr.admitted(ref, margin)
    print("d=%d: %d of %d rows blurred; N: %d rows without a violator, largest %d" % (d, blurred.sum(), B, (ref["trials"] == 0).sum(), ref["trials"].max()))
    assert blurred.mean() <= 0.01
    assert ok[np.arange(B), ref["trials"]].all() and (ok.sum(1) == 1)[~blurred].all()
    assert (ref["trials"] > 4).mean() > 0.1                               # rows on both sides of the first round


def test_few_step_triplets_sit_on_the_kink():
    """The Gaussian step case of the GPU suite: at most 1 % of the triplets have h_t within the bound of 0."""
    for d, B in ((64, 256), (256, 300)):
        rng = np.random.default_rng(d)
        U, I = (rng.standard_normal((dr.NU, d)) * 0.3).astype(np.float32), (rng.standard_normal((dr.NI, d)) * 0.3).astype(np.float32)
        users, pos, neg = (rng.integers(0, n, B) for n in (dr.NU, dr.NI, dr.NI))
        _, _, _, h = wr.step_grads(U, I, users, pos, neg, np.ones(B), margin=1.0, regs=0.0, reg_div=B)
        assert (np.abs(h) <= wr.h_bound(U, I, users, pos, neg)).mean() <= 0.01
