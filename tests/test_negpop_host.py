"""CPU suite for popularity-weighted negative sampling (`--neg_sampler pop`, include/pda_hip_negpop.h): the accuracy of the alias
table ops.NegPopTable builds against the exact distribution it implies, the frequencies of the restatement's draws, the flags and the
refusals of check_negpop, the binding against the header, and a float32 restatement of the logQ step with its three mutants."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import negpop_ref as nr
import sampler_ref as sr
import ssm_ref
from test_abi import declared_in

NAMES = ["pda_negpop_sample_batches_dev", "pda_negpop_sample_triplets", "pda_negpop_sample_triplets_dev", "pda_negpop_ssm_sample",
         "pda_negpop_ssm_sample_dev", "pda_ssm_adam_step_logq_f32", "pda_ssm_step_logq_f32"]


def make_args(**over):
    from pda_amd.parse import parse_args
    a = parse_args(["--neg_sampler", "pop", "--embed_size", "32", "--batch_size", "16"])
    for k, v in over.items():
        setattr(a, k, v)
    return a


def table_for(n, beta, lo=0, extra=0):
    """ops.NegPopTable over [lo, lo + n) of lo + n + extra items with Pareto-skewed counts -> (table, counts of the range)."""
    from pda_amd import ops
    counts = nr.pareto_counts(n)
    idx = np.repeat(np.arange(lo, lo + n), counts).astype(np.int32)
    return ops.NegPopTable(idx, lo + n + extra, beta, (lo, lo + n), "cpu"), counts


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.75, 1.0, 2.0])
@pytest.mark.parametrize("n", [1, 2, 3, 37, 1000, 5000])
def test_the_table_draws_q_within_the_derived_bound(n, beta):
    """|P_i - q_i| <= (k_i + 1) 2^-31, k_i the slots aliased to i: a slot's mass is off 1 / n by less than 2^-32 (bounded), its split by at most
    2^-33 / n (thr rounded to 32 bits); the factor two is the room of the float64 build."""
    t, counts = table_for(n, beta)
    P = nr.implied(t.thr, t.alias)
    assert sum(P) == 1                                                   # exactly: Fractions
    w = [Fraction(float(x)) for x in nr.weights(counts, beta)]           # (the float64 weights as they are, the quotient exact)
    tot = sum(w)
    k = np.bincount(t.alias[t.alias != np.arange(n)].astype(np.int64), minlength=n)
    worst = 0.0
    for i in range(n):
        err, bound = abs(P[i] - w[i] / tot), Fraction(int(k[i]) + 1, 1 << 31)
        worst = max(worst, float(err / bound))
        assert err <= bound, (i, float(err), float(bound))
    print("n=%d beta=%g: worst error / bound = %.3f" % (n, beta, worst))
    assert np.allclose(t.q[:n], np.array([float(x / tot) for x in w]), rtol=1e-14, atol=0)


@pytest.mark.parametrize("n", [1, 2, 3, 37, 1000])
def test_power_zero_is_the_uniform_table(n):
    t, _ = table_for(n, 0.0)
    assert t.all_full() and (t.alias == np.arange(n)).all()
    assert (t.q[:n] == 1.0 / n).all() and np.allclose(t.logq, np.log(1.0 / n))
    assert all(p == Fraction(c, 1 << 32) for p, c in zip(nr.implied(t.thr, t.alias), nr.slot_counts(n)))


def test_the_reference_builder_meets_the_bound_too():
    counts = nr.pareto_counts(1000)
    w = nr.weights(counts, 1.0)
    thr, alias = nr.build(w)
    P, tot = nr.implied(thr, alias), sum(Fraction(float(x)) for x in w)
    k = np.bincount(alias[alias != np.arange(1000)].astype(np.int64), minlength=1000)
    assert all(abs(P[i] - Fraction(float(w[i])) / tot) <= Fraction(int(k[i]) + 1, 1 << 31) for i in range(1000))


def test_q_logq_and_the_range():
    from pda_amd import ops
    t, counts = table_for(37, 0.75, lo=5, extra=4)
    assert t.neg_range == (5, 42) and t.n == 37 and t.table.dtype == torch.int64 and tuple(t.table.shape) == (37,)
    assert t.q.dtype == np.float64 and t.q.shape == (46,) and (t.q[:5] == 0).all() and (t.q[42:] == 0).all() and abs(t.q.sum() - 1) < 1e-12
    assert t.logq.dtype == np.float32 and np.isfinite(t.logq).all()
    assert (t.logq[:5] == np.float32(np.log(t.q[5:42].min()))).all()                     # q = 0: the log of the smallest positive q
    assert np.allclose(t.logq[5:42], np.log(t.q[5:42]), rtol=1e-6)
    words = t.table.numpy().view(np.uint64)
    assert ((words & np.uint64(0xFFFFFFFF)) == t.thr).all() and ((words >> np.uint64(32)) == t.alias).all()
    mx, ent, uni = t.stats()
    assert mx == t.q.max() and 0 < ent < uni == pytest.approx(np.log(37))
    # an item without train pairs stays drawable
    assert (t.q[5:42][counts == 0] > 0).all()
    for kw, what in ((dict(power=-0.1), "power"), (dict(power=4.5), "power"), (dict(power=float("nan")), "power"), (dict(neg_range=(3, 3)), "neg_range"),
                     (dict(neg_range=(0, 50)), "neg_range")):
        a = dict(power=0.75, neg_range=(5, 42))
        a.update(kw)
        with pytest.raises(ValueError, match=what):
            ops.NegPopTable(np.zeros(3, np.int32), 46, a["power"], a["neg_range"], "cpu")
    with pytest.raises(ValueError, match="train item"):
        ops.NegPopTable(np.array([46], np.int32), 46, 1.0, (0, 46), "cpu")


def test_a_table_is_refused_unless_every_alias_is_a_slot():
    from pda_amd import ops
    ok = ops.NegPopTable.from_slots([0, 5, 2 ** 32 - 1], [1, 2, 2], (0, 3), 3, "cpu")
    assert not ok.all_full() and ok.logq is None
    with pytest.raises(ValueError, match="alias"):
        ops.NegPopTable.from_slots([0, 5, 7], [1, 3, 2], (0, 3), 3, "cpu")
    with pytest.raises(ValueError, match="32 bits"):
        ops.NegPopTable.from_slots([0, 2 ** 32, 7], [1, 2, 2], (0, 3), 3, "cpu")
    with pytest.raises(ValueError, match="one word per item"):
        ops.NegPopTable.from_slots([0, 5], [1, 0], (0, 3), 3, "cpu")


# ---- empirical frequencies -------------------------------------------------------------------------------------------------------------------
def test_the_draws_follow_the_table_and_not_the_uniform_distribution():
    """200 000 unconstrained draws over 37 items: the chi-square against P stays below its 1 - 1e-6 quantile (its tail probability above 1e-6),
    the same draws against the uniform distribution exceed it."""
    n, draws = 37, 200000
    t, _ = table_for(n, 0.75)
    items = nr.alias_items(2020, 1, np.arange(draws, dtype=np.int64), 16, t.thr, t.alias)
    obs = np.bincount(items, minlength=n).astype(np.float64)
    P = np.array([float(p) for p in nr.implied(t.thr, t.alias)])
    stat = lambda exp: float((((obs - exp) ** 2) / exp).sum())           # noqa: E731
    against_p, against_uniform = stat(P * draws), stat(np.full(n, draws / n))
    print("chi2(36): %.1f against P (tail %.3g), %.1f against uniform (tail %.3g)"
          % (against_p, nr.chi2_sf(against_p, n - 1), against_uniform, nr.chi2_sf(against_uniform, n - 1)))
    assert nr.chi2_sf(against_p, n - 1) > 1e-6 > nr.chi2_sf(against_uniform, n - 1)
    # the closed form itself at two tabulated points: the 1 - 1e-6 quantile of 36 degrees of freedom is 91.5024, the tail at the mean 0.46865
    assert abs(nr.chi2_sf(91.5024, 36) - 1e-6) < 1e-9 and abs(nr.chi2_sf(36.0, 36) - 0.46865) < 1e-5


# ---- flags and refusals ------------------------------------------------------------------------------------------------------------------------
def test_flags_parse_and_the_defaults_change_nothing():
    from pda_amd import parse
    from pda_amd.model_api import check_dns, check_negpop
    a = parse.parse_args([])
    assert (a.neg_sampler, a.neg_pop_power) == ("uniform", 0.75) and isinstance(a.neg_pop_power, float)
    check_negpop(a)
    for train in ("ssm", "dice", "temp_pop", "ials"):                    # uniform: nothing to refuse, whatever else is set
        check_negpop(make_args(neg_sampler="uniform", train=train, gpus=4, sampler="host", neg_pop_power=99.0))
    check_negpop(make_args(neg_sampler="dns", train="dice", gpus=4))     # (check_dns's business)
    b = parse.parse_args("--neg_sampler pop --neg_pop_power 1.5".split())
    assert (b.neg_sampler, b.neg_pop_power) == ("pop", 1.5)
    check_dns(b), check_negpop(b)
    ext = [f[0] for f in parse._EXTENSION_FLAGS]
    assert {"neg_sampler", "neg_pop_power"} <= set(ext) and not set(ext) & set(parse.reference_flag_names())
    text = [f[3] for f in parse._EXTENSION_FLAGS if f[0] == "ssm_logq"][0]
    assert "--neg_sampler pop" in text and "cancels" in text


REFUSED = [({"train": t}, "--train") for t in ("dice", "ips", "macr", "temp_pop", "pcc", "dau", "ials")] + \
          [({"train": "ssm", "ssm_source": "batch"}, "--ssm_source"), ({"train": "ssm", "ssm_source": "all"}, "--ssm_source"),
           ({"sampler": "host"}, "--sampler"), ({"gpus": 2}, "--gpus")]
BAD_POWER = [-0.01, 4.01, float("nan"), float("inf"), "x"]
THROUGH = [{}, {"train": "s_condition"}, {"train": "ssm"}, {"train": "ssm", "ssm_logq": 0}, {"optimizer": "sgd"}, {"optimizer": "sgd_fused"},
           {"deterministic": 1}, {"deterministic": 1, "train": "s_condition"}, {"model": "lightgcn"}, {"table_dtype": "bf16"},
           {"neg_pop_power": 0.0}, {"neg_pop_power": 4.0}, {"neg_pop_power": 1}]


@pytest.mark.parametrize("over, flag", REFUSED)
def test_refused_options_name_their_flag(over, flag):
    from pda_amd.model_api import check_negpop
    with pytest.raises(NotImplementedError, match=flag):
        check_negpop(make_args(**over))


@pytest.mark.parametrize("beta", BAD_POWER)
def test_a_bad_power_is_a_value_error_that_names_its_flag(beta):
    from pda_amd.model_api import check_negpop
    with pytest.raises(ValueError, match="--neg_pop_power"):
        check_negpop(make_args(neg_pop_power=beta))


@pytest.mark.parametrize("over", THROUGH)
def test_what_the_uniform_sampler_goes_with_is_let_through(over):
    from pda_amd.model_api import check_dns, check_negpop
    a = make_args(**over)
    check_dns(a), check_negpop(a)


def test_check_dns_still_raises_on_an_unknown_sampler():
    from pda_amd.model_api import check_dns
    with pytest.raises(ValueError, match="--neg_sampler"):
        check_dns(make_args(neg_sampler="popular"))
    check_dns(make_args(neg_sampler="pop", train="dice"))               # pop is check_negpop's to judge


def test_the_trainer_refuses_before_anything_is_built(monkeypatch):
    from pda_amd import train_new_api as t
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(train="dice", test="normal")))
    with pytest.raises(NotImplementedError, match="--neg_sampler pop goes with --train normal"):
        t.main([])
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(neg_pop_power=5.0)))
    with pytest.raises(ValueError, match="--neg_pop_power"):
        t.main([])
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(train="ssm", test="ssm", ssm_source="batch")))
    with pytest.raises(NotImplementedError, match="--ssm_source batch"):
        t.main([])


def test_the_device_sampler_takes_a_table_in_two_modes_only():
    from pda_amd import ops
    from pda_amd.sampler import DeviceSampler
    t = ops.NegPopTable.from_slots([1, 1], [1, 1], (0, 2), 2, "cpu")
    for mode, kw in (("dice", {}), ("dns", dict(n_cands=4))):
        with pytest.raises(ValueError, match="neg_table"):
            DeviceSampler(None, "cpu", False, mode=mode, neg_table=t, **kw)
    with pytest.raises(ValueError, match="NegPopTable"):
        DeviceSampler(None, "cpu", False, neg_table=object())
    with pytest.raises(ValueError, match="neg_range"):
        DeviceSampler(None, "cpu", False, neg_table=t, neg_range=(0, 3))


def test_the_ssm_model_corrects_and_records_only_under_the_proposal():
    """wants_neg_logq follows the three flags, and only a sampled run under --neg_sampler pop adds keys to the checkpoint."""
    from pda_amd.model_api import BPRMF, SSMBPRMF
    extra = {"neg_sampler", "neg_pop_power", "ssm_logq"}
    wants, keys = {}, {}
    for name, over in (("uniform", dict(neg_sampler="uniform")), ("pop1", dict(ssm_logq=1)), ("pop0", dict(ssm_logq=0)),
                       ("batch", dict(neg_sampler="uniform", ssm_source="batch"))):
        a = make_args(train="ssm", **over)
        m = SSMBPRMF.__new__(SSMBPRMF)
        m.ssm_source, m.neg_sampler, m.ssm_logq, m.neg_pop_power = a.ssm_source, a.neg_sampler, a.ssm_logq, a.neg_pop_power
        m.ssm_negs, m.ssm_tau, m.ssm_norm, m.ssm_mask_train = 64, 0.1, 1, 1
        wants[name] = m.wants_neg_logq()
        orig = BPRMF.state_dict
        BPRMF.state_dict = lambda self: {}
        try:
            keys[name] = set(m.state_dict())
        finally:
            BPRMF.state_dict = orig
    assert wants == dict(uniform=False, pop1=True, pop0=False, batch=False)
    assert keys["uniform"] == {"ssm_negs", "ssm_tau", "ssm_norm"} and keys["pop1"] == keys["pop0"] == keys["uniform"] | extra
    assert keys["batch"] == keys["uniform"] | {"ssm_source", "ssm_logq", "ssm_mask_train"}


# ---- the binding ---------------------------------------------------------------------------------------------------------------------------------
def test_the_library_loads_and_the_binding_equals_the_header():
    from pda_amd import _lib
    lib = _lib.load()
    assert declared_in("pda_hip_negpop.h") == sorted(_lib.NEGPOP_SIGNATURES) == NAMES
    for d in (_lib.SIGNATURES, _lib.SSM_SIGNATURES, _lib.DNS_SIGNATURES, _lib.INBATCH_SIGNATURES, _lib.DICE_SIGNATURES):
        assert not set(NAMES) & set(d)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pda_hip_negpop.h")).read(),
                  flags=re.S)
    for n in NAMES:
        assert getattr(lib, n).argtypes == _lib.NEGPOP_SIGNATURES[n][1] and getattr(lib, n).restype is C.c_int
        params = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert len(params.split(",")) == len(_lib.NEGPOP_SIGNATURES[n][1]), n


def test_ops_refuses_bad_calls_before_the_library():
    from pda_amd import ops
    t = ops.NegPopTable.from_slots([1, 1, 1], [0, 1, 2], (0, 3), 3, "cpu")
    ip, ix = torch.zeros(10, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="NegPopTable"):
        ops.negpop_sample_triplets(object(), ip, ix, 4, seed=1, step=1, n_pool=9)
    with pytest.raises(ValueError, match="HBM"):
        ops.negpop_sample_triplets(t, ip, ix, 4, seed=1, step=1, n_pool=9)
    with pytest.raises(ValueError, match="negatives per row"):
        ops.negpop_ssm_sample(t, ip, ix, 4, 257, seed=1, step=1, n_pool=9)
    with pytest.raises(ValueError, match="logq"):
        ops._ssm_logq(torch.zeros(5, dtype=torch.float64), torch.zeros(5, 32))


# ---- the logQ step in float32, and what the tolerance tells apart ------------------------------------------------------------------------------
def logq_case(d, B, N, n_items, seed):
    rng = np.random.default_rng(seed)
    U, I = ssm_ref.tables(rng, d, nU=40, nI=n_items)
    users = rng.integers(0, 40, B).astype(np.int32)
    pos = rng.integers(0, n_items, B).astype(np.int32)
    negs = rng.integers(0, n_items, (B, N)).astype(np.int32)
    q = nr.weights(np.floor(rng.pareto(1.2, n_items) * 3.0), 1.0)
    logq = np.log(q / q.sum()).astype(np.float32)
    return U, I, users, pos, negs, logq


LOGQ_CASES = [(32, 1, 1, 20, 0, 1.0), (64, 5, 7, 50, 1, 0.1), (128, 69, 64, 500, 0, 0.1), (256, 5, 64, 200, 1, 1.0)]


@pytest.mark.parametrize("d, B, N, n_items, norm, tau", LOGQ_CASES)
def test_a_float32_restatement_of_the_logq_step_stays_inside_the_tolerance(d, B, N, n_items, norm, tau):
    U, I, users, pos, negs, logq = logq_case(d, B, N, n_items, 1000 * d + N)
    kw = dict(tau=tau, norm=norm, regs=ssm_ref.REGS, reg_div=B)
    t64, gU64, gI64 = nr.logq_grads(U, I, users, pos, negs, logq, **kw)
    t32, gU32, gI32 = nr.logq_grads(U, I, users, pos, negs, logq, dtype=torch.float32, **kw)
    tol_g, tol_l = ssm_ref.tolerance(tau), nr.loss_tolerance(tau, logq)
    eg, el = max(np.abs(gU32 - gU64).max(), np.abs(gI32 - gI64).max()), np.abs(t32 - t64).max()
    print("float32 restatement: gradients %.2e (tolerance %.1e), loss terms %.2e (%.1e)" % (eg, tol_g, el, tol_l))
    assert eg <= tol_g and el <= tol_l


@pytest.mark.parametrize("mutant", nr.MUTANTS)
def test_the_tolerance_tells_the_mutants_apart(mutant):
    d, B, N, n_items, norm, tau = 64, 5, 7, 50, 1, 0.1
    U, I, users, pos, negs, logq = logq_case(d, B, N, n_items, 1000 * d + N)
    kw = dict(tau=tau, norm=norm, regs=ssm_ref.REGS, reg_div=B)
    t64, gU64, gI64 = nr.logq_grads(U, I, users, pos, negs, logq, **kw)
    tm, gUm, gIm = nr.logq_grads(U, I, users, pos, negs, logq, mutant=mutant, **kw)
    assert max(np.abs(gUm - gU64).max(), np.abs(gIm - gI64).max()) > ssm_ref.tolerance(tau)
    assert np.abs(tm - t64).max() > nr.loss_tolerance(tau, logq)


def test_no_table_is_the_uncorrected_loss():
    U, I, users, pos, negs, logq = logq_case(32, 5, 7, 50, 3)
    kw = dict(tau=0.1, norm=1, regs=ssm_ref.REGS, reg_div=5)
    a = nr.logq_grads(U, I, users, pos, negs, None, **kw)
    b = ssm_ref.ssm_grads(U, I, users, pos, negs, **kw)
    c = nr.logq_grads(U, I, users, pos, negs, np.zeros(50, np.float32), **kw)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)


# ---- the restatement of the draw ---------------------------------------------------------------------------------------------------------------
def test_an_all_full_table_is_the_uniform_restatement():
    indptr, indices, slots = nr.toy_graph(40, 50, 5)
    pop = np.random.default_rng(1).random((60, 4)).astype(np.float32)
    thr, alias = np.full(50, 123, np.uint32), np.arange(50, dtype=np.uint32)
    for seed, step in ((2020, 1), (2 ** 63 + 5, 2 ** 32 + 1)):
        a = nr.sample(seed, step, 37, indptr, indices, thr, alias, neg_lo=3, slots=slots, n_pool=40, pop_matrix=pop)
        b = sr.sample(seed, step, 37, indptr, indices, slots=slots, n_pool=40, neg_range=(3, 53), pop_matrix=pop)
        for k in ("users", "pos", "neg", "pos_pop", "neg_pop", "rejections"):
            assert np.array_equal(a[k], b[k]), k
        c = nr.block(seed, step, 37, 7, indptr, indices, thr, alias, neg_lo=3, n_pool=40)
        d = ssm_ref.ssm_sample(seed, step, 37, 7, indptr, indices, n_pool=40, neg_range=(3, 53))
        assert np.array_equal(c["negs"], d["negs"]) and np.array_equal(c["negs"][:, 0], a["neg"])
