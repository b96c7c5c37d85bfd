"""CPU suite for the sampled-softmax loss (`--train ssm`, include/pda_hip_ssm.h): the flags, the refusals, the binding against the header, the
entry points' argument checks (all before any HIP call), the checkpoint, the sampler's restatement (column 0, rejection, distribution), the
restatement of tests/ssm_ref.py against the oracle's BPR at N = 1, the mutants the GPU tests must be able to tell from the contract, and the
float32 restatement inside the bounds the GPU suite holds the kernel to."""
import ctypes as C
import functools
import io

import numpy as np
import pytest
import torch

import sampler_ref as sr
from ssm_ref import CASES, MUTANTS, NI, NU, REGS, TOL, adam_steps_reference, parity_case, ssm_grads, ssm_sample, tables, tolerance, tpb
from test_abi import declared_in

ERR_ARG, ERR_UNSUPPORTED = -1, -2
CONFIG = {"n_users": 9, "n_items": 12}


def make_args(**over):
    from pda_amd.parse import parse_args
    a = parse_args(["--train", "ssm", "--embed_size", "32", "--batch_size", "16"])
    for k, v in over.items():
        setattr(a, k, v)
    return a


# ---- flags and refusals --------------------------------------------------------------------------------------------------------------------
def test_flags_parse_and_the_reference_flags_stay():
    from pda_amd import parse
    a = parse.parse_args([])
    assert (a.ssm_negs, a.ssm_tau, a.ssm_norm) == (64, 0.1, 1)
    assert isinstance(a.ssm_negs, int) and isinstance(a.ssm_tau, float) and isinstance(a.ssm_norm, int)
    b = parse.parse_args("--train ssm --test ssm --ssm_negs 8 --ssm_tau 0.5 --ssm_norm 0".split())
    assert (b.train, b.test, b.ssm_negs, b.ssm_tau, b.ssm_norm) == ("ssm", "ssm", 8, 0.5, 0)
    ext = [f[0] for f in parse._EXTENSION_FLAGS]
    assert ext[-12:-9] == ["ssm_negs", "ssm_tau", "ssm_norm"] and ext[-9] == "ips_clip"            # in front of the IPS block
    ref = parse.reference_flag_names()
    assert not set(ext) & set(ref) and len(ref) == 54 and ref[:5] == ["data_path", "dataset", "source", "train", "test"]
    table = {f[0]: f for f in parse._REFERENCE_FLAGS}
    for k in ("train", "test"):                                        # only the help text changed: it names ssm
        assert table[k][1] is None and table[k][2] == "normal" and "ssm" in table[k][3]


REFUSED = [({"deterministic": 1}, "--deterministic"), ({"table_dtype": "bf16"}, "--table_dtype"), ({"optimizer": "sgd"}, "--optimizer"),
           ({"optimizer": "lazy_adam"}, "--optimizer"), ({"optimizer": "sgd_fused"}, "--optimizer"), ({"adam_sweep": "replay"}, "--adam_sweep"),
           ({"adam_sweep": "replay_fast"}, "--adam_sweep"), ({"gpus": 2}, "--gpus"), ({"sampler": "host"}, "--sampler")]
BAD_VALUES = [({"ssm_negs": 0}, "--ssm_negs"), ({"ssm_negs": 257}, "--ssm_negs"), ({"ssm_negs": 2.5}, "--ssm_negs"), ({"ssm_tau": 0.0}, "--ssm_tau"),
              ({"ssm_tau": -0.1}, "--ssm_tau"), ({"ssm_tau": float("nan")}, "--ssm_tau"), ({"ssm_tau": float("inf")}, "--ssm_tau"),
              ({"ssm_norm": 2}, "--ssm_norm"), ({"ssm_norm": -1}, "--ssm_norm")]


@pytest.mark.parametrize("over, flag", REFUSED)
def test_refused_options_name_their_flag(over, flag):
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


def test_the_trainer_and_the_backbone_refuse_what_ssm_does_not_have(monkeypatch):
    from pda_amd import train_new_api as t
    from pda_amd.model_api import check_lightgcn
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(test="s_condition")))
    with pytest.raises(NotImplementedError, match="--train ssm goes with --test normal"):
        t.main([])
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(test="normal", sampler="host")))
    with pytest.raises(NotImplementedError, match="--sampler"):
        t.main([])
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(test="ssm", ssm_negs=300)))
    with pytest.raises(ValueError, match="--ssm_negs"):
        t.main([])
    with pytest.raises(NotImplementedError, match="--model lightgcn --train ssm"):
        check_lightgcn(make_args(model="lightgcn"))


def test_the_device_sampler_refuses_what_the_ssm_mode_does_not_draw():
    """The refusals stand in front of everything the constructor builds: no data set is needed to meet them."""
    from pda_amd.sampler import DeviceSampler
    for kw, what in ((dict(with_pop=True, n_negs=4), "with_pop"), (dict(with_pop=False, temp_slots=3, n_negs=4), "temp_slots"),
                     (dict(with_pop=False, n_negs=0), "n_negs"), (dict(with_pop=False, n_negs=257), "n_negs")):
        with pytest.raises(ValueError, match=what):
            DeviceSampler(None, "cpu", mode="ssm", **kw)
    with pytest.raises(ValueError, match="'ssm'"):
        DeviceSampler(None, "cpu", False, mode="softmax")


# ---- the binding and the argument checks ---------------------------------------------------------------------------------------------------
NAMES = ["pda_ssm_adam_step_f32", "pda_ssm_normalize_rows_f32", "pda_ssm_sample", "pda_ssm_sample_dev", "pda_ssm_step_f32"]


def test_binding_equals_the_header():
    from pda_amd import _lib
    assert declared_in("pda_hip_ssm.h") == sorted(_lib.SSM_SIGNATURES) == NAMES
    for d in (_lib.SIGNATURES, _lib.TEMP_POP_SIGNATURES, _lib.PC_SIGNATURES, _lib.DET_SIGNATURES, _lib.DEEP_SIGNATURES, _lib.XQUAD_SIGNATURES,
              _lib.DICE_SIGNATURES, _lib.IPS_SIGNATURES, _lib.MACR_SIGNATURES, _lib.GCN_SIGNATURES, _lib.EXPOSURE_SIGNATURES):
        assert not set(NAMES) & set(d)
    assert not set(NAMES) & (set(declared_in("pda_hip.h")) | set(declared_in("pda_hip_experimental.h")))
    lib = _lib.load()
    for n in NAMES:
        assert getattr(lib, n).argtypes == _lib.SSM_SIGNATURES[n][1]
    # the number of arguments of every declaration in the header
    import os
    import re
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pda_hip_ssm.h")).read(),
                  flags=re.S)
    for n in NAMES:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert len(params.split(",")) == len(_lib.SSM_SIGNATURES[n][1]), n
    assert _lib.SSM_MAX_NEGS == int(re.search(r"#define PDA_SSM_MAX_NEGS (\d+)", text).group(1)) == 256


def test_entry_points_check_arguments_without_gpu():
    from pda_amd import _lib
    lib = _lib.load()
    keep = C.create_string_buffer(4096)
    b, null = C.c_void_p(C.addressof(keep)), C.c_void_p(None)

    def step(U=b, users=b, negs=b, gU=b, tagI=b, B=8, N=4, d=32, tau=0.1, norm=1, reg_div=8.0, tag=1, flags=0x100, nu=9, ni=12):
        return lib.pda_ssm_step_f32(U, b, nu, ni, users, b, negs, B, N, d, tau, norm, 1e-3, reg_div, gU, b, b, tagI, tag, flags, null, null)

    assert step(U=null) == ERR_ARG and step(users=null) == ERR_ARG and step(negs=null) == ERR_ARG and step(gU=null) == ERR_ARG and step(tagI=null) == ERR_ARG
    assert step(N=0) == ERR_ARG and step(N=257) == ERR_ARG and step(N=-1) == ERR_ARG
    assert step(tau=0.0) == ERR_ARG and step(tau=-1.0) == ERR_ARG and step(tau=float("nan")) == ERR_ARG and step(tau=float("inf")) == ERR_ARG
    assert step(norm=2) == ERR_ARG and step(norm=-1) == ERR_ARG
    assert step(B=0) == ERR_ARG and step(reg_div=0.0) == ERR_ARG and step(reg_div=float("nan")) == ERR_ARG and step(tag=0) == ERR_ARG
    assert step(nu=0) == ERR_ARG and step(ni=0) == ERR_ARG and step(ni=1 << 31) == ERR_ARG and step(flags=0x400) == ERR_ARG and step(flags=2) == ERR_ARG
    assert step(d=16) == ERR_UNSUPPORTED and step(d=48) == ERR_UNSUPPORTED and step(d=512) == ERR_UNSUPPORTED
    assert step(d=48, N=0) == ERR_ARG                                   # (the argument errors come first)

    def adam(m=b, negs=b, policy=0, d=64, flags=0x300, B=8, N=4, tau=0.1, norm=0):
        return lib.pda_ssm_adam_step_f32(b, m, b, b, b, 9, b, b, b, b, b, 12, b, b, negs, B, N, d, tau, norm, 1e-3, 8.0, 1, 1e-3, 0.9, 0.999, 1e-8,
                                         flags, policy, null, null)

    assert adam(m=null) == ERR_ARG and adam(negs=null) == ERR_ARG and adam(policy=5) == ERR_ARG and adam(policy=-1) == ERR_ARG and adam(flags=1) == ERR_ARG
    assert adam(B=-3) == ERR_ARG and adam(N=257) == ERR_ARG and adam(tau=0.0) == ERR_ARG and adam(norm=2) == ERR_ARG and adam(d=8) == ERR_UNSUPPORTED

    def sample(users=b, indptr=b, negs=b, gen=1, n_pool=9, B=8, N=4, lo=0, hi=12):
        return lib.pda_ssm_sample(users, gen, null, n_pool, B, N, indptr, b, lo, hi, 1, 1, b, negs, null)

    assert sample(users=null) == ERR_ARG and sample(indptr=null) == ERR_ARG and sample(negs=null) == ERR_ARG and sample(B=0) == ERR_ARG
    assert sample(N=0) == ERR_ARG and sample(N=257) == ERR_ARG and sample(hi=0) == ERR_ARG and sample(n_pool=0) == ERR_ARG

    def sample_dev(step_dev=b, step_next=null, N=4):
        return lib.pda_ssm_sample_dev(b, 1, null, 9, 8, N, b, b, 0, 12, 1, step_dev, step_next, b, b, null)

    assert sample_dev(step_dev=null) == ERR_ARG and sample_dev(step_next=b) == ERR_ARG and sample_dev(N=0) == ERR_ARG
    assert lib.pda_ssm_normalize_rows_f32(null, 4, 32, b, null) == ERR_ARG and lib.pda_ssm_normalize_rows_f32(b, 4, 32, null, null) == ERR_ARG
    assert lib.pda_ssm_normalize_rows_f32(b, 0, 32, b, null) == ERR_ARG and lib.pda_ssm_normalize_rows_f32(b, 4, 48, b, null) == ERR_UNSUPPORTED
    del keep


def test_ops_refuses_bad_batches_before_the_library():
    from pda_amd import ops
    U, I = torch.zeros(9, 32), torch.zeros(12, 32)
    i4, n4 = torch.zeros(4, dtype=torch.int32), torch.zeros((4, 3), dtype=torch.int32)
    with pytest.raises(ValueError, match="HBM"):
        ops.ssm_step(U, I, i4, i4, n4, U.clone(), I.clone(), torch.zeros(9, dtype=torch.int32), torch.zeros(12, dtype=torch.int32), tau=0.1, norm=1,
                     regs=1e-3, reg_div=4, step=1)
    with pytest.raises(ValueError, match="HBM"):
        ops.ssm_normalize_rows(U)
    with pytest.raises(ValueError, match="tau"):
        ops._ssm_params(0.0, 1)
    with pytest.raises(ValueError, match="norm"):
        ops._ssm_params(0.1, 2)


# ---- the model and its checkpoint ----------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_holds_the_raw_tables_and_a_bprmf_loads_it():
    from pda_amd.model_api import BPRMF, SSMBPRMF
    a = SSMBPRMF(make_args(ssm_negs=8, ssm_tau=0.25, ssm_norm=0), CONFIG, device="cpu", seed=1)
    assert isinstance(a, BPRMF) and [f.name for f in (a.opt, a.loss, a.mf_loss, a.reg_loss, a.batch_ratings)] == ["opt", "loss", "mf_loss", "reg_loss",
                                                                                                                   "batch_ratings"]
    U, I = a.score_tables()                                            # norm == 0: the raw tables themselves
    assert U is a.weights["user_embedding"] and I is a.weights["item_embedding"]
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
    assert set(sd) == set(plain.state_dict()) | {"mU", "vU", "mI", "vI", "ssm_negs", "ssm_tau", "ssm_norm"} and sd["format"] == "pda_amd/2"
    assert (sd["ssm_negs"], sd["ssm_tau"], sd["ssm_norm"], sd["adam_t"], sd["embed_size"]) == (8, 0.25, 0, 17, 32)
    normed = SSMBPRMF(make_args(ssm_norm=1), CONFIG, device="cpu", seed=3)
    for m in (plain, normed):
        assert not torch.equal(a.weights["user_embedding"], m.weights["user_embedding"])
        m.load_state_dict(sd)
        for k in ("user_embedding", "item_embedding"):
            assert torch.equal(a.weights[k], m.weights[k])
        assert m._t == 17
    sd1 = normed.state_dict()                                          # a norm == 1 model stores the raw tables
    assert sd1["ssm_norm"] == 1 and torch.equal(sd1["user_embedding"], a.weights["user_embedding"])
    with pytest.raises(ValueError, match="embed_size"):
        SSMBPRMF(make_args(embed_size=64), CONFIG, device="cpu").load_state_dict(sd)


# ---- the sampler's restatement ---------------------------------------------------------------------------------------------------------------------
def toy_csr(n_users, n_items, seed, max_len):
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.permutation(n_items)[:rng.integers(0, max_len + 1)]) for _ in range(n_users)]
    indptr = np.zeros(n_users + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.concatenate(rows).astype(np.int32), rows


@pytest.mark.parametrize("gen_users", [True, False])
def test_column_zero_is_the_triplet_sampler_and_no_negative_is_a_train_item(gen_users):
    """Rows of at most 12 of 40 items: a draw is rejected with probability <= 0.3, and 4 096 attempts cannot run out."""
    n_users, n_items, B = 50, 40, 32
    indptr, indices, rows = toy_csr(n_users, n_items, 5, 12)
    users = None if gen_users else np.random.default_rng(1).integers(0, n_users, B).astype(np.int32)
    for seed, step, N in ((2020, 1, 1), (2020, 77, 5), (0x9E3779B97F4A7C15, 3, 64)):
        got = ssm_sample(seed, step, B, N, indptr, indices, n_pool=n_users, users=users, neg_range=(0, n_items))
        ref = sr.sample(seed, step, B, indptr, indices, n_pool=n_users, users=users, neg_range=(0, n_items))
        np.testing.assert_array_equal(got["users"], ref["users"])
        np.testing.assert_array_equal(got["pos"], ref["pos"])
        np.testing.assert_array_equal(got["negs"][:, 0], ref["neg"])
        np.testing.assert_array_equal(got["rejections"][:, 0], ref["rejections"])
        assert got["negs"].shape == (B, N) and got["negs"].dtype == np.int32 and got["rejections"].max() < 64
        for r in range(B):
            assert not np.isin(got["negs"][r], rows[int(got["users"][r])]).any()
        if N > 1:
            assert got["rejections"].sum() > 0 and (got["negs"][:, 1:] != got["negs"][:, :1]).any()       # the columns are draws of their own
    lo, hi = 10, 25                                                     # a narrowed range
    got = ssm_sample(7, 2, B, 9, indptr, indices, n_pool=n_users, users=users, neg_range=(lo, hi))
    assert got["negs"].min() >= lo and got["negs"].max() < hi


def test_the_negatives_are_uniform_over_the_items_outside_the_history():
    """Every column of the block: the rank of the negative in the complement of the user's row is uniform, judged like the negative of the
    triplet sampler (tests/test_sampler_distribution.py: the statistic of the restatement at three seeds against protocol replicas, its margin
    and its number of replicas), over the whole block and column by column -- no column is drawn from another distribution."""
    from test_sampler_distribution import chi2_ragged, judge, make_csr, protocol_users
    n, n_items, B, N, S = 40, 30, 20, 5, 300
    csr = make_csr(n, n_items, np.random.default_rng(3).integers(1, 13, n), 4)
    indptr, indices, lens, rank = csr

    def drawn(seed):
        u, k = [], []
        for s in range(1, S + 1):
            out = ssm_sample(seed, s, B, N, indptr, indices, n_pool=n, neg_range=(0, n_items))
            uu = out["users"].astype(np.int64)
            kk = rank[uu[:, None], out["negs"]]
            assert kk.min() >= 0, "a negative from the user's row"
            u.append(uu)
            k.append(kk)
        return np.stack(u), np.stack(k)                                 # [S, B], [S, B, N]

    def protocol(rng):
        u = protocol_users(rng, S, B, n)
        return u, rng.integers(0, (n_items - lens[u])[:, :, None], size=(S, B, N))

    sizes = lambda u: n_items - lens[u.ravel()]                          # noqa: E731
    stats = {"negative's rank in the complement, all columns": lambda u, k: chi2_ragged(k.ravel(), np.repeat(sizes(u), N)),
             "the same per column, summed": lambda u, k: sum(chi2_ragged(k[:, :, j].ravel(), sizes(u)) for j in range(N))}
    judge(stats, drawn, protocol, cells=N * (n_items - 1))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
def test_one_negative_at_tau_one_is_the_bpr_loss_of_the_oracle():
    """N = 1, tau = 1, norm = 0: l = log(1 + exp(s_1 - s_0)) = -log sigmoid(x), x = s_0 - s_1 -- the BPR loss without the 1e-10 inside its log,
    which is all that separates the two at |x| <= 10 (here |x| < 3: 1e-10 / sigmoid(x) < 1e-9 / B per row)."""
    from oracle import pda_oracle as po
    rng = np.random.default_rng(12)
    U, I = tables(rng, 32)
    B = 64
    users, pos, neg = rng.integers(0, NU, B), rng.integers(0, NI, B), rng.integers(0, NI, B)
    fw = po.bpr_forward(U, I, users, pos, neg)
    assert np.abs(fw["ps"] - fw["ns"]).max() <= 10
    want = po.bpr_loss(fw, REGS, B)
    wU, wI = po.dense_grads(NU, NI, users, pos, neg, *po.bpr_grads(fw, REGS, B))
    terms, gU, gI = ssm_grads(U, I, users, pos, neg[:, None], tau=1.0, norm=0, regs=REGS, reg_div=B)
    np.testing.assert_allclose(terms, want, atol=1e-9, rtol=0)
    np.testing.assert_allclose(gU, wU, atol=1e-9, rtol=0)
    np.testing.assert_allclose(gI, wI, atol=1e-9, rtol=0)


def test_restated_gradients_match_the_closed_form_of_the_contract():
    """ssm_grads (autograd) against the formulas of include/pda_hip_ssm.h written out in numpy float64, for both values of norm."""
    rng = np.random.default_rng(3)
    nU, nI, d, B, N, tau = 7, 9, 4, 6, 5, 0.3
    U, I = rng.standard_normal((nU, d)) * 0.4, rng.standard_normal((nI, d)) * 0.4
    users, pos, negs = rng.integers(0, nU, B), rng.integers(0, nI, B), rng.integers(0, nI, (B, N))
    c_reg = 1e-2 / B
    for norm in (0, 1):
        terms, gU, gI = ssm_grads(U, I, users, pos, negs, tau=tau, norm=norm, regs=1e-2, reg_div=B)
        eU, eI, mf, l2 = np.zeros_like(U), np.zeros_like(I), 0.0, 0.0
        for r in range(B):
            u, ids = U[users[r]], np.concatenate([[pos[r]], negs[r]])
            nu = max(np.sqrt((u ** 2).sum()), 1e-12) if norm else 1.0
            uh = u / nu
            ni = np.array([max(np.sqrt((I[i] ** 2).sum()), 1e-12) if norm else 1.0 for i in ids])
            ih = I[ids] / ni[:, None]
            s = ih @ uh / tau
            m = s.max()
            lse = m + np.log(np.exp(s - m).sum())
            mf += (lse - s[0]) / B
            c = np.exp(s - lse) / (tau * B)
            c[0] -= 1 / (tau * B)
            g = (c[:, None] * ih).sum(0)
            eU[users[r]] += ((g - (uh @ g) * uh) / nu if norm else g) + c_reg * u
            l2 += 0.5 * (u ** 2).sum()
            for k, i in enumerate(ids):
                eI[i] += (c[k] * (uh - (uh @ ih[k]) * ih[k]) / ni[k] if norm else c[k] * u) + c_reg * I[i]
                l2 += 0.5 * (I[i] ** 2).sum()
        np.testing.assert_allclose(gU, eU, rtol=1e-10, atol=1e-14)
        np.testing.assert_allclose(gI, eI, rtol=1e-10, atol=1e-14)
        assert terms[1] == pytest.approx(mf, rel=1e-12) and terms[2] == pytest.approx(1e-2 * l2 / B, rel=1e-12)
        assert terms[0] == pytest.approx(terms[1] + terms[2], rel=1e-14)


@functools.lru_cache(maxsize=None)
def reference(case):
    d, N, norm, tau, one_row, grouped, distinct = case
    U, I, b, B = parity_case(*case)
    return ssm_grads(U, I, *b, tau=tau, norm=norm, regs=REGS, reg_div=B)


def worst(a, b):
    return max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max(), np.abs(a[2] - b[2]).max())


def test_the_cases_cover_every_value_of_every_axis_with_every_d():
    assert len(CASES) == 24
    for d in (32, 64, 128, 256):
        mine = [c for c in CASES if c[0] == d]
        assert {c[1] for c in mine} == {1, 2, 7, 64, 256} and {c[2] for c in mine} == {0, 1} and {c[3] for c in mine} == {1.0, 0.1}
        assert {c[4] for c in mine} == {True, False} and {c[5] for c in mine} == {True, False} and {c[6] for c in mine} == {True, False}
    for case in CASES:
        d, N, norm, tau, one_row, grouped, distinct = case
        U, I, (users, pos, negs), B = parity_case(*case)
        assert B == (1 if one_row else tpb(d) + 3) and negs.shape == (B, N) and U.shape == (NU, d) and I.shape == (NI, d)
        if distinct:
            assert len(np.unique(users)) == B                          # the precondition of PDA_UPD_USERS_DISTINCT
        elif B > 20:
            assert len(np.unique(users)) < B
        if grouped:
            assert (np.diff(pos) >= 0).all()
        if B > 1:
            T = tpb(d)                                                 # a run of the hot positive crosses the workgroup boundary of a grouped batch
            assert (pos == NI - 1).sum() >= 5 and (not grouped or pos[T - 1] == pos[T] == NI - 1)
            assert negs.size < 100 or len(np.unique(negs)) < negs.size  # negatives repeat across rows
        if N == 256:
            assert all(len(np.unique(row)) < N for row in negs)        # inside every row


@pytest.mark.parametrize("case", CASES, ids=lambda c: "d%d-N%d-norm%d-tau%g-B%s-%s-%s" % (c[0], c[1], c[2], c[3], "1" if c[4] else "T+3",
                                                                                          "grouped" if c[5] else "any", "distinct" if c[6] else "rep"))
def test_the_float32_restatement_stays_inside_the_gpu_bounds(case):
    """tests/test_gpu_ssm.py holds the kernel to tolerance(tau) on these very inputs: the restatement itself, computed in float32, stays inside
    them with a factor of four to spare, so the bounds ask nothing float32 arithmetic cannot give."""
    d, N, norm, tau, one_row, grouped, distinct = case
    U, I, b, B = parity_case(*case)
    f32 = ssm_grads(U, I, *b, dtype=torch.float32, tau=tau, norm=norm, regs=REGS, reg_div=B)
    tol = tolerance(tau)
    assert tol == (1e-5 if tau == 1.0 else 1e-4)
    w = worst(reference(case), f32)
    print("ssm float32 restatement %s: worst error %.3g (bound %.3g)" % (case, w, tol))
    assert w <= tol / 4, (w, tol)


@pytest.mark.parametrize("norm", [0, 1])
def test_three_adam_steps_in_float32_stay_inside_the_gpu_bound(norm):
    """The three whole steps of tests/test_gpu_ssm.py (ssm_ref.ADAM_STEPS) with the gradients taken in float32: tables and moments stay within a
    quarter of the 1e-5 the GPU test asks, against the float64 steps."""
    r64, _ = adam_steps_reference(norm)
    r32, _ = adam_steps_reference(norm, dtype=torch.float32)
    w = max(np.abs(r64[k] - r32[k]).max() for k in r64)
    print("ssm three steps in float32, norm=%d: worst error %.3g (bound %.3g)" % (norm, w, TOL))
    assert w <= TOL / 4, w


@pytest.mark.parametrize("mutant", MUTANTS)
def test_a_broken_contract_is_outside_the_bounds_on_the_gpu_inputs(mutant):
    """The GPU comparison has power: each restatement with one clause broken -- the positive dropped from the denominator, 1 / tau forgotten in
    the gradient, the projection term of the normalisation skipped, every distinct item regularised once instead of once per occurrence --
    differs from the contract by more than the bound, in a loss term or a gradient element, on EVERY case of the GPU tests the clause takes
    part in (1 / tau: tau != 1; the projection: norm == 1; per occurrence: a batch in which an item occurs twice)."""
    n = 0
    for case in CASES:
        d, N, norm, tau, one_row, grouped, distinct = case
        U, I, b, B = parity_case(*case)
        if mutant == "no_tau_grad" and tau == 1.0:
            continue
        if mutant == "no_proj" and not norm:
            continue
        if mutant == "reg_distinct" and len(np.unique(np.concatenate([b[1], b[2].ravel()]))) == b[1].size + b[2].size:
            continue
        bad = ssm_grads(U, I, *b, tau=tau, norm=norm, regs=REGS, reg_div=B, mutant=mutant)
        w = worst(reference(case), bad)
        print("ssm mutant %s on %s: differs by %.3g (bound %.3g)" % (mutant, case, w, tolerance(tau)))
        assert w > tolerance(tau), (mutant, case, w)
        n += 1
    assert n >= {"drop_pos": 24, "no_tau_grad": 12, "no_proj": 12, "reg_distinct": 20}[mutant]
