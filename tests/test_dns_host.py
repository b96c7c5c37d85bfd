"""CPU suite for dynamic hard-negative sampling (`--neg_sampler dns`, include/pda_hip_dns.h): the flags, the refusals of check_dns, the
binding against the header, the entry points' argument checks (every call carries a violation, so none reaches a launch), the sampler's own
refusals, and the properties of the restatement tests/dns_ref.py that the GPU suite leans on: the pick index is uniform, M = 1 is the
triplet sampler's batch, the order rule, and the conditions on the inputs of the rounded-data GPU test."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dns_ref as dr
import sampler_ref as sr
from test_abi import declared_in
from test_sampler_distribution import SEEDS, chi2, judge

ERR_ARG, ERR_UNSUPPORTED = -1, -2
NULL = C.c_void_p(None)
NAMES = ["pda_dns_sample_f32", "pda_dns_sample_f32_dev"]


def make_args(**over):
    from pda_amd.parse import parse_args
    a = parse_args(["--neg_sampler", "dns", "--embed_size", "32", "--batch_size", "16"])
    for k, v in over.items():
        setattr(a, k, v)
    return a


# ---- flags and refusals --------------------------------------------------------------------------------------------------------------------
def test_flags_parse_and_the_default_changes_nothing():
    from pda_amd import parse
    from pda_amd.model_api import check_dns
    a = parse.parse_args([])
    assert (a.neg_sampler, a.dns_candidates, a.dns_topn) == ("uniform", 16, 1)
    assert isinstance(a.dns_candidates, int) and isinstance(a.dns_topn, int)
    check_dns(a)                                                       # uniform: nothing to refuse, whatever else is set
    for train in ("ssm", "dice", "temp_pop"):
        check_dns(make_args(neg_sampler="uniform", train=train, table_dtype="bf16", gpus=4, sampler="host"))
    b = parse.parse_args("--neg_sampler dns --dns_candidates 32 --dns_topn 4".split())
    assert (b.neg_sampler, b.dns_candidates, b.dns_topn) == ("dns", 32, 4)
    ext = [f[0] for f in parse._EXTENSION_FLAGS]
    assert {"neg_sampler", "dns_candidates", "dns_topn"} <= set(ext) and not set(ext) & set(parse.reference_flag_names())


REFUSED = [({"train": "ssm"}, "--train"), ({"train": "ips"}, "--train"), ({"train": "macr"}, "--train"), ({"train": "dice"}, "--train"),
           ({"train": "temp_pop"}, "--train"), ({"model": "lightgcn"}, "--model"), ({"table_dtype": "bf16"}, "--table_dtype"),
           ({"adam_sweep": "replay"}, "--adam_sweep"), ({"adam_sweep": "replay_fast"}, "--adam_sweep"), ({"adam_exact_lazy": True}, "adam_exact_lazy"),
           ({"sampler": "host"}, "--sampler"), ({"gpus": 2}, "--gpus")]
BAD_VALUES = [({"dns_candidates": 0}, "--dns_candidates"), ({"dns_candidates": 257}, "--dns_candidates"), ({"dns_candidates": 2.5}, "--dns_candidates"),
              ({"dns_topn": 0}, "--dns_topn"), ({"dns_topn": 17}, "--dns_topn"), ({"dns_candidates": 4, "dns_topn": 5}, "--dns_topn"),
              ({"dns_topn": 1.5}, "--dns_topn"), ({"neg_sampler": "hard"}, "--neg_sampler")]


@pytest.mark.parametrize("over, flag", REFUSED)
def test_refused_options_name_their_flag(over, flag):
    from pda_amd.model_api import check_dns
    with pytest.raises(NotImplementedError, match=flag):
        check_dns(make_args(**over))


@pytest.mark.parametrize("over, flag", BAD_VALUES)
def test_bad_values_are_value_errors_that_name_their_flag(over, flag):
    from pda_amd.model_api import check_dns
    with pytest.raises(ValueError, match=flag):
        check_dns(make_args(**over))


@pytest.mark.parametrize("over", [{}, {"train": "s_condition"}, {"optimizer": "sgd"}, {"optimizer": "sgd_fused"}, {"deterministic": 1},
                                  {"adam_sweep": "sweep"}, {"dns_candidates": 256, "dns_topn": 256}, {"dns_candidates": 1}])
def test_what_dns_goes_with_is_let_through(over):
    from pda_amd.model_api import check_dns
    check_dns(make_args(**over))


def test_the_trainer_refuses_before_anything_is_built(monkeypatch):
    from pda_amd import train_new_api as t
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(train="ssm", test="ssm")))
    with pytest.raises(NotImplementedError, match="--neg_sampler dns goes with --train normal"):
        t.main([])
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(dns_candidates=300)))
    with pytest.raises(ValueError, match="--dns_candidates"):
        t.main([])


def test_the_device_sampler_refuses_bad_sizes_before_touching_the_device():
    from pda_amd.sampler import DeviceSampler
    for kw, what in ((dict(n_cands=0), "n_cands"), (dict(n_cands=257), "n_cands"), (dict(n_cands=2.5), "n_cands"), (dict(n_cands=4, topn=0), "topn"),
                     (dict(n_cands=4, topn=5), "topn"), (dict(), "n_cands")):
        with pytest.raises(ValueError, match=what):
            DeviceSampler(None, "cpu", False, mode="dns", **kw)
    with pytest.raises(ValueError, match="'dns'"):
        DeviceSampler(None, "cpu", False, mode="hard")


# ---- the binding and the argument checks ---------------------------------------------------------------------------------------------------
def test_the_library_loads_and_the_binding_equals_the_header():
    from pda_amd import _lib
    lib = _lib.load()
    assert declared_in("pda_hip_dns.h") == sorted(_lib.DNS_SIGNATURES) == NAMES
    for d in (_lib.SIGNATURES, _lib.TEMP_POP_SIGNATURES, _lib.PC_SIGNATURES, _lib.DET_SIGNATURES, _lib.DEEP_SIGNATURES, _lib.XQUAD_SIGNATURES,
              _lib.DICE_SIGNATURES, _lib.IPS_SIGNATURES, _lib.MACR_SIGNATURES, _lib.GCN_SIGNATURES, _lib.EXPOSURE_SIGNATURES, _lib.SSM_SIGNATURES,
              _lib.INBATCH_SIGNATURES):
        assert not set(NAMES) & set(d)
    assert not set(NAMES) & (set(declared_in("pda_hip.h")) | set(declared_in("pda_hip_experimental.h")))
    for n in NAMES:
        assert getattr(lib, n).argtypes == _lib.DNS_SIGNATURES[n][1] and getattr(lib, n).restype is C.c_int
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pda_hip_dns.h")).read(),
                  flags=re.S)
    for n in NAMES:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert len(params.split(",")) == len(_lib.DNS_SIGNATURES[n][1]), n
    from pda_amd import ops
    assert _lib.DNS_MAX_CANDIDATES == ops.DNS_MAX_CANDIDATES == int(re.search(r"#define PDA_DNS_MAX_CANDIDATES (\d+)", text).group(1)) == 256


@pytest.fixture(scope="module")
def entry_points():
    """name -> call(**what differs from a sound call); two distinct non-null addresses stand for every buffer (never dereferenced)."""
    from pda_amd import _lib
    lib = _lib.load()
    keep = C.create_string_buffer(4096)
    b, c = C.c_void_p(C.addressof(keep)), C.c_void_p(C.addressof(keep) + 64)

    def plain(U=b, I=b, nu=9, ni=12, d=32, users=b, gen=1, n_pool=9, B=8, indptr=b, indices=b, pop=NULL, n_slots=0, lo=0, hi=12, M=4, topn=2, head=0,
              pos=b, neg=b, pos_pop=NULL, neg_pop=NULL):
        return lib.pda_dns_sample_f32(U, I, nu, ni, d, users, gen, NULL, n_pool, B, indptr, indices, NULL, pop, n_slots, lo, hi, M, topn, head, 1, 1,
                                      pos, neg, pos_pop, neg_pop, NULL, NULL, NULL, NULL)

    def dev(U=b, I=b, nu=9, ni=12, d=32, users=b, gen=1, n_pool=9, B=8, indptr=b, indices=b, pop=NULL, n_slots=0, lo=0, hi=12, M=4, topn=2, head=0,
            pos=b, neg=b, pos_pop=NULL, neg_pop=NULL, step_dev=b, step_next=c):
        return lib.pda_dns_sample_f32_dev(U, I, nu, ni, d, users, gen, NULL, n_pool, B, indptr, indices, NULL, pop, n_slots, lo, hi, M, topn, head, 1,
                                          step_dev, step_next, pos, neg, pos_pop, neg_pop, NULL, NULL, NULL, NULL)

    yield {"pda_dns_sample_f32": plain, "pda_dns_sample_f32_dev": dev}, b, c
    del keep


@pytest.mark.parametrize("name", NAMES)
def test_every_argument_error_comes_back_before_any_launch(entry_points, name):
    eps, b, c = entry_points
    call = eps[name]
    for arg in ("U", "I", "users", "indptr", "indices", "pos", "neg"):                    # null required pointers
        assert call(**{arg: NULL}) == ERR_ARG, arg
    assert call(gen=1, n_pool=0) == ERR_ARG and call(gen=1, n_pool=-4) == ERR_ARG         # users to be drawn from an empty pool
    assert call(B=0) == ERR_ARG and call(B=-1) == ERR_ARG and call(B=(1 << 22) + 1) == ERR_ARG
    assert call(nu=0) == ERR_ARG and call(ni=0) == ERR_ARG and call(ni=1 << 31, hi=12) == ERR_ARG
    assert call(M=0) == ERR_ARG and call(M=257) == ERR_ARG and call(M=-1) == ERR_ARG
    assert call(topn=0) == ERR_ARG and call(topn=5) == ERR_ARG and call(M=256, topn=257) == ERR_ARG and call(topn=-1) == ERR_ARG
    assert call(lo=5, hi=5) == ERR_ARG and call(lo=6, hi=5) == ERR_ARG and call(lo=-1) == ERR_ARG and call(hi=13) == ERR_ARG
    assert call(head=1) == ERR_ARG and call(head=1, pop=b, n_slots=0) == ERR_ARG and call(head=0, pop=b, n_slots=-2) == ERR_ARG
    assert call(head=2) == ERR_ARG and call(head=-1) == ERR_ARG
    assert call(pop=b, n_slots=3, pos_pop=b) == ERR_ARG and call(pop=b, n_slots=3, neg_pop=b) == ERR_ARG        # one without the other
    assert call(pos_pop=b, neg_pop=b) == ERR_ARG                                                                  # both without pop
    for d in (16, 48, 512, 0):
        assert call(d=d) == ERR_UNSUPPORTED, d
    assert call(d=48, M=0) == ERR_ARG                                                     # (the argument errors come first)
    if name.endswith("_dev"):
        assert call(step_dev=NULL) == ERR_ARG and call(step_dev=NULL, step_next=NULL) == ERR_ARG
        assert call(step_dev=b, step_next=b) == ERR_ARG                                   # step + 1 stored where other workgroups still read the step


def test_ops_refuses_bad_calls_before_the_library():
    import torch
    from pda_amd import ops
    U, I = torch.zeros(9, 32), torch.zeros(12, 32)
    ip, ix = torch.zeros(10, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="HBM"):
        ops.dns_sample(U, I, ip, ix, 4, n_cands=4, seed=1, step=1, neg_range=(0, 12), n_pool=9)
    for kw, what in ((dict(n_cands=0), "n_cands"), (dict(n_cands=257), "n_cands"), (dict(n_cands=4, topn=5), "topn")):
        with pytest.raises(ValueError, match=what):
            ops.check_dns_sizes(kw["n_cands"], kw.get("topn", 1))


# ---- the restatement's own properties ------------------------------------------------------------------------------------------------------------
def test_the_order_rule():
    nan, inf = float("nan"), float("inf")
    s = np.array([[1.0, 3.0, 3.0, -2.0], [nan, 0.0, nan, -inf], [nan, nan, nan, nan], [0.0, -0.0, inf, 0.0]])
    assert dr.order(s).tolist() == [[1, 2, 0, 3], [1, 3, 0, 2], [0, 1, 2, 3], [2, 0, 1, 3]]


@pytest.mark.parametrize("N", [2, 3, 7])
def test_the_pick_index_is_uniform(N):
    """t = bounded(draw(seed, step, r, 3), N) over steps x rows: its frequency and the pair (t of row r, t of row r + 1), against numpy's
    integers(0, N), by the replica rule of tests/test_sampler_distribution.py."""
    S, B = 300, 64

    def sampler_draw(seed):
        return (np.stack([dr.pick_index(seed, s, B, N, 256) for s in range(1, S + 1)]),)

    stats = {"pick index": lambda t: chi2(np.bincount(t.ravel(), minlength=N), t.size / N),
             "pick index of neighbouring rows": lambda t: chi2(np.bincount((t[:, :-1] * N + t[:, 1:]).ravel(), minlength=N * N),
                                                              t[:, 1:].size / (N * N))}
    got, _ = judge(stats, sampler_draw, lambda g: (g.integers(0, N, (S, B)),), N * N)
    assert (sampler_draw(SEEDS[0])[0].max(), sampler_draw(SEEDS[0])[0].min()) == (N - 1, 0)
    assert (dr.pick_index(5, 9, B, 1, 256) == 0).all() and (dr.pick_index(5, 9, B, 9, 4) < 4).all()        # topn = 1; min(topn, M)


@pytest.mark.parametrize("with_pop", [False, True])
def test_one_candidate_is_the_triplet_sampler_s_batch(with_pop):
    indptr, indices, slots = dr.graph()
    U, I = dr.gaussian_tables(32)
    pop = dr.pop_matrix() if with_pop else None
    pool = np.arange(dr.NU, dtype=np.int32)[::-1].copy()
    for step, B in ((1, 37), (2, 600)):
        kw = dict(slots=slots if with_pop else None, user_pool=pool, n_pool=dr.NU, neg_range=(10, 150), pop_matrix=pop)
        ref = sr.sample(2020, step, B, indptr, indices, **kw)
        got = dr.sample(2020, step, B, 1, 1, U, I, indptr, indices, head=dr.HEAD_POP if with_pop else dr.HEAD_RAW, **kw)
        for k in ("users", "pos", "neg") + (("pos_pop", "neg_pop") if with_pop else ()):
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
        assert (got["pick_col"] == 0).all()
        many = dr.sample(2020, step, B, 8, 3, U, I, indptr, indices, head=dr.HEAD_POP if with_pop else dr.HEAD_RAW, **kw)
        np.testing.assert_array_equal(many["cand"][:, 0], ref["neg"])                     # column 0 is the uniform sampler's negative
        np.testing.assert_array_equal(many["users"], ref["users"])


def test_the_rounded_data_leave_the_bound_no_say():
    """The inputs of the GPU suite's rounded-data case (unit Gaussians, d = 64, M = 32): the gaps between neighbouring scores are orders of
    magnitude above the a-priori bound, so in at least 95 % of the rows the picked position admits a single item."""
    indptr, indices, slots = dr.graph()
    U, I = dr.gaussian_tables(64)
    for head in (dr.HEAD_RAW, dr.HEAD_POP):
        ref = dr.sample(2020, 1, 600, 32, 3, U, I, indptr, indices, head=head, slots=slots, user_pool=None, n_pool=dr.NU, neg_range=(0, dr.NI),
                        pop_matrix=dr.pop_matrix())
        assert dr.single_item_share(ref) >= 0.95
        assert np.isfinite(ref["score"]).all()
        top = np.take_along_axis(ref["score"], ref["order"][:, :4], 1)                    # the scores around the picked positions 0 .. 2
        assert np.median(top[:, :-1] - top[:, 1:]) > 100 * np.median(ref["bound"])

