"""CPU suite for DICE (`--train dice`, include/pda_hip_dice.h): the flags, the refusals, the binding against the header, the entry points'
argument checks (all before any HIP call), PNSM's boundaries in the restatement of tests/dice_ref.py by enumeration, the share of rows the
rejection cap may take in the sampler tests' inputs, the schedule, and the checkpoint."""
import argparse
import ctypes as C
import io

import numpy as np
import pytest
import torch

from dice_ref import PARITY_CASES, PARITY_SEED, PARITY_STEP, dice_grads, parity_data, pnsm, pnsm_bounds, pnsm_sets, pop_order
from sampler_ref import REJECT_CAP
from test_abi import declared_in

ERR_ARG, ERR_UNSUPPORTED = -1, -2


def make_args(**over):
    from pda_amd.parse import parse_args
    a = parse_args(["--train", "dice", "--embed_size", "32", "--batch_size", "16"])
    for k, v in over.items():
        setattr(a, k, v)
    return a


CONFIG = {"n_users": 9, "n_items": 12}


# ---- flags and refusals --------------------------------------------------------------------------------------------------------------------
def test_flags_parse_and_the_reference_flags_stay():
    from pda_amd import parse
    a = parse.parse_args([])
    assert (a.dice_int_weight, a.dice_con_weight, a.dice_dis_pen, a.dice_dis_loss) == (0.1, 0.1, 0.01, "l1")
    assert (a.dice_margin, a.dice_margin_decay, a.dice_loss_decay) == (40.0, 0.9, 0.9)
    b = parse.parse_args("--train dice --test dice --dice_int_weight 0.2 --dice_con_weight 0.3 --dice_dis_pen 0.5 --dice_dis_loss l2 "
                         "--dice_margin 7 --dice_margin_decay 0.8 --dice_loss_decay 0.7".split())
    assert (b.train, b.test, b.dice_int_weight, b.dice_con_weight, b.dice_dis_pen, b.dice_dis_loss, b.dice_margin, b.dice_margin_decay,
            b.dice_loss_decay) == ("dice", "dice", 0.2, 0.3, 0.5, "l2", 7.0, 0.8, 0.7)
    ext = [f[0] for f in parse._EXTENSION_FLAGS]
    assert ext[-7:] == ["dice_int_weight", "dice_con_weight", "dice_dis_pen", "dice_dis_loss", "dice_margin", "dice_margin_decay", "dice_loss_decay"]
    assert not set(ext) & set(parse.reference_flag_names()) and parse.reference_flag_names()[:5] == ["data_path", "dataset", "source", "train", "test"]


@pytest.mark.parametrize("over, flag", [({"deterministic": 1}, "--deterministic"), ({"table_dtype": "bf16"}, "--table_dtype"),
                                        ({"optimizer": "sgd"}, "--optimizer"), ({"optimizer": "lazy_adam"}, "--optimizer"),
                                        ({"adam_sweep": "replay"}, "--adam_sweep"), ({"gpus": 2}, "--gpus"),
                                        ({"dice_dis_loss": "dcor"}, "--dice_dis_loss")])
def test_refused_options_name_their_flag(over, flag):
    from pda_amd.model_api import DICE
    with pytest.raises(NotImplementedError, match=flag):
        DICE(make_args(**over), CONFIG, device="cpu")


@pytest.mark.parametrize("d", [16, 48, 256])
def test_an_embed_size_without_a_kernel_is_a_value_error(d):
    from pda_amd.model_api import DICE
    with pytest.raises(ValueError, match="embed_size"):
        DICE(make_args(embed_size=d), CONFIG, device="cpu")


def test_the_trainer_refuses_a_test_mode_dice_does_not_have(monkeypatch, tmp_path):
    from pda_amd import train_new_api as t
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(test="s_condition")))
    with pytest.raises(NotImplementedError, match="--train dice goes with --test normal"):
        t.main([])
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(test="normal", optimizer="sgd")))
    with pytest.raises(NotImplementedError, match="--optimizer"):
        t.main([])


def test_tables_are_two_xavier_halves_side_by_side():
    from pda_amd.model_api import DICE
    m = DICE(make_args(), CONFIG, device="cpu")
    U, I = m.score_tables()
    assert U.shape == (9, 64) and I.shape == (12, 64) and U.is_contiguous() and I.is_contiguous()
    for t, n in ((U, 9), (I, 12)):
        lim = (6.0 / (n + 32)) ** 0.5                       # the bound of a [n, 32] table, not of a [n, 64] one
        assert float(t.abs().max()) <= lim and float(t.abs().max()) > 0.9 * lim
        assert not torch.equal(t[:, :32], t[:, 32:])


# ---- the binding and the argument checks ---------------------------------------------------------------------------------------------------
def test_binding_equals_the_header():
    from pda_amd import _lib
    names = ["pda_dice_adam_step_f32", "pda_dice_dis_f32", "pda_dice_rows_ws_words", "pda_dice_sample", "pda_dice_sample_dev", "pda_dice_step_f32"]
    assert declared_in("pda_hip_dice.h") == sorted(_lib.DICE_SIGNATURES) == names
    for d in (_lib.SIGNATURES, _lib.TEMP_POP_SIGNATURES, _lib.PC_SIGNATURES, _lib.DET_SIGNATURES, _lib.DEEP_SIGNATURES, _lib.XQUAD_SIGNATURES):
        assert not set(names) & set(d)
    lib = _lib.load()
    for n in names:
        assert getattr(lib, n).argtypes == _lib.DICE_SIGNATURES[n][1]
    assert lib.pda_dice_rows_ws_words(2048) == 4 + 3 * 2048 and lib.pda_dice_rows_ws_words(0) == 0


def test_entry_points_check_arguments_without_gpu():
    from pda_amd import _lib
    lib = _lib.load()
    keep = C.create_string_buffer(4096)
    b, null = C.c_void_p(C.addressof(keep)), C.c_void_p(None)

    def step(U=b, users=b, mask=b, B=8, d=32, reg_div=8.0, tag=1, ws=b, nu=9, ni=12):
        return lib.pda_dice_step_f32(U, b, nu, ni, users, b, b, mask, B, d, 0.1, 0.1, 1e-3, reg_div, b, b, b, b, tag, ws, null, null)

    assert step(U=null) == ERR_ARG and step(users=null) == ERR_ARG and step(mask=null) == ERR_ARG and step(ws=null) == ERR_ARG
    assert step(B=0) == ERR_ARG and step(reg_div=0.0) == ERR_ARG and step(tag=0) == ERR_ARG and step(nu=0) == ERR_ARG and step(ni=0) == ERR_ARG
    assert step(d=16) == ERR_UNSUPPORTED and step(d=256) == ERR_UNSUPPORTED and step(d=48) == ERR_UNSUPPORTED

    def dis(U=b, B=8, d=32, kind=0, ws=b, nu=9):
        return lib.pda_dice_dis_f32(U, b, nu, 12, B, d, kind, 0.01, b, b, ws, null, null)

    assert dis(nu=0) == ERR_ARG and dis(U=null) == ERR_ARG and dis(ws=null) == ERR_ARG and dis(B=0) == ERR_ARG and dis(kind=2) == ERR_ARG and dis(kind=-1) == ERR_ARG
    assert dis(d=20) == ERR_UNSUPPORTED

    def adam(m=b, kind=0, policy=0, d=64):
        return lib.pda_dice_adam_step_f32(b, m, b, b, b, 9, b, b, b, b, b, 12, b, b, b, b, 8, d, 0.1, 0.1, kind, 0.01, 1e-3, 8.0, 1, 1e-3, 0.9, 0.999, 1e-8,
                                          policy, b, null, null)

    assert adam(m=null) == ERR_ARG and adam(kind=3) == ERR_ARG and adam(policy=5) == ERR_ARG and adam(d=8) == ERR_UNSUPPORTED

    def sample(users=b, order=b, B=8, n_items=12, n_pool=9, gen=1, margin=3.0):
        return lib.pda_dice_sample(users, gen, b, n_pool, B, b, b, n_items, order, b, b, margin, 1, 1, b, b, b, null)

    assert sample(users=null) == ERR_ARG and sample(order=null) == ERR_ARG and sample(B=0) == ERR_ARG and sample(n_items=0) == ERR_ARG
    assert sample(n_pool=0) == ERR_ARG and sample(margin=-1.0) == ERR_ARG and sample(margin=float("nan")) == ERR_ARG

    def sample_dev(margin=b, step=b, nxt=null):
        return lib.pda_dice_sample_dev(b, 1, b, 9, 8, b, b, 12, b, b, b, margin, 1, step, nxt, b, b, b, null)

    assert sample_dev(margin=null) == ERR_ARG and sample_dev(step=null) == ERR_ARG and sample_dev(nxt=b) == ERR_ARG
    del keep


def test_ops_refuses_bad_batches_before_the_library():
    from pda_amd import ops
    U, I = torch.zeros(9, 64), torch.zeros(12, 64)
    with pytest.raises(ValueError, match="HBM"):
        ops._dice_check(U, I, *(torch.zeros(4, dtype=torch.int32),) * 3, torch.zeros(4, dtype=torch.uint8), False)


# ---- PNSM: the boundaries, by enumeration --------------------------------------------------------------------------------------------------
POP12 = np.array([5, 1, 5, 9, 1, 0, 5, 12, 9, 3, 1, 12], dtype=np.int32)     # ties at 1, 5, 9 and at the top


@pytest.mark.parametrize("margin", [0.0, 0.5, 1.0, 3.0, 4.0, 6.5, 11.0, 12.0, 1e9])
def test_boundaries_equal_the_enumerated_sets(margin):
    order, sorted_pop = pop_order(POP12)
    assert list(sorted_pop) == sorted(POP12) and all((POP12[a], a) < (POP12[b], b) for a, b in zip(order[:-1], order[1:]))
    for p in range(12):
        H, L = pnsm_sets(POP12, p, margin)
        hi_at, lo_end = pnsm_bounds(sorted_pop, POP12[p], margin)
        assert sorted(order[hi_at:]) == list(H) and sorted(order[:lo_end]) == list(L), (p, margin)
        if margin == 0.0:       # ties belong to neither side
            assert len(H) + len(L) + int((POP12 == POP12[p]).sum()) == 12
        if margin >= 12.0:
            assert len(H) == 0 and len(L) == 0
    if margin == 0.0:
        for top in (7, 11):     # the most popular items: nothing above them; the least popular one: nothing below
            assert len(pnsm_sets(POP12, top, margin)[0]) == 0 and len(pnsm_sets(POP12, top, margin)[1]) == 10
        assert len(pnsm_sets(POP12, 5, margin)[1]) == 0 and len(pnsm_sets(POP12, 5, margin)[0]) == 11


def catalogue12():
    """Nine users over the 12 items of POP12: indptr / indices whose item counts ARE POP12."""
    rows = [[] for _ in range(12)]
    for item, c in enumerate(POP12):
        for k in range(c):
            rows[(item + k) % 12].append(item)
    rows = [sorted(r) for r in rows]
    indptr = np.zeros(13, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows])
    assert (np.bincount(indices, minlength=12) == POP12).all()
    return indptr, indices


@pytest.mark.parametrize("margin", [0.0, 3.0, 6.5, 1e9])
def test_restated_sampler_draws_from_the_enumerated_side(margin):
    indptr, indices = catalogue12()
    seen = set()
    for step in range(1, 9):
        s = pnsm(11, step, 12, indptr, indices, POP12, margin, n_pool=12)
        assert sorted(s["users"]) == list(range(12))                  # B == pool: a permutation
        for r in range(12):
            u, p, n, m = int(s["users"][r]), int(s["pos"][r]), int(s["neg"][r]), int(s["mask"][r])
            row = indices[indptr[u]:indptr[u + 1]]
            assert p in row
            H, L = pnsm_sets(POP12, p, margin)
            if s["rejections"][r] < REJECT_CAP:
                assert n not in row
            if len(H) == 0 and len(L) == 0:
                assert s["whole"][r] and m == int(POP12[n] > POP12[p])
                seen.add("whole")
            elif m:
                assert len(H) > 0 and (n in H or s["rejections"][r] == REJECT_CAP) and s["from_h"][r]
                seen.add("H" if len(L) else "H only")
            else:
                assert len(L) > 0 and (n in L or s["rejections"][r] == REJECT_CAP)
                seen.add("L" if len(H) else "L only")
    # every kind of positive that can be drawn (an item somebody owns) was drawn, and both sides where both exist
    want = set()
    for p in np.nonzero(POP12 > 0)[0]:
        H, L = pnsm_sets(POP12, p, margin)
        want |= {"H", "L"} if len(H) and len(L) else ({"H only"} if len(H) else ({"L only"} if len(L) else {"whole"}))
    assert seen == want, (seen, want)
    assert want == {"whole"} if margin == 1e9 else want >= {"L only"}
    assert margin != 0.0 or want >= {"H", "L"}


def test_the_cap_takes_at_most_one_per_cent_of_the_parity_inputs():
    """tests/test_gpu_dice.py compares the kernel with pnsm() on these inputs and checks PNSM's invariants on the rows that did not reach the
    rejection cap: those are at least 99 % of every case, and the case that is meant to reach the cap does."""
    indptr, indices, pop = parity_data()
    capped = {}
    for B, M in PARITY_CASES:
        s = pnsm(PARITY_SEED, PARITY_STEP, B, indptr, indices, pop, M, n_pool=len(indptr) - 1)
        cap = s["rejections"] >= REJECT_CAP
        assert cap.mean() <= 0.01, (B, M, cap.mean())
        assert (s["users"][cap] == 0).all()                            # only the user who owns the popular side
        capped[(B, M)] = int(cap.sum())
    assert capped[(2048, 0.0)] > 0 and capped[(2048, 3.0)] > 0 and capped[(2048, 1e9)] == 0, capped


def test_the_host_twin_draws_from_the_same_sides():
    import random
    from pda_amd.sampler import HostDiceSampler
    indptr, indices = catalogue12()
    data = argparse.Namespace(n_items=12, n_users=12, batch_size=12, n_train=len(indices),
                              train_user_list={u: [int(x) for x in indices[indptr[u]:indptr[u + 1]]] for u in range(12)})
    random.seed(3)
    np.random.seed(3)
    s = HostDiceSampler(data, margin=3.0, margin_decay=0.5)
    assert (s.pop == POP12).all()
    n = 0
    for users, pos, neg, mask in s():
        for u, p, ng, m in zip(users, pos, neg, mask):
            H, L = pnsm_sets(POP12, p, 3.0)
            own = set(data.train_user_list[u])
            side = set(H) if m else (set(L) if len(L) else set(range(12)) - own)
            assert p in own and ng in side and (ng not in own or side <= own)      # (a side the user owns entirely: the cap's last draw)
            n += 1
    assert n == 12 * (len(indices) // 12 + 1)


# ---- the schedule ----------------------------------------------------------------------------------------------------------------------------
def test_the_schedule_multiplies_at_epoch_starts_only():
    from pda_amd.model_api import DICE
    from pda_amd.sampler import HostDiceSampler
    m = DICE(make_args(dice_int_weight=0.1, dice_con_weight=0.2, dice_loss_decay=0.9), CONFIG, device="cpu")
    data = argparse.Namespace(n_items=12, n_users=1, batch_size=1, n_train=1, train_user_list={0: [1]})
    s = HostDiceSampler(data, margin=40.0, margin_decay=0.9)
    m.start_epoch(0, s.start_epoch(0))
    assert (m.w_int, m.w_con, m.margin, s.margin) == (0.1, 0.2, 40.0, 40.0)
    for _ in s():                                                      # running an epoch moves nothing
        pass
    assert (m.w_int, m.w_con, s.margin) == (0.1, 0.2, 40.0)
    m.start_epoch(1, s.start_epoch(1))
    m.start_epoch(2, s.start_epoch(2))
    assert m.w_int == pytest.approx(0.1 * 0.81) and m.w_con == pytest.approx(0.2 * 0.81) and s.margin == pytest.approx(40.0 * 0.81)
    assert m.margin == s.margin


# ---- the checkpoint --------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_and_refusal_of_another_model():
    from pda_amd.model_api import BPRMF, DICE
    a = DICE(make_args(), CONFIG, device="cpu", seed=1)
    st = a._dice_state()
    g = torch.Generator().manual_seed(4)
    for k in ("mU", "vU", "mI", "vI"):
        getattr(st, k).copy_(torch.rand(getattr(st, k).shape, generator=g))
    a._t = 17
    a.start_epoch(1, 36.0)
    buf = io.BytesIO()
    torch.save(a.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf)
    assert sd["format"] == "pda_amd/2" and sd["model"] == "dice" and sd["embed_size"] == 32
    b = DICE(make_args(), CONFIG, device="cpu", seed=2)
    assert not torch.equal(a.weights["user_embedding"], b.weights["user_embedding"])
    b._dice_state().tagU.fill_(18)                                   # the tags of a step the checkpoint has not run yet
    b.load_state_dict(sd)
    assert int(b._dice.tagU.abs().max()) == 0 and int(b._dice.tagI.abs().max()) == 0 and float(b._dice.gU.abs().max()) == 0.0
    with pytest.raises(ValueError, match="format"):
        b.load_state_dict(dict(sd, format="pda_amd/1"))
    for k in ("user_embedding", "item_embedding"):
        assert torch.equal(a.weights[k], b.weights[k])
    for k in ("mU", "vU", "mI", "vI"):
        assert torch.equal(getattr(a._dice, k), getattr(b._dice, k))
    assert (b._t, b.margin, b.w_int, b.w_con) == (17, 36.0, a.w_int, a.w_con) and b.w_int == pytest.approx(0.09)
    # the other way round, and a BPRMF file of the same shape (embed_size 64 = the row width of this DICE model)
    plain_args = make_args(train="normal", embed_size=64)
    plain = BPRMF(plain_args, CONFIG, device="cpu")
    with pytest.raises(ValueError, match="dice model cannot be loaded into BPRMF"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="mf model cannot be loaded into DICE"):
        b.load_state_dict(plain.state_dict())
    with pytest.raises(ValueError, match="embed_size"):
        DICE(make_args(embed_size=64), CONFIG, device="cpu").load_state_dict(sd)


# ---- the loss restatement against a second derivation -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["l1", "l2"])
def test_restated_gradients_match_the_closed_form(kind):
    """dice_grads (autograd) against the closed form the kernel implements, in float64: the coefficients of the three log-sigmoids per half,
    the L2 term, and the discrepancy on the distinct rows with its zero subgradient."""
    rng = np.random.default_rng(3)
    nU, nI, d, B = 7, 9, 4, 16
    U, I = rng.standard_normal((nU, 2 * d)) * 0.4, rng.standard_normal((nI, 2 * d)) * 0.4
    U[2, d:d + 2] = U[2, :2]                                           # int == con in two elements of a row of the batch
    users, pos, neg = rng.integers(0, nU, B), rng.integers(0, nI, B), rng.integers(0, nI, B)
    users[0] = 2
    mask = rng.integers(0, 2, B)
    kw = dict(w_int=0.3, w_con=0.2, dis_pen=0.05, dis_kind=kind, regs=1e-2, reg_div=B)
    terms, gU, gI = dice_grads(U, I, users, pos, neg, mask, **kw)
    sg = lambda x: 1 / (1 + np.exp(-x))                                # noqa: E731
    dl = lambda x: sg(x) * (1 - sg(x)) / (sg(x) + 1e-10)               # noqa: E731  d log(sigmoid(x) + 1e-10) / dx
    eU, eI = np.zeros_like(U), np.zeros_like(I)
    c = kw["regs"] / B
    for u, p, n, m in zip(users, pos, neg, mask):
        xi = U[u, :d] @ I[p, :d] - U[u, :d] @ I[n, :d]
        xc = U[u, d:] @ I[p, d:] - U[u, d:] @ I[n, d:]
        gk = -dl(xi + xc) / B
        gi = gk - m * kw["w_int"] * dl(xi) / B
        gc = gk + kw["w_con"] * (m * dl(-xc) - (1 - m) * dl(xc)) / B
        for half, gx in ((slice(0, d), gi), (slice(d, 2 * d), gc)):
            eU[u, half] += gx * (I[p, half] - I[n, half])
            eI[p, half] += gx * U[u, half]
            eI[n, half] -= gx * U[u, half]
        eU[u] += c * U[u]
        eI[p] += c * I[p]
        eI[n] += c * I[n]
    for X, e, S in ((U, eU, np.unique(users)), (I, eI, np.unique(np.concatenate([pos, neg])))):
        df = X[S, :d] - X[S, d:]
        dd = (np.sign(df) if kind == "l1" else 2 * df) / (len(S) * d)
        e[S, :d] -= kw["dis_pen"] * dd
        e[S, d:] += kw["dis_pen"] * dd
    np.testing.assert_allclose(gU, eU, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(gI, eI, rtol=1e-10, atol=1e-14)
    assert terms[0] == pytest.approx(terms[1] + terms[2], rel=1e-14)
