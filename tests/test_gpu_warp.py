"""GPU: the WARP loss (`--train warp`, include/pda_hip_warp.h) against the float64 restatement of tests/warp_ref.py -- T = 1 with an infinite margin
is the triplet sampler bit for bit; on tables whose dot products are exact in fp32 every output of the draw IS the restatement's, over the
embedding sizes, trial counts, batch sizes and margins at which the rounds of the kernel take another path; on Gaussian tables the trial count
is one the a-priori bound admits and the other outputs follow it; the edge rows; determinism, the device counter, a replayed graph and dirty
buffers; the step against float64 (exactly where the sums are exact, to the project's fp32 contract elsewhere); three Adam steps; the CLI."""
import functools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import dns_ref as dr
import warp_ref as wr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 2020
INDPTR, INDICES, SLOTS = dr.graph()
POOL = np.arange(dr.NU, dtype=np.int32)[::-1].copy()
TOL = 1e-5                      # the project's fp32 contract on a loss term or gradient element (tests/ips_ref.py, tests/train_ref.py)


def to(dev, *arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def np_(t):
    return None if t is None else t.cpu().numpy()


def given_users(B):
    """The users of the exact-data batches (those of tests/test_gpu_dns.py): a lone ordinary row; else FULL_USER (all candidates equal),
    EMPTY_USER, and draws with replacement."""
    if B == 1:
        return np.array([7], dtype=np.int32)
    u = np.random.default_rng(B).integers(0, dr.NU, B).astype(np.int32)
    u[0], u[1], u[B - 1] = dr.FULL_USER, dr.EMPTY_USER, dr.FULL_USER
    return u


def wtab32(T, kind="harmonic", n=dr.NI):
    return wr.weight_table(n, T, kind).astype(np.float32)


def run(dev, U, I, B, T, margin, *, wtab=None, step=1, users=None, pop=None, slots=None, neg_range=(0, dr.NI), check_ids=True, stat=None):
    """-> (users, pos, neg, coef, trials, pos_pop, neg_pop, cand, cand_score, pos_score), stat int64 [2]."""
    from pda_amd import ops
    wtab = wtab32(T) if wtab is None else wtab
    Ut, It, ip, ix, sl, pt, pm, us, wt = to(dev, U, I, INDPTR, INDICES, slots, POOL, pop, users, wtab)
    stat = torch.zeros(2, dtype=torch.int64, device=dev) if stat is None else stat
    out = ops.warp_sample(Ut, It, ip, ix, B, max_trials=T, margin=margin, wtab=wt, seed=SEED, step=step, neg_range=neg_range, users=us,
                          user_pool=pt, n_pool=dr.NU, train_slots=sl, pop_matrix=pm, want_cands=True, stat=stat, check_ids=check_ids)
    torch.cuda.synchronize()
    return out, stat


def ref(U, I, B, T, margin, *, wtab=None, step=1, users=None, pop=None, slots=None, neg_range=(0, dr.NI)):
    return wr.sample(SEED, step, B, T, margin, wtab32(T) if wtab is None else wtab, U, I, INDPTR, INDICES, slots=slots, user_pool=POOL,
                     n_pool=dr.NU, users=users, neg_range=neg_range, pop_matrix=pop)


def assert_is_the_restatement(got, stat, want, what=""):
    u, p, n, coef, trials, pp, pn, cand, score, ps = (np_(t) for t in got)
    np.testing.assert_array_equal(u, want["users"], err_msg=what)
    np.testing.assert_array_equal(p, want["pos"], err_msg=what)
    np.testing.assert_array_equal(trials, want["trials"], err_msg=what)
    np.testing.assert_array_equal(n, want["neg"], err_msg=what)
    np.testing.assert_array_equal(coef.view(np.int32), want["coef"].view(np.int32), err_msg=what)
    np.testing.assert_array_equal(cand, want["cand_out"], err_msg=what)
    np.testing.assert_array_equal(score.astype(np.float64), want["score_out"], err_msg=what)
    np.testing.assert_array_equal(ps.astype(np.float64), want["pos_score"], err_msg=what)
    np.testing.assert_array_equal(np_(stat), want["stat"], err_msg=what)


# ---- 1. identity ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 37, 600])
@pytest.mark.parametrize("with_pop, gen, neg_range", [(False, 1, (0, dr.NI)), (True, 1, (0, dr.NI)), (True, 0, (10, 150)), (False, 0, (10, 150)),
                                                      (True, 1, (10, 150))])
def test_one_trial_and_an_infinite_margin_is_the_triplet_sampler_bit_for_bit(dev, B, with_pop, gen, neg_range):
    from pda_amd import ops
    U, I = dr.gaussian_tables(64)
    pop, slots = (dr.pop_matrix(), SLOTS) if with_pop else (None, None)
    users = None if gen else given_users(B)
    ip, ix, sl, pt, pm, us = to(dev, INDPTR, INDICES, slots, POOL, pop, users)
    for step in (1, 2):
        want = ops.sample_triplets(ip, ix, B, seed=SEED, step=step, users=None if us is None else us.clone(), user_pool=pt, n_pool=dr.NU,
                                   train_slots=sl, neg_range=neg_range, pop_matrix=pm)
        got, stat = run(dev, U, I, B, 1, math.inf, wtab=np.array([0, 1], dtype=np.float32), step=step, users=users, pop=pop, slots=slots,
                        neg_range=neg_range)
        for k, (g, w) in enumerate(zip((got[0], got[1], got[2], got[5], got[6]), want)):
            assert (g is None) == (w is None), k
            if g is not None:
                assert torch.equal(g.view(torch.int32), w.view(torch.int32)), (k, step)
        assert (got[3] == 1).all() and (got[4] == 1).all() and torch.equal(got[7][:, 0], want[2]) and stat.tolist() == [B, 0]


# ---- 2. exact tables -----------------------------------------------------------------------------------------------------------------------------
EXACT = [(d, T, B) for d in (32, 64, 128, 256) for T in (1, 2, 7, 64, 256) for B in (1, 5, 69, 300)]


@functools.lru_cache(maxsize=None)
def exact_ref(d, T, B):
    U, I = dr.exact_tables(d)
    return ref(U, I, B, T, 1.0, users=given_users(B))


@pytest.mark.parametrize("d, T, B", EXACT)
def test_exact_tables_give_the_restatement_itself(dev, d, T, B):
    """Entries that are multiples of 1/8 in [-1, 1] and margins that are multiples of 1/8: every score, every x_j and every margin - x_j is exact
    in fp32 in any order, so nothing is left to a tolerance.  Four margins: 1; one so large that every row closes at N = 1; one so negative
    that no row closes (every round runs, all T columns are scored); one chosen from the float64 scores so that N spreads over 1 .. T."""
    U, I = dr.exact_tables(d)
    users = given_users(B)
    base = exact_ref(d, T, B)
    s, sp = base["score"], base["pos_score"]
    assert (s == s.astype(np.float32)).all() and (np.abs(s) < 256).all() and (s * 64 == np.round(s * 64)).all()     # exact in fp32, as claimed
    if B > 1:
        full = np.nonzero(users == dr.FULL_USER)[0]
        assert len(full) >= 2 and (base["cand"][full] == dr.FREE_ITEM).all() and (base["pos"][users == dr.EMPTY_USER] == 0).all()
    chosen = wr.spread_margin(sp, s)
    for margin in (1.0, 1024.0, -1024.0, chosen):
        want = dict(base)
        N = wr.first_violator(sp, s, margin)
        want["trials"] = N.astype(np.int32)
        want.update(wr.outputs_for(N, base["cand"], s, wtab32(T)))
        if margin == 1024.0:
            assert (N == 1).all()
        if margin == -1024.0:
            assert (N == 0).all() and (want["cand_out"] == base["cand"]).all()
        if margin == chosen and B == 300 and T >= 7:
            early = ((N >= 1) & (N <= 4)).mean()
            assert early >= 0.2 and 1 - early >= 0.2 and (N == 0).sum() >= 1 and N.max() > 4
        got, stat = run(dev, U, I, B, T, margin, users=users)
        assert_is_the_restatement(got, stat, want, "d=%d T=%d B=%d margin=%g" % (d, T, B, margin))


def test_batches_beyond_the_resident_workgroups_take_more_rows_each(dev):
    """The rows of a workgroup double once four rows each would mean more than 512 workgroups (pda_warp.hip, rows_per_block): B = 2 049 takes 8,
    B = 40 000 the cap of 64.  Equal to the restatement, and row for row to the small geometry (the same users, four rows a workgroup)."""
    d, T = 256, 7
    U, I = dr.exact_tables(d)
    for B in (2049, 40000):
        users = given_users(B)
        want = ref(U, I, B, T, -7.0, users=users)
        assert 0.2 < (want["trials"] == 0).mean() < 0.8
        got, stat = run(dev, U, I, B, T, -7.0, users=users)
        assert_is_the_restatement(got, stat, want, "B=%d" % B)
        small, _ = run(dev, U, I, 300, T, -7.0, users=users[:300].copy())
        for g, s in zip(got, small):
            assert g is None or torch.equal(g[:300].view(torch.int32), s.view(torch.int32))


# ---- 3. Gaussian tables --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 256])
def test_gaussian_tables_give_a_trial_count_the_bound_admits(dev, d):
    """T = 64, B = 300, margin 1 on N(0, 1) tables.  A candidate whose float64 margin - x_j lies within the a-priori bound of 0 is undecided;
    the kernel's N_r is one of the values the bound admits, and the other outputs are those of that N_r.  (tests/test_warp_host.py: no row of
    this batch holds an undecided candidate before its first sure violator; at most 1 % may.)"""
    U, I = dr.gaussian_tables(d)
    pop = dr.pop_matrix()
    T, B, margin = 64, 300, 1.0
    want = ref(U, I, B, T, margin, pop=pop, slots=SLOTS)
    ok, blurred = wr.admitted(want, margin)
    assert blurred.mean() <= 0.01
    got, stat = run(dev, U, I, B, T, margin, pop=pop, slots=SLOTS)
    u, p, n, coef, trials, pp, pn, cand, score, ps = (np_(t) for t in got)
    np.testing.assert_array_equal(u, want["users"])
    np.testing.assert_array_equal(p, want["pos"])
    np.testing.assert_array_equal(pp, want["pos_pop"])
    N = trials.astype(np.int64)
    print("warp d=%d: rows whose N is the restatement's: %.4f; blurred rows %d" % (d, (N == want["trials"]).mean(), blurred.sum()))
    assert ok[np.arange(B), N].all()
    np.testing.assert_array_equal(N[~blurred], want["trials"][~blurred])
    follow = wr.outputs_for(N, want["cand"], want["score"], wtab32(T))
    np.testing.assert_array_equal(n, follow["neg"])
    np.testing.assert_array_equal(coef, follow["coef"])
    np.testing.assert_array_equal(cand, follow["cand_out"])
    np.testing.assert_array_equal(np_(stat), follow["stat"])
    np.testing.assert_array_equal(pn, pop[n.astype(np.int64), want["slot"]])
    kept = cand >= 0
    assert (score[~kept] == 0).all()
    assert (np.abs(score.astype(np.float64) - want["score"])[kept] <= want["e_cand"][kept]).all()
    assert (np.abs(ps.astype(np.float64) - want["pos_score"]) <= want["e_pos"]).all()


# ---- 4. edge rows --------------------------------------------------------------------------------------------------------------------------------
def test_full_and_empty_users(dev):
    """FULL_USER: every candidate is FREE_ITEM, so the row closes at N = 1 or never; EMPTY_USER: positive 0, every item a candidate."""
    U, I = dr.exact_tables(64)
    B, T = 37, 16
    users = given_users(B)
    for margin in (1.0, -2.0):
        want = ref(U, I, B, T, margin, users=users)
        full = users == dr.FULL_USER
        assert set(want["trials"][full]) <= {0, 1} and (want["neg"][full] == dr.FREE_ITEM).all()
        got, stat = run(dev, U, I, B, T, margin, users=users)
        assert_is_the_restatement(got, stat, want)
        assert (np_(got[1])[users == dr.EMPTY_USER] == 0).all()


def test_an_unknown_user_reads_nothing_and_takes_candidate_zero(dev):
    """Memory safety of the library call (ops refuses such ids on the host): a user id outside [0, n_users) is drawn as a user without train
    items, scores nothing, has no violator and takes candidate 0; its neighbours are untouched."""
    U, I = dr.exact_tables(32)
    B, T = 37, 9
    users = given_users(B)
    good, _ = run(dev, U, I, B, T, 1.0, users=users)
    bad = users.copy()
    bad[[2, 30]] = [dr.NU, -1]
    with pytest.raises(ValueError, match="user id"):
        run(dev, U, I, B, T, 1.0, users=bad)
    got, stat = run(dev, U, I, B, T, 1.0, users=bad, check_ids=False)
    keep = np.ones(B, dtype=bool)
    keep[[2, 30]] = False
    for g, w in zip(got[1:], good[1:]):
        if g is not None:
            assert torch.equal(g[torch.from_numpy(keep).to(dev)], w[torch.from_numpy(keep).to(dev)])
    u, p, n, coef, trials, _, _, cand, score, ps = (np_(t) for t in got)
    assert (trials[~keep] == 0).all() and (coef[~keep] == 0).all() and (p[~keep] == 0).all() and (n[~keep] == cand[~keep, 0]).all()
    assert (score[~keep] == 0).all() and (ps[~keep] == 0).all() and (cand[~keep] >= 0).all()
    as_empty = ref(U, I, B, T, 1.0, users=np.where(keep, users, dr.EMPTY_USER).astype(np.int32))     # drawn as a user without train items
    np.testing.assert_array_equal(cand[~keep], as_empty["cand"][~keep])
    assert np_(stat)[1] == (trials == 0).sum()


def test_nan_rows_never_violate(dev):
    """A NaN planted in candidate rows: those candidates are never the violator.  A NaN planted in a user's row (so in its positive's score,
    and in every x_j): no violator at all."""
    U, I = dr.exact_tables(64)
    U, I = U.copy(), I.copy()
    I[np.arange(0, dr.NI, 3)] = np.nan                                    # a third of the catalogue
    B, T = 37, 16
    users = given_users(B)
    nan_user = int(users[5])
    assert nan_user not in (dr.FULL_USER, dr.EMPTY_USER)
    U[nan_user] = np.nan
    want = ref(U, I, B, T, 1.0, users=users)
    s = want["score"]
    assert (np.isnan(s).any(1) & ~np.isnan(s).all(1)).sum() > B // 2 and (want["trials"][users == nan_user] == 0).all()
    rows = np.arange(B)
    closed = want["trials"] > 0
    assert closed.sum() > B // 3 and not np.isnan(s[rows[closed], want["trials"][closed] - 1]).any()
    nan_pos = np.isnan(want["pos_score"])
    assert nan_pos.sum() > 3 and (want["trials"][nan_pos] == 0).all()     # (positives among the NaN items too)
    got, stat = run(dev, U, I, B, T, 1.0, users=users)
    u, p, n, coef, trials, _, _, cand, score, ps = (np_(t) for t in got)
    np.testing.assert_array_equal(trials, want["trials"])
    np.testing.assert_array_equal(n, want["neg"])
    np.testing.assert_array_equal(coef, want["coef"])
    np.testing.assert_array_equal(cand, want["cand_out"])
    np.testing.assert_array_equal(np.isnan(score), np.isnan(want["score_out"]))
    np.testing.assert_array_equal(np.isnan(ps), nan_pos)
    np.testing.assert_array_equal(np_(stat), want["stat"])


# ---- 5. determinism, the device counter, a replayed graph, dirty buffers -------------------------------------------------------------------------------
@pytest.mark.parametrize("d, T", [(32, 256), (256, 7)])
def test_two_calls_are_bit_equal(dev, d, T):
    U, I = dr.gaussian_tables(d)
    pop = dr.pop_matrix()
    (a, sa), (b, sb) = (run(dev, U, I, 600, T, 1.0, pop=pop, slots=SLOTS) for _ in range(2))
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(sa, sb)


def test_stat_adds_onto_its_previous_value(dev):
    U, I = dr.exact_tables(64)
    B, T = 69, 7
    want = ref(U, I, B, T, -3.0, users=given_users(B))["stat"]
    assert want[0] > 0 and want[1] > 0
    stat = torch.tensor([1000, -5], dtype=torch.int64, device=dev)
    for k in (1, 2):
        run(dev, U, I, B, T, -3.0, users=given_users(B), stat=stat)
        assert stat.tolist() == [1000 + k * int(want[0]), -5 + k * int(want[1])]


def test_the_device_counter_and_a_replayed_graph(dev):
    from pda_amd import ops
    U, I = dr.gaussian_tables(64)
    pop = dr.pop_matrix()
    B, T, margin = 37, 8, 1.0
    Ut, It, ip, ix, sl, pt, pm, wt = to(dev, U, I, INDPTR, INDICES, SLOTS, POOL, pop, wtab32(T))
    kw = dict(max_trials=T, margin=margin, wtab=wt, seed=SEED, neg_range=(0, dr.NI), user_pool=pt, n_pool=dr.NU, train_slots=sl, pop_matrix=pm)
    direct = [ops.warp_sample(Ut, It, ip, ix, B, step=s, want_cands=True, **kw) for s in range(1, 7)]

    def buffers(fill=0):
        i32 = lambda *s: torch.full(s, fill, dtype=torch.int32, device=dev)             # noqa: E731
        f32 = lambda *s: torch.full(s, float("nan") if fill else 0.0, dtype=torch.float32, device=dev)      # noqa: E731
        return (i32(B), i32(B), i32(B), f32(B), i32(B), f32(B), f32(B)), (i32(B, T), f32(B, T), f32(B))

    def same(out, cands, want):
        return all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out + cands, want))

    ctr = torch.tensor([1, -1], dtype=torch.int64, device=dev)
    out, cands = buffers()
    for s in (1, 2, 3):
        ops.warp_sample_into(out, Ut, It, ip, ix, step_dev=ctr, parity=(s - 1) & 1, cands=cands, **kw)
        assert same(out, cands, direct[s - 1]), s
        assert ctr[s & 1].item() == s + 1
    out, cands = buffers(0x3F3F3F3F)                                     # garbage ids, NaN floats: the outputs do not depend on them
    ops.warp_sample_into(out, Ut, It, ip, ix, step_dev=ctr[1:], cands=cands, **kw)          # read only: slot 1 holds 4
    assert same(out, cands, direct[3]) and ctr.tolist() == [3, 4]

    # a graph of two calls (an even number: the counter is back in slot 0 behind them), replayed three times: steps 1 .. 6
    ctr.copy_(torch.tensor([1, -1], dtype=torch.int64))
    (oa, ca), (ob, cb) = buffers(), buffers(-1)
    stat = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ops.warp_sample_into(oa, Ut, It, ip, ix, step_dev=ctr, parity=0, cands=ca, stat=stat, **kw)
            ops.warp_sample_into(ob, Ut, It, ip, ix, step_dev=ctr, parity=1, cands=cb, stat=stat, **kw)
    torch.cuda.synchronize()
    assert ctr.tolist() == [1, -1] and stat.tolist() == [0, 0]           # capturing runs nothing
    total = 0
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert same(oa, ca, direct[2 * k]) and same(ob, cb, direct[2 * k + 1]), k
        assert ctr[0].item() == 2 * k + 3
        total += int(direct[2 * k][4].sum()) + int(direct[2 * k + 1][4].sum())
        assert stat[0].item() == total


@pytest.mark.parametrize("fill", [0xFF, 0x3F])
def test_the_outputs_do_not_depend_on_what_the_buffers_held(dev, fill):
    """Output buffers whose every byte is 0xFF (NaN as fp32, -1 as int32) or 0x3F (0.747 as fp32, a large positive id), the fills of
    tests/dirty_buffers.py, handed to the call that writes into given buffers: the outputs are those of ops.warp_sample, which hands the library
    a zeroed block, and a guard element behind every buffer keeps its fill."""
    from pda_amd import ops
    U, I = dr.gaussian_tables(128)
    pop = dr.pop_matrix()
    Ut, It, ip, ix, sl, pt, pm = to(dev, U, I, INDPTR, INDICES, SLOTS, POOL, pop)

    def filled(dtype, *shape):
        """-> (the buffer, a view of it and one guard element behind it)."""
        n = int(np.prod(shape))
        raw = torch.full(((n + 1) * 4,), fill, dtype=torch.uint8, device=dev).view(dtype)
        return raw[:n].view(*shape), raw

    for B, T, margin in ((69, 7, 1.0), (300, 64, -20.0), (5, 256, 1e6)):
        wt, = to(dev, wtab32(T))
        kw = dict(max_trials=T, margin=margin, wtab=wt, seed=SEED, neg_range=(0, dr.NI), user_pool=pt, n_pool=dr.NU, train_slots=sl, pop_matrix=pm)
        plain = ops.warp_sample(Ut, It, ip, ix, B, step=5, want_cands=True, **kw)
        i32, f32 = torch.int32, torch.float32
        bufs = [filled(dt, *shape) for dt, shape in ((i32, (B,)), (i32, (B,)), (i32, (B,)), (f32, (B,)), (i32, (B,)), (f32, (B,)), (f32, (B,)),
                                                      (i32, (B, T)), (f32, (B, T)), (f32, (B,)))]
        out, cands = tuple(b for b, _ in bufs[:7]), tuple(b for b, _ in bufs[7:])
        ops.warp_sample_into(out, Ut, It, ip, ix, step_dev=torch.tensor([5], dtype=torch.int64, device=dev), cands=cands, **kw)
        torch.cuda.synchronize()
        for (got, raw), want in zip(bufs, plain):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (B, T, margin)
            assert raw.view(torch.uint8)[-4:].tolist() == [fill] * 4          # nothing written behind the buffer


# ---- 6. the step ---------------------------------------------------------------------------------------------------------------------------------
class State:
    """What ops.warp_step / ops.warp_adam_step write besides the tables."""

    def __init__(self, Ut, It):
        from pda_amd import ops
        z = torch.zeros_like
        self.mU, self.vU, self.gU, self.mI, self.vI, self.gI = z(Ut), z(Ut), z(Ut), z(It), z(It), z(It)
        self.tagU, self.tagI = ops.adam_row_tags(Ut.shape[0], It.shape[0], Ut.device)

    def adam(self, Ut, It):
        return Ut, self.mU, self.vU, self.gU, self.tagU, It, self.mI, self.vI, self.gI, self.tagI


def run_step(dev, U, I, b, coef, margin, regs, reg_div, *, tag=3, users_distinct=False, grouped=False, check_ids=True):
    from pda_amd import ops
    Ut, It, ut, pt, nt, ct = to(dev, U, I, *b, coef)
    st = State(Ut, It)
    loss = torch.zeros(3, device=dev)
    ops.warp_step(Ut, It, ut, pt, nt, ct, st.gU, st.gI, st.tagU, st.tagI, margin=margin, regs=regs, reg_div=reg_div, step=tag, grouped=grouped,
                  users_distinct=users_distinct, loss_acc=loss, check_ids=check_ids)
    torch.cuda.synchronize()
    return np_(loss), np_(st.gU), np_(st.gI), np_(st.tagU), np_(st.tagI)


def assert_tags(tagU, tagI, b, tag):
    wu, wi = np.zeros(dr.NU, dtype=np.int32), np.zeros(dr.NI, dtype=np.int32)
    wu[b[0]] = tag
    wi[b[1]] = tag
    wi[b[2]] = tag
    np.testing.assert_array_equal(tagU, wu)
    np.testing.assert_array_equal(tagI, wi)


@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_the_step_on_exact_tables_is_float64_itself(dev, d, distinct):
    """B = 8 (a power of two: 1 / B is exact), coefficients in {0, 1/2, 1, 2}, regs / reg_div = 1/16, a margin that is a multiple of 1/8, table
    entries that are multiples of 1/8: every product and every sum of the loss and of the gradients is exact in fp32 in any order, so loss_acc,
    gU, gI and the tags equal float64 exactly -- with a positive that occurs three times and an inactive triplet of either kind."""
    U, I = dr.exact_tables(d)
    rng = np.random.default_rng(d)
    B = 8
    users = rng.permutation(dr.NU)[:B].astype(np.int32) if distinct else np.array([5, 9, 5, 100, 7, 9, 5, 299], dtype=np.int32)
    pos = np.array([11, 11, 40, 11, 3, 199, 0, 40], dtype=np.int32)
    neg = rng.integers(0, dr.NI, B).astype(np.int32)
    coef = np.array([1, 0.5, 2, 0, 1, 2, 0.5, 0], dtype=np.float32)
    for margin in (0.5, -1.0, 300.0):
        terms, gU, gI, h = wr.step_grads(U, I, users, pos, neg, coef, margin=margin, regs=0.5, reg_div=8.0)
        if margin == 0.5:
            act = (coef > 0) & (h > 0)
            assert 0 < act.sum() < (coef > 0).sum()                       # active, inactive by the hinge, inactive by the coefficient
        loss, hU, hI, tagU, tagI = run_step(dev, U, I, (users, pos, neg), coef, margin, 0.5, 8.0, users_distinct=distinct)
        np.testing.assert_array_equal(loss.astype(np.float64), terms)
        np.testing.assert_array_equal(hU.astype(np.float64), gU)
        np.testing.assert_array_equal(hI.astype(np.float64), gI)
        assert_tags(tagU, tagI, (users, pos, neg), 3)


def gaussian_step_case(d, B, hot, distinct):
    """-> (U, I, (users, pos, neg), coef float32, margin, kept): tables of N(0, 0.3^2), coefficients drawn from the harmonic table of T = 64 (and
    zeros), the triplets whose h_t lies within the bound of 0 left out (kept: the mask; at most 1 % may go)."""
    rng = np.random.default_rng(1000 * d + B + hot)
    U, I = (rng.standard_normal((dr.NU, d)) * 0.3).astype(np.float32), (rng.standard_normal((dr.NI, d)) * 0.3).astype(np.float32)
    users = (rng.permutation(dr.NU)[:B] if distinct else rng.integers(0, dr.NU, B)).astype(np.int32)
    pos, neg = rng.integers(0, dr.NI, B).astype(np.int32), rng.integers(0, dr.NI, B).astype(np.int32)
    if hot:
        pos[rng.permutation(B)[:hot]] = 17                                # one positive `hot` times
    coef = rng.choice(np.concatenate([wtab32(64), np.zeros(16, dtype=np.float32)]), B).astype(np.float32)
    margin = 1.0
    _, _, _, h = wr.step_grads(U, I, users, pos, neg, coef, margin=margin, regs=0.0, reg_div=B)
    kept = np.abs(h) > wr.h_bound(U, I, users, pos, neg)
    assert (~kept).mean() <= 0.01
    return U, I, tuple(a[kept] for a in (users, pos, neg)), coef[kept], margin, kept


@pytest.mark.parametrize("d, B, hot, distinct", [(32, 1, 0, False), (64, 256, 100, False), (64, 256, 100, True), (128, 69, 0, True),
                                                 (256, 300, 0, False), (256, 2048, 0, False)])
def test_the_step_on_gaussian_tables_is_within_the_fp32_contract(dev, d, B, hot, distinct):
    """Loss terms and gradient elements within 1e-5 max(1, max wtab) of float64: 1e-5 is the project's fp32 contract, the factor the largest
    coefficient a gradient is scaled by.  Hot-item batches (one positive 100 times in 256), PDA_UPD_USERS_DISTINCT on and off, coef == 0 rows."""
    U, I, b, coef, margin, kept = gaussian_step_case(d, B, hot, distinct and B <= dr.NU)
    n = len(b[0])
    tol = TOL * max(1.0, float(wtab32(64).max()))
    terms, gU, gI, h = wr.step_grads(U, I, *b, coef, margin=margin, regs=1e-2, reg_div=n)
    if B >= 69:
        assert (coef == 0).sum() > 0 and ((coef > 0) & (h > 0)).sum() > n // 4 and ((coef > 0) & (h <= 0)).sum() > 0
    if hot:
        assert (b[1] == 17).sum() >= 99
    loss, hU, hI, tagU, tagI = run_step(dev, U, I, b, coef, margin, 1e-2, n, users_distinct=distinct and B <= dr.NU)
    print("warp step d=%d B=%d hot=%d distinct=%d: max err loss %.3g gU %.3g gI %.3g (tol %.3g)"
          % (d, B, hot, distinct, np.abs(loss - terms).max(), np.abs(hU - gU).max(), np.abs(hI - gI).max(), tol))
    np.testing.assert_allclose(loss, terms, atol=tol, rtol=0)
    np.testing.assert_allclose(hU, gU, atol=tol, rtol=0)
    np.testing.assert_allclose(hI, gI, atol=tol, rtol=0)
    assert abs(loss[0] - (loss[1] + loss[2])) <= tol
    assert_tags(tagU, tagI, b, 3)


def test_a_zero_coefficient_moves_its_rows_by_the_regulariser_alone(dev):
    d, B = 64, 64
    U, I, b, coef, margin, _ = gaussian_step_case(d, B, 0, True)
    coef = np.zeros_like(coef)
    c = np.float32(1e-2) / np.float32(len(coef))                          # regs / reg_div as the library takes it, in fp32
    loss, hU, hI, _, _ = run_step(dev, U, I, b, coef, margin, 1e-2, len(coef), users_distinct=True)
    assert loss[1] == 0.0 and loss[2] > 0
    np.testing.assert_array_equal(hU[b[0]], c * U[b[0]])                  # the plain store of c u, one rounding
    want = np.zeros_like(I, dtype=np.float64)
    np.add.at(want, b[1], float(c) * I[b[1]].astype(np.float64))
    np.add.at(want, b[2], float(c) * I[b[2]].astype(np.float64))
    np.testing.assert_allclose(hI, want, atol=1e-7, rtol=0)


def test_a_triplet_with_an_id_outside_the_tables_is_skipped(dev):
    d, B = 64, 69
    U, I, b, coef, margin, _ = gaussian_step_case(d, B, 0, False)
    users, pos, neg = (a.copy() for a in b)
    n = len(users)
    users[3], pos[5], neg[7], users[11] = dr.NU, -1, dr.NI, -7
    keep = np.ones(n, dtype=bool)
    keep[[3, 5, 7, 11]] = False
    with pytest.raises(ValueError, match="outside the tables"):
        run_step(dev, U, I, (users, pos, neg), coef, margin, 1e-2, n)
    terms, gU, gI, _ = wr.step_grads(U, I, users[keep], pos[keep], neg[keep], coef[keep], margin=margin, regs=1e-2, reg_div=n, B=n)
    loss, hU, hI, tagU, tagI = run_step(dev, U, I, (users, pos, neg), coef, margin, 1e-2, n, check_ids=False)
    tol = TOL * max(1.0, float(wtab32(64).max()))
    np.testing.assert_allclose(loss, terms, atol=tol, rtol=0)
    np.testing.assert_allclose(hU, gU, atol=tol, rtol=0)
    np.testing.assert_allclose(hI, gI, atol=tol, rtol=0)
    assert_tags(tagU, tagI, (users[keep], pos[keep], neg[keep]), 3)


def test_three_whole_steps_against_the_restatement(dev):
    """Three steps of ops.warp_adam_step against the float64 restatement with the oracle's Adam (oracle/pda_oracle.py), as tests/test_gpu_ips.py
    does it, with that file's tolerances: 1e-5 on tables and moments (the project's fp32 contract on a table entry after three steps), 1e-5
    max(1, largest coefficient) on the loss terms."""
    from pda_amd import ops
    d, B, lr, margin, regs = 32, 64, 1e-2, 1.0, 1e-2
    rng = np.random.default_rng(33)
    U, I = (rng.standard_normal((dr.NU, d)) * 0.3).astype(np.float32), (rng.standard_normal((dr.NI, d)) * 0.3).astype(np.float32)
    Ut, It = to(dev, U, I)
    st = State(Ut, It)
    Ur, Ir, state = U.astype(np.float64), I.astype(np.float64), None
    table = np.concatenate([wtab32(64), np.zeros(8, dtype=np.float32)])
    for t in (1, 2, 3):
        b = tuple(rng.integers(0, n, B).astype(np.int32) for n in (dr.NU, dr.NI, dr.NI))
        coef = rng.choice(table, B).astype(np.float32)
        _, _, _, h = wr.step_grads(Ur, Ir, *b, coef, margin=margin, regs=regs, reg_div=B)
        assert (np.abs(h) > 1e-4).all()                                   # no triplet on the kink of the hinge
        Ur, Ir, state, terms = wr.step_adam(Ur, Ir, state, t, lr, *b, coef, margin=margin, regs=regs, reg_div=B)
        loss = torch.zeros(3, device=dev)
        ops.warp_adam_step(*st.adam(Ut, It), *to(dev, *b, coef), margin=margin, regs=regs, reg_div=B, step=t, lr_t=ops.adam_lr_t(lr, t),
                           loss_acc=loss, check_ids=True)
        np.testing.assert_allclose(np_(loss), terms, atol=TOL * max(1.0, float(coef.max())), rtol=0)
        assert float(st.gU.abs().max()) == 0.0 and float(st.gI.abs().max()) == 0.0
    got = dict(U=Ut, I=It, mU=st.mU, vU=st.vU, mI=st.mI, vI=st.vI)
    want = dict(U=Ur, I=Ir, **state)
    for k in got:
        print("warp three steps: max |%s err| %.3g" % (k, np.abs(np_(got[k]) - want[k]).max()))
    for k in got:
        np.testing.assert_allclose(np_(got[k]), want[k], atol=TOL, rtol=0, err_msg=k)


# ---- 7. through the sampler and the CLI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from pda_amd import synthetic
    root = tmp_path_factory.mktemp("warp_data")
    synthetic.write_dataset(str(root / "toy"), n_users=400, n_items=300, mean_hist=20)
    return str(root) + "/"


def _argv(toy, save, test="normal", extra=()):
    return ["--data_path", toy, "--dataset", "toy", "--train", "warp", "--test", test, "--epoch", "2", "--log_interval", "1",
            "--batch_size", "256", "--lr", "1e-2", "--regs", "1e-2", "--valid_set", "valid", "--pop_exp", "0.22",
            "--save_dir", save, "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t", "--cuda", "0", "--eval_block", "128"] + list(extra)


def written_bytes(u, p, n):
    """The bytes of a triplet plan that the plan kernel writes: where two plans laid over different fillings agree."""
    from pda_amd import ops
    nb = ops.triplet_plan_bytes(u.numel())
    a = ops.triplet_plan(u, p, n, out=torch.zeros((1, nb), dtype=torch.uint8, device=u.device))[0]
    b = ops.triplet_plan(u, p, n, out=torch.full((1, nb), 255, dtype=torch.uint8, device=u.device))[0]
    return a, a == b


def test_the_device_sampler_is_the_call_on_the_tables_as_they_stood(dev, toy, tmp_path):
    """DeviceSampler(mode="warp") hands out (users, pos, neg, coef), drawn on the tables as they stand at each batch; its trial counts add up on
    the device.  Built from the flags --warp_max_trials 1 --warp_margin inf --warp_weight none it draws the uniform sampler's batches, compared
    as written_bytes compares them (the trainer itself refuses a margin that is not finite: check_warp)."""
    from pda_amd import ops, parse
    from pda_amd import train_new_api as t
    from pda_amd.model_api import check_warp
    from pda_amd.sampler import DeviceSampler
    t.configure(_argv(toy, str(tmp_path) + "/"))
    a, data = t.args, t.data
    T, d, B = 16, 64, data.batch_size
    w = ops.WarpWeights.build(data.n_items, T, "harmonic", dev)
    s = DeviceSampler(data, dev, False, mode="warp", max_trials=T, margin=0.5, wtab=w)
    with pytest.raises(ValueError, match="set_tables"):
        s.batch()
    s.step = 0
    gen = torch.Generator(device=dev).manual_seed(3)
    tables = {"U": torch.randn(data.n_users, d, device=dev, generator=gen), "I": torch.randn(data.n_items, d, device=dev, generator=gen)}
    s.set_tables(lambda: (tables["U"], tables["I"]))
    total = none = 0
    for step in (1, 2, 3):
        got = s.batch()
        want = ops.warp_sample(tables["U"], tables["I"], s.indptr, s.indices, B, max_trials=T, margin=0.5, wtab=w.wtab, seed=s.seed, step=step,
                               neg_range=(0, data.n_items), user_pool=s.pool, n_pool=s.pool.numel())
        assert len(got) == 4 and s.plan is None
        for g, x in zip(got, want[:4]):
            assert torch.equal(g.view(torch.int32), x.view(torch.int32)), step
        total, none = total + int(want[4].sum()), none + int((want[4] == 0).sum())
        tables["U"] = tables["U"] + 0.5 * torch.randn(data.n_users, d, device=dev, generator=gen)      # the tables move: new tensors, new values
        tables["I"].add_(0.5 * torch.randn(data.n_items, d, device=dev, generator=gen))
    trials, share = s.take_warp_stat()
    assert trials == total / max(3 * B - none, 1) and share == none / (3 * B) and s.take_warp_stat() == (0.0, 0.0)

    b = parse.parse_args(_argv(toy, str(tmp_path) + "/", extra=("--warp_max_trials", "1", "--warp_margin", "inf", "--warp_weight", "none")))
    with pytest.raises(ValueError, match="--warp_margin"):
        check_warp(b)
    one = DeviceSampler(data, dev, False, mode="warp", max_trials=b.warp_max_trials, margin=b.warp_margin,
                        wtab=ops.WarpWeights.build(data.n_items, b.warp_max_trials, b.warp_weight, dev))
    one.set_tables(lambda: (tables["U"], tables["I"]))
    uni = DeviceSampler(data, dev, False, ahead=1)
    for step in (1, 2):
        g, x = one.batch(), uni.batch()
        (pa, wa), (pb, wb) = written_bytes(*g[:3]), written_bytes(*x[:3])
        assert torch.equal(wa, wb) and wa.float().mean() > 0.5 and torch.equal(pa[wa], pb[wb])
        assert all(torch.equal(p, q) for p, q in zip(g[:3], x[:3])) and (g[3] == 1).all()
    assert one.take_warp_stat() == (1.0, 0.0)


def _cli(module, argv):
    r = subprocess.run([sys.executable, "-m", module] + argv, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_cli_trains_reports_and_leaves_a_bprmf_checkpoint(dev, toy, tmp_path):
    """`--train warp --test normal` trains two epochs, prints the `||--- warp` line under each loss line and writes a checkpoint that loads into
    a plain BPRMF, goes through export_topk and, in the run itself, through --rank_report 1."""
    from pda_amd import model_api, parse
    save = str(tmp_path / "a") + "/"
    out = _cli("pda_amd.train_new_api", _argv(toy, save, extra=("--rank_report", "1")))
    losses = [[float(x) for x in m.groups()] for m in re.finditer(r"Epoch \d+ \[[^\]]*\]: train==\[([-\d.]+)=([-\d.]+) \+ ([-\d.]+)\]", out)]
    assert len(losses) == 2 and np.isfinite(losses).all() and all(l[1] > 0 for l in losses), out[-2000:]
    lines = out.splitlines()
    stats = [(i, re.fullmatch(r"\|\|--- warp trials=(\d+\.\d{3}) none=(\d\.\d{4})", ln)) for i, ln in enumerate(lines) if ln.startswith("||--- warp")]
    assert len(stats) == 2 and all(m for _, m in stats) and all(lines[i - 1].startswith("Epoch ") for i, _ in stats)
    assert all(float(m.group(1)) >= 1.0 and 0.0 <= float(m.group(2)) < 1.0 for _, m in stats)
    assert "recall=[" in out and "||--- rank auc=" in out and "running WARP" in out
    ckpts = [os.path.join(dp, f) for dp, _, fs in os.walk(save) for f in fs if f == "best_ckpt.ckpt"]
    assert len(ckpts) == 1 and ckpts[0].rstrip("/").split("/")[-2].endswith("warp_train_warp")
    sd = torch.load(ckpts[0], map_location=dev)
    assert (sd["warp_margin"], sd["warp_max_trials"], sd["warp_weight"]) == (1.0, 64, "harmonic")
    plain = model_api.BPRMF(parse.parse_args(["--train", "normal", "--batch_size", "256"]), {"n_users": sd["n_users"], "n_items": sd["n_items"]},
                            device=dev)
    plain.load_state_dict(sd)
    assert torch.equal(plain.weights["user_embedding"], sd["user_embedding"]) and torch.equal(plain.weights["item_embedding"], sd["item_embedding"])
    npz = str(tmp_path / "lists.npz")
    _cli("pda_amd.export_topk", _argv(toy, save, extra=("--export_out", npz)))
    lists = np.load(npz)
    assert lists["idx"].ndim == 2 and lists["idx"].shape[0] > 0 and lists["idx"].shape[1] == 50


def test_cli_a_large_margin_closes_every_row_on_its_first_candidate(dev, toy, tmp_path):
    out = _cli("pda_amd.train_new_api", _argv(toy, str(tmp_path / "b") + "/", test="warp", extra=("--warp_margin", "1e6", "--warp_max_trials", "8")))
    stats = [ln for ln in out.splitlines() if ln.startswith("||--- warp")]
    assert stats == ["||--- warp trials=1.000 none=0.0000"] * 2, stats
    assert "---- WARP result:" in out
