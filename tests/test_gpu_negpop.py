"""GPU: popularity-weighted negative sampling (`--neg_sampler pop`, include/pda_hip_negpop.h) against the restatement of tests/negpop_ref.py --
the triplet batch and the [B, N] block bit for bit; the edges of the draw on hand-made tables; an all-full table IS the uniform sampler; the
look-ahead call and the device counter; the logQ step of include/pda_hip_ssm.h against float64; the entry points' refusals; the sampler
object; the command line."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import negpop_ref as nr
import sampler_ref as sr
import ssm_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NU = 120
FULL = (1 << 32) - 1
BIG = [(2020, 1), (1 << 32, (1 << 32) + 3), ((1 << 63) + 1, (1 << 63) + 7), ((1 << 64) - 1, (1 << 64) - 2)]


def to(dev, *arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def np_(t):
    return None if t is None else t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def world(n, lo=0, extra=0, beta=1.0):
    """A train graph over lo + n + extra items (heavy users, empty rows, Zipf items), the table ops builds for [lo, lo + n) and a popularity
    matrix.  Computed once per shape and shared."""
    from pda_amd import ops
    n_items = lo + n + extra
    indptr, indices, slots = nr.toy_graph(NU, n_items, 100 + n)
    table = ops.NegPopTable(indices, n_items, beta, (lo, lo + n), "cpu")
    pop = np.random.default_rng(n).random((n_items, 4)).astype(np.float32)
    return indptr, indices, slots, table, pop


def on(dev, table):
    from pda_amd import ops
    return ops.NegPopTable.from_slots(table.thr, table.alias, table.neg_range, table.n_items, dev, q=table.q)


def same_bits(got, want, what):
    assert (got is None) == (want is None), what
    if got is not None:
        g, w = np_(got) if torch.is_tensor(got) else got, np_(want) if torch.is_tensor(want) else want
        assert g.shape == w.shape and np.array_equal(g.view(np.int32), w.view(np.int32)), what


def repeated_users(B):
    u = np.random.default_rng(B).integers(0, NU, B).astype(np.int32)
    u[B // 2:] = u[:B - B // 2]                                        # every id of the first half occurs again
    return u


# ---- 1. the triplet batch, bit for bit -----------------------------------------------------------------------------------------------------------
TRIPLETS = [  # n, lo, extra, B, with_pop, given users, (seed, step)
    (1000, 0, 0, 1, False, False, BIG[0]), (1000, 0, 0, 37, True, False, BIG[1]), (1000, 0, 0, 2048, True, False, BIG[0]),
    (1000, 17, 5, 37, True, False, BIG[2]), (1000, 17, 5, 2048, False, True, BIG[3]), (1000, 17, 5, 37, True, True, BIG[0]),
    (1, 0, 0, 37, True, False, BIG[0]), (1, 3, 2, 37, False, True, BIG[1]), (2, 0, 0, 37, True, False, BIG[2]), (3, 0, 0, 37, False, False, BIG[0]),
    (3, 2, 0, 2048, True, True, BIG[3])]


@pytest.mark.parametrize("n, lo, extra, B, with_pop, given, seed_step", TRIPLETS)
def test_the_triplet_batch_is_the_restatement_bit_for_bit(dev, n, lo, extra, B, with_pop, given, seed_step):
    from pda_amd import ops
    seed, step = seed_step
    indptr, indices, slots, table, pop = world(n, lo, extra)
    users = repeated_users(B) if given else None
    pool = np.arange(NU, dtype=np.int32)[::-1].copy()
    want = nr.sample(seed, step, B, indptr, indices, table.thr, table.alias, neg_lo=lo, slots=slots if with_pop else None, user_pool=pool, n_pool=NU,
                     users=users, pop_matrix=pop if with_pop else None)
    ip, ix, sl, pm, us, pl = to(dev, indptr, indices, slots if with_pop else None, pop if with_pop else None, users, pool)
    got = ops.negpop_sample_triplets(on(dev, table), ip, ix, B, seed=seed, step=step, users=us, user_pool=pl, n_pool=NU, train_slots=sl, pop_matrix=pm)
    torch.cuda.synchronize()
    for g, k in zip(got, ("users", "pos", "neg", "pos_pop", "neg_pop")):
        same_bits(g, want[k], k)
    neg = np_(got[2])
    assert ((neg >= lo) & (neg < lo + n)).all()
    print("n=%d B=%d: mean tries %.2f, most %d" % (n, B, 1 + want["rejections"].mean(), 1 + want["rejections"].max()))


# ---- 2. the [B, N] block, bit for bit ------------------------------------------------------------------------------------------------------------
BLOCKS = [(1000, 0, 1, 1, False, BIG[0]), (1000, 0, 37, 7, False, BIG[1]), (1000, 17, 37, 256, True, BIG[2]), (1000, 0, 2048, 1, False, BIG[3]),
          (1000, 17, 2048, 7, True, BIG[0]), (1000, 0, 2048, 256, False, BIG[0]), (1, 0, 37, 7, False, BIG[0]), (2, 0, 1, 256, True, BIG[1]),
          (3, 2, 37, 7, False, BIG[2])]


@pytest.mark.parametrize("n, lo, B, N, given, seed_step", BLOCKS)
def test_the_block_is_the_restatement_bit_for_bit(dev, n, lo, B, N, given, seed_step):
    from pda_amd import ops
    seed, step = seed_step
    indptr, indices, _, table, _ = world(n, lo, 5 if lo else 0)
    users = repeated_users(B) if given else None
    want = nr.block(seed, step, B, N, indptr, indices, table.thr, table.alias, neg_lo=lo, n_pool=NU, users=users)
    ip, ix, us = to(dev, indptr, indices, users)
    t = on(dev, table)
    u, p, negs = ops.negpop_ssm_sample(t, ip, ix, B, N, seed=seed, step=step, users=us, n_pool=NU)
    torch.cuda.synchronize()
    same_bits(u, want["users"], "users"), same_bits(p, want["pos"], "pos"), same_bits(negs, want["negs"], "negs")
    tri = ops.negpop_sample_triplets(t, ip, ix, B, seed=seed, step=step, users=us, n_pool=NU)
    assert torch.equal(negs[:, 0], tri[2]) and torch.equal(p, tri[1]) and torch.equal(u, tri[0])        # column 0 is the triplet entry's negative
    print("n=%d B=%d N=%d: mean tries %.2f" % (n, B, N, 1 + want["rejections"].mean()))


# ---- 3. look-ahead, the device counter -----------------------------------------------------------------------------------------------------------
def counter(dev, step):
    return torch.from_numpy(np.array([step & sr.MASK, 0], dtype=np.uint64).view(np.int64)).to(dev)


@pytest.mark.parametrize("with_pop, step0", [(True, 1), (False, (1 << 63) + 5)])
def test_one_look_ahead_call_is_thirty_two_single_calls(dev, with_pop, step0):
    from pda_amd import ops
    B, n, lo = 37, 1000, 17
    indptr, indices, slots, table, pop = world(n, lo, 5)
    ip, ix, sl, pm = to(dev, indptr, indices, slots if with_pop else None, pop if with_pop else None)
    t = on(dev, table)
    kw = dict(seed=2020, n_pool=NU, train_slots=sl, pop_matrix=pm)
    i32, f32 = (lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)), (lambda *s: torch.full(s, -7.0, dtype=torch.float32, device=dev))
    out = (i32(32, B), i32(32, B), i32(32, B)) + ((f32(32, B), f32(32, B)) if with_pop else (None, None))
    ctr = counter(dev, step0)
    ops.negpop_sample_batches_into(out, t, ip, ix, step_dev=ctr, parity=0, **kw)
    torch.cuda.synchronize()
    assert (ctr[1].item() & sr.MASK) == (step0 + 32) & sr.MASK and (ctr[0].item() & sr.MASK) == step0 & sr.MASK
    one = (i32(B), i32(B), i32(B)) + ((f32(B), f32(B)) if with_pop else (None, None))
    c1 = counter(dev, step0)
    for j in range(32):
        ops.negpop_sample_triplets_into(one, t, ip, ix, step_dev=c1, parity=j & 1, **kw)         # _dev on the two-slot counter
        byval = ops.negpop_sample_triplets(t, ip, ix, B, step=step0 + j, **kw)                   # the by-value call
        for k in range(5):
            same_bits(None if out[k] is None else out[k][j], one[k], (j, k)), same_bits(one[k], byval[k], (j, k))
        assert (c1[(j + 1) & 1].item() & sr.MASK) == (step0 + j + 1) & sr.MASK
    # the same batches over buffers that held something else: nothing read from them
    out2 = tuple(None if o is None else torch.zeros_like(o) for o in out)
    ops.negpop_sample_batches_into(out2, t, ip, ix, step_dev=counter(dev, step0), parity=0, **kw)
    for a, b in zip(out, out2):
        same_bits(a, b, "fill")


def test_the_block_with_a_device_counter_is_the_by_value_call(dev):
    from pda_amd import ops
    B, N = 37, 7
    indptr, indices, _, table, _ = world(1000, 17, 5)
    ip, ix = to(dev, indptr, indices)
    t = on(dev, table)
    ctr = counter(dev, 5)
    out = tuple(torch.full(s, -7, dtype=torch.int32, device=dev) for s in ((B,), (B,), (B, N)))
    for j in range(4):
        ops.negpop_ssm_sample_into(out, t, ip, ix, seed=9, step_dev=ctr, parity=j & 1, n_pool=NU)
        want = ops.negpop_ssm_sample(t, ip, ix, B, N, seed=9, step=5 + j, n_pool=NU)
        for a, b in zip(out, want):
            same_bits(a, b, j)
    ops.negpop_ssm_sample_into(out, t, ip, ix, seed=9, step_dev=ctr[:1], n_pool=NU)              # read only: slot 0 holds 9
    same_bits(out[2], ops.negpop_ssm_sample(t, ip, ix, B, N, seed=9, step=9, n_pool=NU)[2], "read only")
    assert ctr.tolist() == [9, 8]


# ---- 4. the edges of the draw, on hand-made tables -------------------------------------------------------------------------------------------------
def hand_made(dev, thr, alias, rows, B=256, lo=0, seed=2020, step=3):
    """Every user holds the train items `rows` (a list); -> (negatives of the device, the restatement's dict, slot and coin of try 0 per row)."""
    from pda_amd import ops
    n = len(thr)
    indptr = np.arange(NU + 1, dtype=np.int64) * len(rows)
    indices = np.tile(np.asarray(sorted(rows), dtype=np.int32), NU)
    t = ops.NegPopTable.from_slots(thr, alias, (lo, lo + n), lo + n, dev)
    ip, ix = to(dev, indptr, indices if len(rows) else np.zeros(1, np.int32))
    users = (np.arange(B) % NU).astype(np.int32)
    got = ops.negpop_sample_triplets(t, ip, ix, B, seed=seed, step=step, users=to(dev, users)[0])
    torch.cuda.synchronize()
    want = nr.sample(seed, step, B, indptr, indices, np.asarray(thr, np.uint32), np.asarray(alias, np.uint32), neg_lo=lo, users=users)
    r = np.arange(B)
    slot = sr.bounded(sr.draw(seed, step, r, 16), n).astype(np.int64)
    coin = sr.draw(seed, step, r, 16 | nr.COIN)
    same_bits(got[2], want["neg"], "neg")
    return np_(got[2]).astype(np.int64), want, slot, coin


def test_a_zero_threshold_never_keeps_the_slot(dev):
    n = 8
    neg, want, slot, _ = hand_made(dev, [0] * n, [(s + 1) % n for s in range(n)], [], lo=4)
    assert np.array_equal(neg, 4 + (slot + 1) % n) and (want["rejections"] == 0).all()


def test_the_largest_threshold_keeps_the_slot_unless_the_coin_is_all_ones(dev):
    n = 8
    neg, _, slot, coin = hand_made(dev, [FULL] * n, [(s + 1) % n for s in range(n)], [])
    keep = coin != np.uint64(FULL)
    assert keep.any() and np.array_equal(neg[keep], slot[keep]) and np.array_equal(neg[~keep], (slot[~keep] + 1) % n)


def test_a_slot_aliased_to_a_train_item_is_rejected(dev):
    # slot 0 always hands over to item 1, which every user holds: tries that land on slot 0 or 1 are drawn again
    neg, want, slot, _ = hand_made(dev, [0, FULL, FULL, FULL], [1, 1, 2, 3], [1])
    assert set(neg.tolist()) == {2, 3} and (want["rejections"][slot < 2] > 0).all() and (want["rejections"][slot >= 2] == 0).all()


def test_a_row_whose_train_items_hold_all_the_mass_keeps_its_last_draw(dev):
    neg, want, _, _ = hand_made(dev, [0, 0, FULL, 0], [2, 2, 2, 2], [2], B=64)
    assert (neg == 2).all() and (want["rejections"] == sr.REJECT_CAP).all()


def test_a_row_that_leaves_one_drawable_item_gets_it(dev):
    neg, want, _, _ = hand_made(dev, [1 << 31, FULL, 1 << 30], [2, 1, 1], [0, 1], B=64, lo=0)
    assert (neg == 2).all() and want["rejections"].max() < sr.REJECT_CAP


# ---- 5. the identity: an all-full table is the uniform sampler ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, lo, with_pop", [(1, 0, False), (37, 17, True), (2048, 17, True), (2048, 0, False)])
def test_an_all_full_table_is_the_uniform_sampler_bit_for_bit(dev, B, lo, with_pop):
    from pda_amd import ops
    n = 1000
    indptr, indices, slots, _, pop = world(n, lo, 5 if lo else 0)
    n_items = lo + n + (5 if lo else 0)
    full = ops.NegPopTable(indices, n_items, 0.0, (lo, lo + n), dev)                  # power 0: every slot full by construction
    assert full.all_full()
    ip, ix, sl, pm = to(dev, indptr, indices, slots if with_pop else None, pop if with_pop else None)
    kw = dict(n_pool=NU, train_slots=sl, pop_matrix=pm)
    for seed, step in BIG[:3]:
        got = ops.negpop_sample_triplets(full, ip, ix, B, seed=seed, step=step & sr.MASK, **kw)
        want = ops.sample_triplets(ip, ix, B, seed=seed, step=step & sr.MASK, neg_range=(lo, lo + n), **kw)
        for k, (g, w) in enumerate(zip(got, want)):
            same_bits(g, w, (k, seed))
    for N in (1, 7, 256):
        got = ops.negpop_ssm_sample(full, ip, ix, B, N, seed=11, step=4, n_pool=NU)
        want = ops.ssm_sample(ip, ix, B, N, seed=11, step=4, neg_range=(lo, lo + n), n_pool=NU)
        for k, (g, w) in enumerate(zip(got, want)):
            same_bits(g, w, (k, N))
    i32, f32 = (lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)), (lambda *s: torch.zeros(s, dtype=torch.float32, device=dev))
    mk = lambda: (i32(4, B), i32(4, B), i32(4, B)) + ((f32(4, B), f32(4, B)) if with_pop else (None, None))    # noqa: E731
    a, b = mk(), mk()
    ops.negpop_sample_batches_into(a, full, ip, ix, seed=3, step_dev=counter(dev, 7), parity=0, **kw)
    ops.sample_batches_into(b, ip, ix, seed=3, step_dev=counter(dev, 7), parity=0, neg_range=(lo, lo + n), **kw)
    for k, (g, w) in enumerate(zip(a, b)):
        same_bits(g, w, ("ahead", k))


def test_a_skewed_table_draws_popular_items_more_often(dev):
    """200 000 negatives of users without train items at beta = 1 against the table's exact distribution and against the uniform one: the
    chi-square of tests/test_negpop_host.py on what the DEVICE drew."""
    from pda_amd import ops
    n, B, N = 37, 2048, 98
    counts = nr.pareto_counts(n)
    table = ops.NegPopTable(np.repeat(np.arange(n), counts).astype(np.int32), n, 1.0, (0, n), dev)
    ip, ix = to(dev, np.zeros(NU + 1, dtype=np.int64), np.zeros(1, dtype=np.int32))
    negs = np_(ops.negpop_ssm_sample(table, ip, ix, B, N, seed=5, step=1, n_pool=NU)[2]).ravel()
    obs = np.bincount(negs, minlength=n).astype(np.float64)
    P = np.array([float(p) for p in nr.implied(table.thr, table.alias)])
    stat = lambda exp: float((((obs - exp) ** 2) / exp).sum())           # noqa: E731
    a, b = stat(P * negs.size), stat(np.full(n, negs.size / n))
    print("chi2(36) of %d device draws: %.1f against P (tail %.3g), %.1f against uniform (tail %.3g)"
          % (negs.size, a, nr.chi2_sf(a, n - 1), b, nr.chi2_sf(b, n - 1)))
    assert nr.chi2_sf(a, n - 1) > 1e-6 > nr.chi2_sf(b, n - 1)


# ---- 6. the logQ step against float64 ----------------------------------------------------------------------------------------------------------------
#           d   B   N  n_items norm tau
LOGQ = [(32, 1, 1, 20, 0, 1.0), (32, 69, 7, 50, 1, 0.1), (64, 5, 64, 500, 0, 0.1), (64, 69, 64, 200, 1, 1.0), (128, 69, 1, 20, 1, 0.1),
        (128, 5, 7, 500, 0, 1.0), (256, 69, 64, 500, 1, 0.1), (256, 1, 64, 50, 0, 0.1)]


def logq_case(d, B, N, n_items, seed):
    rng = np.random.default_rng(seed)
    U, I = ssm_ref.tables(rng, d, nU=40, nI=n_items)
    users = rng.integers(0, 40, B).astype(np.int32)
    pos = rng.integers(0, n_items, B).astype(np.int32)
    negs = rng.integers(0, n_items, (B, N)).astype(np.int32)
    q = nr.weights(np.floor(rng.pareto(1.2, n_items) * 3.0), 1.0)
    return U, I, users, pos, negs, np.log(q / q.sum()).astype(np.float32)


class State:
    def __init__(self, Ut, It):
        from pda_amd import ops
        z = torch.zeros_like
        self.mU, self.vU, self.gU, self.mI, self.vI, self.gI = z(Ut), z(Ut), z(Ut), z(It), z(It), z(It)
        self.tagU, self.tagI = ops.adam_row_tags(Ut.shape[0], It.shape[0], Ut.device)
        self.loss = torch.zeros(3, device=Ut.device)


@pytest.mark.parametrize("d, B, N, n_items, norm, tau", LOGQ)
def test_the_logq_step_against_float64(dev, d, B, N, n_items, norm, tau):
    """Gradients within ssm_ref.tolerance(tau) -- logq reaches them only through p_k <= 1 --, loss terms within 1e-5 max(1, 1 / tau + max |logq|);
    logq = NULL through the new entry within 2e-6 of the existing entry (the figure of the graph-replay test)."""
    from pda_amd import _lib, ops
    U, I, users, pos, negs, logq = logq_case(d, B, N, n_items, 1000 * d + N + B)
    kw = dict(tau=tau, norm=norm, regs=ssm_ref.REGS, reg_div=B)
    want_t, want_gU, want_gI = nr.logq_grads(U, I, users, pos, negs, logq, **kw)
    Ut, It, ut, pt, nt, lq = to(dev, U, I, users, pos, negs, logq)
    st = State(Ut, It)
    ops.ssm_step(Ut, It, ut, pt, nt, st.gU, st.gI, st.tagU, st.tagI, step=1, loss_acc=st.loss, logq=lq, **kw)
    torch.cuda.synchronize()
    eg = max(np.abs(np_(st.gU) - want_gU).max(), np.abs(np_(st.gI) - want_gI).max())
    el = np.abs(np_(st.loss).astype(np.float64) - want_t).max()
    tol_g, tol_l = ssm_ref.tolerance(tau), nr.loss_tolerance(tau, logq)
    print("d=%d B=%d N=%d norm=%d tau=%g: gradients %.2e (tolerance %.1e), loss terms %.2e (%.1e), max |logq| %.2f"
          % (d, B, N, norm, tau, eg, tol_g, el, tol_l, np.abs(logq).max()))
    assert eg <= tol_g and el <= tol_l
    touched = np.unique(np.concatenate([pos, negs.ravel()]))
    assert set(np.flatnonzero(np_(st.tagI)).tolist()) == set(touched.tolist()) and set(np.flatnonzero(np_(st.tagU)).tolist()) == set(users.tolist())
    # NULL through the new entry against the existing entry
    a, b = State(Ut, It), State(Ut, It)
    ops.ssm_step(Ut, It, ut, pt, nt, a.gU, a.gI, a.tagU, a.tagI, step=1, loss_acc=a.loss, **kw)
    p = _lib.ptr
    rc = _lib.load().pda_ssm_step_logq_f32(p(Ut), p(It), 40, n_items, p(ut), p(pt), p(nt), None, B, N, d, tau, norm, ssm_ref.REGS, float(B), p(b.gU),
                                           p(b.gI), p(b.tagU), p(b.tagI), 1, 0x100, p(b.loss), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    en = max(float((a.gU - b.gU).abs().max()), float((a.gI - b.gI).abs().max()), float((a.loss - b.loss).abs().max()))
    print("    NULL through the new entry against the existing entry: %.2e" % en)
    assert en <= 2e-6
    # and a table of zeros is no correction either
    c = State(Ut, It)
    ops.ssm_step(Ut, It, ut, pt, nt, c.gU, c.gI, c.tagU, c.tagI, step=1, loss_acc=c.loss, logq=torch.zeros_like(lq), **kw)
    assert max(float((a.gU - c.gU).abs().max()), float((a.gI - c.gI).abs().max()), float((a.loss - c.loss).abs().max())) <= 2e-6


@pytest.mark.parametrize("norm", [0, 1])
def test_the_logq_adam_step_is_the_logq_gradient_under_the_shared_sweep(dev, norm):
    """pda_ssm_adam_step_logq_f32 against float64: the gradients of the restatement, then the project's Adam restatement; tables within 1e-5 at the
    trainer's default rate (ssm_ref.ADAM_STEPS has the reasoning)."""
    from oracle import pda_oracle as po
    from pda_amd import ops
    c = ssm_ref.ADAM_STEPS
    U, I, users, pos, negs, logq = logq_case(c["d"], c["B"], c["N"], 200, 77)
    kw = dict(tau=c["tau"], norm=norm, regs=ssm_ref.REGS, reg_div=c["B"])
    terms, gU, gI = nr.logq_grads(U, I, users, pos, negs, logq, **kw)
    z = np.zeros_like
    U1, _, _ = po.adam_dense_decay_step(U.astype(np.float64), z(gU), z(gU), gU, 1, c["lr"])
    I1, _, _ = po.adam_dense_decay_step(I.astype(np.float64), z(gI), z(gI), gI, 1, c["lr"])
    Ut, It, ut, pt, nt, lq = to(dev, U, I, users, pos, negs, logq)
    st = State(Ut, It)
    ops.ssm_adam_step(Ut, st.mU, st.vU, st.gU, st.tagU, It, st.mI, st.vI, st.gI, st.tagI, ut, pt, nt, step=1, lr_t=ops.adam_lr_t(c["lr"], 1),
                      loss_acc=st.loss, logq=lq, check_ids=True, **kw)
    torch.cuda.synchronize()
    eu, ei = np.abs(np_(Ut) - U1).max(), np.abs(np_(It) - I1).max()
    print("norm=%d: tables after one step %.2e / %.2e, loss terms %.2e" % (norm, eu, ei, np.abs(np_(st.loss) - terms).max()))
    assert eu <= 1e-5 and ei <= 1e-5 and np.abs(np_(st.loss) - terms).max() <= nr.loss_tolerance(c["tau"], logq)
    assert float(st.gU.abs().max()) == 0.0 and float(st.gI.abs().max()) == 0.0          # the sweep zeroes what the step wrote
    no = State(*to(dev, U, I))
    U0, I0 = to(dev, U, I)
    ops.ssm_adam_step(U0, no.mU, no.vU, no.gU, no.tagU, I0, no.mI, no.vI, no.gI, no.tagI, ut, pt, nt, step=1, lr_t=ops.adam_lr_t(c["lr"], 1), **kw)
    assert not torch.equal(U0, Ut)                                                       # the correction does something


# ---- 7. the entry points refuse before they launch ---------------------------------------------------------------------------------------------------
def test_every_argument_error_comes_back_before_any_launch(dev):
    from pda_amd import _lib
    lib = _lib.load()
    indptr, indices, slots, table, pop = world(1000, 0, 0)
    ip, ix, sl, pm = to(dev, indptr, indices, slots, pop)
    t = on(dev, table)
    B, N = 8, 4
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)      # noqa: E731
    users, pos, neg, negs = i32(B), i32(B), i32(B), i32(B, N)
    pp, pn = torch.full((B,), -7.0, device=dev), torch.full((B,), -7.0, device=dev)
    ctr = counter(dev, 1)
    p, NULL, s = _lib.ptr, None, _lib.stream_ptr()

    def tri(users=p(users), gen=1, n_pool=NU, B=B, ip=p(ip), ix=p(ix), lo=0, hi=1000, alias=p(t.table), pop=p(pm), n_slots=4, pos=p(pos), neg=p(neg),
            pp=p(pp), pn=p(pn)):
        return lib.pda_negpop_sample_triplets(users, gen, NULL, n_pool, B, ip, ix, p(sl), lo, hi, alias, pop, n_slots, 1, 1, pos, neg, pp, pn, s)

    def tri_dev(alias=p(t.table), sd=p(ctr[:1]), sn=p(ctr[1:]), B=B, n=None):
        if n is None:
            return lib.pda_negpop_sample_triplets_dev(p(users), 1, NULL, NU, B, p(ip), p(ix), p(sl), 0, 1000, alias, p(pm), 4, 1, sd, sn, p(pos), p(neg),
                                                      p(pp), p(pn), s)
        return lib.pda_negpop_sample_batches_dev(p(users), 1, NULL, NU, B, n, p(ip), p(ix), p(sl), 0, 1000, alias, p(pm), 4, 1, sd, sn, p(pos), p(neg),
                                                 p(pp), p(pn), s)

    def blk(alias=p(t.table), B=B, N=N, users=p(users), gen=1, n_pool=NU, lo=0, hi=1000, negs=p(negs), dev_=False, sd=p(ctr[:1]), sn=p(ctr[1:])):
        if dev_:
            return lib.pda_negpop_ssm_sample_dev(users, gen, NULL, n_pool, B, N, p(ip), p(ix), lo, hi, alias, 1, sd, sn, p(pos), negs, s)
        return lib.pda_negpop_ssm_sample(users, gen, NULL, n_pool, B, N, p(ip), p(ix), lo, hi, alias, 1, 1, p(pos), negs, s)

    assert tri(alias=NULL) == ERR_ARG and tri_dev(alias=NULL) == ERR_ARG and tri_dev(alias=NULL, n=1) == ERR_ARG
    assert blk(alias=NULL) == ERR_ARG and blk(alias=NULL, dev_=True) == ERR_ARG
    # whatever the uniform twins refuse
    for kw in (dict(users=NULL), dict(ip=NULL), dict(ix=NULL), dict(pos=NULL), dict(neg=NULL), dict(n_pool=0), dict(B=0), dict(B=-1), dict(lo=5, hi=5),
               dict(lo=6, hi=5), dict(pp=NULL), dict(pn=NULL), dict(n_slots=0)):
        assert tri(**kw) == ERR_ARG, kw
    assert tri_dev(sd=NULL) == ERR_ARG and tri_dev(sn=p(ctr[:1])) == ERR_ARG and tri_dev(n=0) == ERR_ARG and tri_dev(n=65536) == ERR_ARG
    assert tri_dev(sd=NULL, n=2) == ERR_ARG and tri_dev(sn=p(ctr[:1]), n=2) == ERR_ARG and tri_dev(B=0, n=2) == ERR_ARG
    for kw in (dict(N=0), dict(N=257), dict(B=0), dict(B=(1 << 22) + 1), dict(users=NULL), dict(negs=NULL), dict(n_pool=0), dict(lo=3, hi=3)):
        assert blk(**kw) == ERR_ARG and blk(dev_=True, **kw) == ERR_ARG, kw
    assert blk(dev_=True, sd=NULL) == ERR_ARG and blk(dev_=True, sn=p(ctr[:1])) == ERR_ARG
    torch.cuda.synchronize()
    for x in (users, pos, neg, negs):
        assert int((x != -7).sum()) == 0                                  # nothing was launched
    assert float((pp != -7).sum()) == 0 and ctr.tolist() == [1, 0]
    assert tri() == 0 and tri_dev() == 0 and tri_dev(n=1) == 0 and blk() == 0 and blk(dev_=True) == 0       # and the sound calls run
    torch.cuda.synchronize()
    assert int((neg == -7).sum()) == 0 and int((negs == -7).sum()) == 0


# ---- 8. through the sampler --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from pda_amd import synthetic
    root = tmp_path_factory.mktemp("negpop_data")
    synthetic.write_dataset(str(root / "toy"), n_users=400, n_items=300, mean_hist=20)
    return str(root) + "/"


def _argv(toy, save, train, extra=()):
    return ["--data_path", toy, "--dataset", "toy", "--train", train, "--test", "normal" if train == "ssm" else train, "--epoch", "2",
            "--log_interval", "1", "--batch_size", "256", "--lr", "1e-2", "--regs", "1e-2", "--valid_set", "valid", "--pop_exp", "0.22",
            "--save_dir", save, "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t", "--cuda", "0", "--eval_block", "128", "--embed_size", "32",
            "--ssm_negs", "8"] + list(extra)


@pytest.mark.parametrize("config", ["with_pop", "with_plan", "ssm"])
def test_the_device_sampler_hands_out_the_calls_batches(dev, toy, tmp_path, config):
    from pda_amd import ops
    from pda_amd import train_new_api as t
    from pda_amd.sampler import DeviceSampler
    with_pop = config == "with_pop"
    t.configure(_argv(toy, str(tmp_path) + "/", "s_condition" if with_pop else "normal"))
    a, data = t.args, t.data
    if with_pop:
        data.add_expo_popularity(np.power(t.get_popularity_from_load(t.load_popularity(a)), a.pop_exp))
    table = ops.NegPopTable(data.train_csr("cpu")[1], data.n_items, 1.0, (0, data.n_items), dev)
    B = data.batch_size
    if config == "ssm":
        s = DeviceSampler(data, dev, False, mode="ssm", n_negs=8, ahead=4, neg_table=table)
        uni = DeviceSampler(data, dev, False, mode="ssm", n_negs=8, ahead=4)
        for step in range(1, 7):
            got, other = s.batch(), uni.batch()
            want = ops.negpop_ssm_sample(table, s.indptr, s.indices, B, 8, seed=s.seed, step=step, user_pool=s.pool, n_pool=s.pool.numel())
            for g, w in zip(got, want):
                same_bits(g, w, step)
            assert torch.equal(got[0], other[0]) and torch.equal(got[1], other[1]) and not torch.equal(got[2], other[2])
        return
    s = DeviceSampler(data, dev, with_pop, ahead=4, neg_table=table)
    one = DeviceSampler(data, dev, with_pop, ahead=1, neg_table=table)
    s.with_plan = one.with_plan = not with_pop
    for step in range(1, 7):
        got, single = s.batch(), one.batch()
        want = ops.negpop_sample_triplets(table, s.indptr, s.indices, B, seed=s.seed, step=step, user_pool=s.pool, n_pool=s.pool.numel(),
                                          train_slots=s.slots if with_pop else None, pop_matrix=s.pop)
        assert len(got) == len(single) == (5 if with_pop else 3)
        for g, o, w in zip(got, single, want):
            same_bits(g, w, step), same_bits(o, w, step)
        assert (s.plan is None) == with_pop and (one.plan is None) == with_pop
    assert not torch.equal(got[2], DeviceSampler(data, dev, with_pop, ahead=1).batch()[2])


# ---- 9. through the command line ---------------------------------------------------------------------------------------------------------------------
def _cli(toy, save, train, extra):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "pda_amd.train_new_api"] + _argv(toy, save, train, extra), cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _figures(out):
    """The lines of a run that carry losses and metrics, the wall-clock seconds of the epoch lines taken out."""
    keep = [re.sub(r"^(Epoch \d+) \[[^\]]*\]", r"\1", ln) for ln in out.splitlines() if ln.startswith("Epoch ") or ln.startswith("||---")]
    return [ln for ln in keep if "time:" not in ln and "neg_sampler pop" not in ln]


def _losses(out):
    return [[float(x) for x in m.groups()] for m in re.finditer(r"Epoch \d+ \[[^\]]*\]: train==\[([-\d.]+)=([-\d.]+) \+ ([-\d.]+)\]", out)]


@pytest.mark.parametrize("train, extra", [("normal", ()), ("s_condition", ()), ("ssm", ("--ssm_logq", "0")), ("ssm", ("--ssm_logq", "1"))])
def test_cli_trains_and_evaluates_under_the_popularity_proposal(dev, toy, tmp_path, train, extra):
    save = str(tmp_path / "ckpt") + "/"
    out = _cli(toy, save, train, ("--neg_sampler", "pop", "--neg_pop_power", "1") + tuple(extra))
    banner = [ln for ln in out.splitlines() if ln.startswith("||--- neg_sampler pop")]
    assert len(banner) == 1 and re.match(r"\|\|--- neg_sampler pop power=1 max_q=\S+ entropy=\S+ \(uniform: \S+\)$", banner[0]), banner
    losses = _losses(out)
    assert len(losses) == 2 and np.isfinite(losses).all() and "recall=[" in out and "training and testing end!!!!" in out, out[-2000:]
    best = [os.path.join(dp, f) for dp, _, fs in os.walk(save) for f in fs if f == "best_ckpt.ckpt"]
    assert len(best) == 1 and ("train_%s/" % train) in best[0]                                  # the run directory of its --train
    sd = torch.load(best[0], map_location="cpu")
    if train == "ssm":
        assert (sd["neg_sampler"], sd["neg_pop_power"], sd["ssm_logq"]) == ("pop", 1.0, int(extra[1])) and "ssm_source" not in sd
        if extra[1] == "1":
            from pda_amd import export_topk
            argv = _argv(toy, save, train, ("--neg_sampler", "pop", "--neg_pop_power", "1") + tuple(extra))
            res = export_topk.main(argv + ["--export_out", str(tmp_path / "lists.npz")])
            assert res["idx"].shape == (len(res["users"]), 50) and len(res["users"]) > 0 and np.isfinite(res["val"]).all()
    else:
        assert "neg_sampler" not in sd and "neg_pop_power" not in sd


def test_cli_power_zero_prints_the_uniform_run_s_figures_and_power_one_does_not(dev, toy, tmp_path):
    base = _figures(_cli(toy, str(tmp_path / "a") + "/", "normal", ("--deterministic", "1")))
    zero = _figures(_cli(toy, str(tmp_path / "b") + "/", "normal", ("--deterministic", "1", "--neg_sampler", "pop", "--neg_pop_power", "0")))
    one = _figures(_cli(toy, str(tmp_path / "c") + "/", "normal", ("--deterministic", "1", "--neg_sampler", "pop", "--neg_pop_power", "1")))
    assert len([ln for ln in base if ln.startswith("Epoch ")]) == 2 and any("recall=[" in ln for ln in base)
    assert zero == base and one != base and len([ln for ln in one if ln.startswith("Epoch ")]) == 2
