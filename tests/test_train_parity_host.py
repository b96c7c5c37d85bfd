"""CPU: the power of tests/test_gpu_train_parity.py, proved without a GPU.  The bound of tests/train_ref.py is a bound (an fp32 emulation of the
kernels' expressions, in three summation orders, lies inside it element for element on every case of the GPU list), it separates (every
single-defect mutant of the float64 reference leaves it by more than 10x on a named case of that list), and a record of what the comparator
the old tests use (atol = 1e-5 at B = 2048) lets through."""
import numpy as np
import pytest

from oracle import pda_oracle as po

import train_ref as tr

LR = 0.05


def shared(d, B, kind, pop):
    return tr.shared(d, B, kind, pop, LR)


def test_the_case_list_is_what_the_gpu_tests_rely_on():
    for d in tr.DIMS:
        assert tr.batches(d) == (1, 2048 // d - 1, 2048 // d + 1, 3 * (2048 // d) + 5)
    for d, B, kind in tr.gpu_cases():
        c = tr.case(d, B, kind)
        fw = po.bpr_forward(c.U, c.I, c.users, c.pos, c.neg)
        occ_u, occ_i = tr.occurrences(c)
        if kind == "negative_dots":
            assert (fw["ps"] < 0).all() and (fw["ns"] < 0).all()
        if kind == "spread" and B > 8:
            assert (fw["ps"] > 0).any() and (fw["ps"] < 0).any(), "both ELU branches"
        if kind == "unshared":
            assert occ_u.max() == 1 and occ_i.max() == 1
        if kind == "hot" and B >= 63:
            assert occ_i[7] >= 0.2 * B and occ_u.max() > 1
        if kind == "saturated":
            for pop in (False, True):
                fwp = po.bpr_forward(c.U, c.I, c.users, c.pos, c.neg, *c.heads(pop))
                x = fwp["psw"] - fwp["nsw"]
                for j, t in enumerate(c.sat):
                    assert abs(x[t] - tr.SAT_X[j]) < 1.5, (d, B, pop, j, x[t])
    for d in tr.DIMS:
        for j in range(3):
            c = tr.saturated_single(d, j)
            for pop in (False, True):
                fwp = po.bpr_forward(c.U, c.I, c.users, c.pos, c.neg, *c.heads(pop))
                assert abs((fwp["psw"] - fwp["nsw"])[0] - tr.SAT_X[j]) < 1.5
    c = tr.case(64, 101, "hot", distinct_users=True)
    assert tr.occurrences(c)[0].max() == 1
    c = tr.case(64, 101, "hot", shards=2)
    per = c.I.shape[0] // 2
    assert (c.pos[:50] < per).all() and (c.neg[:50] < per).all() and (c.pos[51:] >= per).all() and (c.neg[51:] >= per).all()


def test_the_mutant_model_without_a_mutant_is_the_oracle():
    for key in ((64, 33, "hot", True), (32, 65, "spread", False), (128, 17, "negative_dots", True), (256, 29, "saturated", True)):
        c, ref, _ = shared(*key)
        got = tr._model(c, key[3], LR, None)
        for q in tr.QUANTITIES:
            np.testing.assert_allclose(got[q], ref[q], rtol=1e-13, atol=1e-300, err_msg=q)


@pytest.mark.parametrize("d", tr.DIMS)
def test_the_bound_is_a_bound(d):
    """|emulation - reference| <= bound, element for element, for every case, emulation order and quantity.  A ratio above 1 means the
    derivation in train_ref's docstring is wrong, not this test."""
    worst = {q: 0.0 for q in tr.QUANTITIES}
    for dd, B, kind in tr.gpu_cases():
        if dd != d:
            continue
        for pop in (False, True):
            c, ref, bnd = shared(d, B, kind, pop)
            for order in tr.ORDERS:
                em = tr.emulate_fp32(c, pop, LR, order)
                for q in tr.QUANTITIES:
                    err = np.abs(em[q].astype(np.float64) - ref[q])
                    assert np.isfinite(em[q]).all() and np.isfinite(bnd[q]).all()
                    assert ((bnd[q] > 0) | (err == 0)).all(), (q, B, kind, pop)
                    ratio = float((err / np.where(bnd[q] > 0, bnd[q], 1.0)).max())
                    worst[q] = max(worst[q], ratio)
                    assert ratio <= 1.0, (q, d, B, kind, pop, order, ratio)
    print("d=%d largest emulation err / bound: %s" % (d, " ".join("%s %.3f" % kv for kv in worst.items())))


def _rows(c, q):
    """The elements of a quantity the batch reaches: all of a per-occurrence array, the batch's rows of a table."""
    if q[-1] == "U" or q == "U_sgd":
        return tr.occurrences(c)[0] > 0
    if q[-1] == "I" or q == "I_sgd":
        return tr.occurrences(c)[1] > 0
    return slice(None)


@pytest.mark.parametrize("name", sorted(tr.MUTANTS))
def test_the_bound_separates(name):
    """On the mutant's named case (one of the GPU list) |mutant - reference| > 10 bound on at least one element of each quantity the mutant is
    declared to change, and on at least half of the elements (of the batch's rows) where it touches every element."""
    m = tr.MUTANTS[name]
    d, B, kind, pop = m["case"]
    assert (d, B, kind) in tr.gpu_cases() and kind in m["kinds"]
    c, ref, bnd = shared(d, B, kind, pop)
    mu = tr.mutant(c, pop, name, LR)
    for q in tr.QUANTITIES:
        sel = _rows(c, q)
        far = (np.abs(mu[q] - ref[q]) > 10 * bnd[q])[sel]
        if q not in m["changes"]:
            continue
        print("%s %s: %.3f of the elements beyond 10 x bound, largest |diff| / bound %.3g" % (
            name, q, far.mean(), (np.abs(mu[q] - ref[q])[sel] / bnd[q][sel]).max()))
        assert far.any(), (name, q)
        if m["everywhere"] == tr.ALL or q in m["everywhere"]:
            if q != "loss":
                assert far.mean() >= 0.5, (name, q, far.mean())


def test_no_eps_shows_on_saturated_only():
    for kind in ("spread", "hot", "negative_dots", "unshared"):
        c, ref, bnd = shared(64, 33, kind, True)
        mu = tr.mutant(c, True, "no_eps", LR)
        assert all((np.abs(mu[q] - ref[q]) <= bnd[q]).all() for q in tr.QUANTITIES)


def _old_inputs(d, with_pop):
    """The inputs of tests/test_gpu_bpr_step.py::test_loss_and_gradients, drawn as that test draws them."""
    rng = np.random.default_rng(d + int(with_pop))
    nU, nI, B = 3000, 900, 2048
    U = (rng.standard_normal((nU, d)) * 0.3).astype(np.float32)
    I = (rng.standard_normal((nI, d)) * 0.3).astype(np.float32)
    users = rng.permutation(nU)[:B].astype(np.int32)
    hi = max(2, nI // 20)
    pos = rng.integers(0, hi, B).astype(np.int32)
    neg = rng.integers(0, hi, B).astype(np.int32)
    one = np.ones(B, np.float32)
    pp = (rng.uniform(0, 1, B) ** 0.22).astype(np.float32) if with_pop else one
    pn = (rng.uniform(0, 1, B) ** 0.22).astype(np.float32) if with_pop else one
    return tr.Case(U, I, users, pos, neg, pp, pn)


@pytest.mark.parametrize("with_pop", [False, True])
@pytest.mark.parametrize("d", [32, 256])
@pytest.mark.parametrize("name", ["no_l2_grad", "l2_twice", "no_eps"])
def test_the_old_comparator_accepts_these_mutants(name, d, with_pop):
    """A record, and the reason this module and test_gpu_train_parity.py exist: on the inputs of test_loss_and_gradients (B = 2048,
    regs = 1e-2), atol = 1e-5 against the float64 oracle accepts a gradient without its L2 term, one with the L2 term twice and one without
    the + 1e-10 of the denominator -- and train_ref's bound on the same inputs rejects the first two by more than 10x on most elements (no input
    of that test saturates a sigmoid, so nothing there can notice the third)."""
    c = _old_inputs(d, with_pop)
    ref, mu = tr.reference(c, with_pop, LR), tr.mutant(c, with_pop, name, LR)
    np.testing.assert_allclose(mu["loss"], ref["loss"], atol=1e-5, rtol=1e-5)
    for q in ("due", "dpe", "dne"):
        np.testing.assert_allclose(mu[q], ref[q], atol=1e-5)              # the old comparator: passes
    bnd = tr.bound(c, with_pop, LR)
    far = np.mean([(np.abs(mu[q] - ref[q]) > 10 * bnd[q]).mean() for q in ("due", "dpe", "dne")])
    print("%s d=%d pop=%d: share of elements beyond 10 x bound %.3f" % (name, d, with_pop, far))
    assert far > 0.5 if name != "no_eps" else far == 0.0
