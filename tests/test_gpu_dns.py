"""GPU: dynamic hard-negative sampling (`--neg_sampler dns`, include/pda_hip_dns.h) against the float64 restatement of tests/dns_ref.py -- M = 1
is the triplet sampler bit for bit; on tables whose dot products are exact in fp32 the candidates, scores, picked columns and negatives ARE
the restatement's; on Gaussian tables every score lies inside its a-priori bound and the pick inside the rank interval the bounds leave; the
invariant of topn = 1; NaN rows; the device counter and a replayed graph; determinism; the sampler object; the CLI."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import dns_ref as dr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 2020
INDPTR, INDICES, SLOTS = dr.graph()
POOL = np.arange(dr.NU, dtype=np.int32)[::-1].copy()


def to(dev, *arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def given_users(B):
    """The users of the exact-data batches: a lone ordinary row; else FULL_USER (all candidates equal), EMPTY_USER, and draws with replacement."""
    if B == 1:
        return np.array([7], dtype=np.int32)
    u = np.random.default_rng(B).integers(0, dr.NU, B).astype(np.int32)
    u[0], u[1], u[B - 1] = dr.FULL_USER, dr.EMPTY_USER, dr.FULL_USER
    return u


def run(dev, U, I, B, M, topn, *, head=dr.HEAD_RAW, step=1, users=None, pop=None, slots=None, neg_range=(0, dr.NI), check_ids=True):
    from pda_amd import ops
    Ut, It, ip, ix, sl, pt, pm, us = to(dev, U, I, INDPTR, INDICES, slots, POOL, pop, users)
    out = ops.dns_sample(Ut, It, ip, ix, B, n_cands=M, topn=topn, head=head, seed=SEED, step=step, neg_range=neg_range, users=us, user_pool=pt,
                         n_pool=dr.NU, train_slots=sl, pop_matrix=pm, want_cands=True, check_ids=check_ids)
    torch.cuda.synchronize()
    return out


def ref(U, I, B, M, topn, *, head=dr.HEAD_RAW, step=1, users=None, pop=None, slots=None, neg_range=(0, dr.NI)):
    return dr.sample(SEED, step, B, M, topn, U, I, INDPTR, INDICES, head=head, slots=slots, user_pool=POOL, n_pool=dr.NU, users=users,
                     neg_range=neg_range, pop_matrix=pop)


def np_(t):
    return None if t is None else t.cpu().numpy()


# ---- 1. identity ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 37, 600])
@pytest.mark.parametrize("with_pop, gen, neg_range", [(False, 1, (0, dr.NI)), (True, 1, (0, dr.NI)), (True, 0, (10, 150)), (False, 0, (10, 150)),
                                                      (True, 1, (10, 150))])
def test_one_candidate_is_the_triplet_sampler_bit_for_bit(dev, B, with_pop, gen, neg_range):
    from pda_amd import ops
    U, I = dr.gaussian_tables(64)
    pop, slots = (dr.pop_matrix(), SLOTS) if with_pop else (None, None)
    users = None if gen else given_users(B)
    ip, ix, sl, pt, pm, us = to(dev, INDPTR, INDICES, slots, POOL, pop, users)
    for step in (1, 2):
        want = ops.sample_triplets(ip, ix, B, seed=SEED, step=step, users=None if us is None else us.clone(), user_pool=pt, n_pool=dr.NU,
                                   train_slots=sl, neg_range=neg_range, pop_matrix=pm)
        for head in (dr.HEAD_RAW,) + ((dr.HEAD_POP,) if with_pop else ()):
            got = run(dev, U, I, B, 1, 1, head=head, step=step, users=users, pop=pop, slots=slots, neg_range=neg_range)
            for k, (g, w) in enumerate(zip(got[:5], want)):
                assert (g is None) == (w is None), k
                if g is not None:
                    assert torch.equal(g.view(torch.int32), w.view(torch.int32)), (k, step, head)
            assert (np_(got[7]) == 0).all() and torch.equal(got[5][:, 0], want[2])


# ---- 2. exact data -------------------------------------------------------------------------------------------------------------------------------
EXACT = [(d, M, topn, B) for d in (32, 64, 128, 256) for M in (2, 5, 32, 256) for topn in sorted({1, 3, M}) if topn <= M for B in (1, 37, 600)]


@functools.lru_cache(maxsize=None)
def exact_ref(d, M, topn, B):
    U, I = dr.exact_tables(d)
    return ref(U, I, B, M, topn, users=given_users(B))


@pytest.mark.parametrize("d, M, topn, B", EXACT)
def test_exact_data_give_the_restatement_itself(dev, d, M, topn, B):
    """Entries that are multiples of 1/8 in [-1, 1]: every fp32 dot product of d <= 256 terms is exact in any order, so nothing is left to a
    tolerance -- candidates, scores, the picked column and the negative equal the float64 restatement."""
    U, I = dr.exact_tables(d)
    want = exact_ref(d, M, topn, B)
    users = given_users(B)
    s = want["score"]
    assert (s == s.astype(np.float32)).all() and (np.abs(s) < 256).all() and (s * 64 == np.round(s * 64)).all()     # exact in fp32, as claimed
    if B > 1:
        full = np.nonzero(users == dr.FULL_USER)[0]
        assert len(full) >= 2 and (want["cand"][full] == dr.FREE_ITEM).all() and (want["pick_col"][full] == want["t"][full]).all()
        assert (want["pos"][users == dr.EMPTY_USER] == 0).all()
    if B == 600 and M >= 32:
        srt = np.sort(want["cand"], 1)
        dup_rows = (srt[:, 1:] == srt[:, :-1]).any(1)
        ssrt = np.sort(s, 1)
        assert dup_rows.mean() > 0.5 and (ssrt[:, 1:] == ssrt[:, :-1]).any(1).mean() > 0.5         # duplicates and ties in most rows
        if d == 32:                                                   # ties between DIFFERENT items too
            o = want["order"]
            so, co = np.take_along_axis(s, o, 1), np.take_along_axis(want["cand"], o, 1)
            assert ((so[:, 1:] == so[:, :-1]) & (co[:, 1:] != co[:, :-1])).any(1).mean() > 0.2
    u, p, n, _, _, cand, score, col = run(dev, U, I, B, M, topn, users=users)
    np.testing.assert_array_equal(np_(u), users)
    np.testing.assert_array_equal(np_(p), want["pos"])
    np.testing.assert_array_equal(np_(cand), want["cand"])
    np.testing.assert_array_equal(np_(score).astype(np.float64), want["score"])
    np.testing.assert_array_equal(np_(col), want["pick_col"])
    np.testing.assert_array_equal(np_(n), want["neg"])


def test_batches_beyond_the_resident_workgroups_take_more_rows_each(dev):
    """The rows of a workgroup double once one round of candidates each would mean more than 512 workgroups (pda_dns.hip, rows_per_block):
    d = 256, M = 2 crosses that at B > 8 192, M = 1 without scores at B > 32 768.  The same two properties as above, on that path."""
    from pda_amd import ops
    B = 20000
    U, I = dr.exact_tables(256)
    users = given_users(B)
    want = ref(U, I, B, 2, 2, users=users)
    _, p, n, _, _, cand, score, col = run(dev, U, I, B, 2, 2, users=users)
    np.testing.assert_array_equal(np_(p), want["pos"])
    np.testing.assert_array_equal(np_(cand), want["cand"])
    np.testing.assert_array_equal(np_(score).astype(np.float64), want["score"])
    np.testing.assert_array_equal(np_(col), want["pick_col"])
    np.testing.assert_array_equal(np_(n), want["neg"])
    B = 70000
    Ut, It, ip, ix, pt = to(dev, U, I, INDPTR, INDICES, POOL)
    tri = ops.sample_triplets(ip, ix, B, seed=SEED, step=3, user_pool=pt, n_pool=dr.NU, neg_range=(0, dr.NI))
    got = ops.dns_sample(Ut, It, ip, ix, B, n_cands=1, seed=SEED, step=3, neg_range=(0, dr.NI), user_pool=pt, n_pool=dr.NU)
    assert all(torch.equal(g, w) for g, w in zip(got[:3], tri[:3]))


# ---- 3. rounded data -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", [dr.HEAD_RAW, dr.HEAD_POP])
@pytest.mark.parametrize("d, M, topn, B", [(64, 32, 3, 600), (32, 5, 5, 37), (128, 256, 1, 37), (256, 32, 32, 600)])
def test_rounded_data_stay_inside_the_a_priori_bound(dev, head, d, M, topn, B):
    U, I = dr.gaussian_tables(d)
    pop = dr.pop_matrix()
    want = ref(U, I, B, M, topn, head=head, pop=pop, slots=SLOTS)
    if (d, M) == (64, 32):                                            # the condition on the inputs: the bound is not what passes the test
        assert dr.single_item_share(want) >= 0.95
    u, p, n, pp, pn, cand, score, col = (np_(t) for t in run(dev, U, I, B, M, topn, head=head, pop=pop, slots=SLOTS))
    np.testing.assert_array_equal(u, want["users"])
    np.testing.assert_array_equal(p, want["pos"])
    np.testing.assert_array_equal(cand, want["cand"])
    np.testing.assert_array_equal(pp, want["pos_pop"])
    err = np.abs(score.astype(np.float64) - want["score"])
    worst = (err / want["bound"]).max()
    print("dns head=%d d=%d M=%d B=%d: worst |score - ref| / bound = %.3g" % (head, d, M, B, worst))
    assert (err <= want["bound"]).all(), worst
    rows = np.arange(B)
    lo, hi = dr.rank_interval(want["score"], want["bound"], col.astype(np.int64))
    assert ((lo <= want["t"]) & (want["t"] < hi)).all()
    np.testing.assert_array_equal(n, cand[rows, col])
    np.testing.assert_array_equal(pn, pop[n.astype(np.int64), want["slot"]])
    print("     rows whose pick is the restatement's: %.4f" % (col == want["pick_col"]).mean())


# ---- 4. invariant --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", [dr.HEAD_RAW, dr.HEAD_POP])
def test_the_best_of_the_candidates_and_column_zero(dev, head):
    from pda_amd import ops
    U, I = dr.gaussian_tables(128)
    pop = dr.pop_matrix()
    B, M = 600, 16
    u, p, n, pp, pn, cand, score, col = run(dev, U, I, B, M, 1, head=head, pop=pop, slots=SLOTS)
    best = score.gather(1, col.long()[:, None])
    assert (best >= score).all()
    first = (score == best).int().argmax(1)
    assert torch.equal(first.int(), col)                              # the first column among equals
    ip, ix, sl, pt, pm = to(dev, INDPTR, INDICES, SLOTS, POOL, pop)
    tri = ops.sample_triplets(ip, ix, B, seed=SEED, step=1, user_pool=pt, n_pool=dr.NU, train_slots=sl, neg_range=(0, dr.NI), pop_matrix=pm)
    assert torch.equal(cand[:, 0], tri[2]) and torch.equal(u, tri[0]) and torch.equal(p, tri[1]) and torch.equal(pp, tri[3])


# ---- 5. NaN ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topn", [1, 4])
def test_nan_scores_rank_last(dev, topn):
    U, I = dr.exact_tables(64)
    U, I = U.copy(), I.copy()
    bad_items = np.arange(0, dr.NI, 3)
    I[bad_items] = np.nan                                             # a third of the catalogue
    B, M = 37, 8
    users = given_users(B)
    nan_user = int(users[5])
    assert nan_user not in (dr.FULL_USER, dr.EMPTY_USER)
    U[nan_user] = np.nan                                              # every score of this user's rows
    want = ref(U, I, B, M, topn, users=users)
    s = want["score"]
    mixed = np.isnan(s).any(1) & ~np.isnan(s).all(1)
    assert mixed.sum() > B // 2 and np.isnan(s[users == nan_user]).all()
    assert not np.isnan(s[np.arange(B), want["pick_col"]])[~np.isnan(s).all(1) & ((~np.isnan(s)).sum(1) >= topn)].any()
    all_nan = np.isnan(s).all(1)
    assert (want["pick_col"][all_nan] == want["t"][all_nan]).all()
    _, _, n, _, _, cand, score, col = (np_(t) for t in run(dev, U, I, B, M, topn, users=users))
    np.testing.assert_array_equal(cand, want["cand"])
    np.testing.assert_array_equal(np.isnan(score), np.isnan(s))
    np.testing.assert_array_equal(score[~np.isnan(s)].astype(np.float64), s[~np.isnan(s)])
    np.testing.assert_array_equal(col, want["pick_col"])
    np.testing.assert_array_equal(n, want["neg"])


def test_an_unknown_user_reads_nothing_and_takes_candidate_zero(dev):
    """Memory safety of the library call (ops refuses such ids on the host): a user id outside [0, n_users) is drawn as a user without train
    items, scores nothing and takes candidate 0; its neighbours are untouched."""
    from pda_amd import ops
    U, I = dr.exact_tables(32)
    B, M = 37, 5
    users = given_users(B)
    good = ref(U, I, B, M, 3, users=users)
    bad = users.copy()
    bad[[2, 30]] = [dr.NU, -1]
    with pytest.raises(ValueError, match="user id"):
        run(dev, U, I, B, M, 3, users=bad)
    u, p, n, _, _, cand, score, col = (np_(t) for t in run(dev, U, I, B, M, 3, users=bad, check_ids=False))
    keep = np.ones(B, dtype=bool)
    keep[[2, 30]] = False
    np.testing.assert_array_equal(n[keep], good["neg"][keep])
    np.testing.assert_array_equal(col[keep], good["pick_col"][keep])
    assert (col[~keep] == 0).all() and (score[~keep] == 0).all() and (p[~keep] == 0).all() and (n[~keep] == cand[~keep, 0]).all()


# ---- 6. the device counter, a replayed graph -----------------------------------------------------------------------------------------------------
def test_the_device_counter_and_a_replayed_graph(dev):
    from pda_amd import ops
    U, I = dr.gaussian_tables(64)
    pop = dr.pop_matrix()
    B, M, topn = 37, 8, 3
    Ut, It, ip, ix, sl, pt, pm = to(dev, U, I, INDPTR, INDICES, SLOTS, POOL, pop)
    kw = dict(n_cands=M, topn=topn, head=dr.HEAD_POP, seed=SEED, neg_range=(0, dr.NI), user_pool=pt, n_pool=dr.NU, train_slots=sl, pop_matrix=pm)
    direct = [ops.dns_sample(Ut, It, ip, ix, B, step=s, want_cands=True, **kw) for s in range(1, 7)]

    def buffers():
        i32, f32 = (lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)), (lambda *s: torch.zeros(s, dtype=torch.float32, device=dev))
        return (i32(B), i32(B), i32(B), f32(B), f32(B)), (i32(B, M), f32(B, M), i32(B))

    def same(out, cands, want):
        return all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out + cands, want))

    ctr = torch.tensor([1, -1], dtype=torch.int64, device=dev)
    out, cands = buffers()
    for s in (1, 2, 3):
        ops.dns_sample_into(out, Ut, It, ip, ix, step_dev=ctr, parity=(s - 1) & 1, cands=cands, **kw)
        assert same(out, cands, direct[s - 1]), s
        assert ctr[s & 1].item() == s + 1
    ops.dns_sample_into(out, Ut, It, ip, ix, step_dev=ctr[1:], cands=cands, **kw)           # read only: slot 1 holds 4
    assert same(out, cands, direct[3]) and ctr.tolist() == [3, 4]

    # a graph of two calls (an even number: the counter is back in slot 0 behind them), replayed three times: steps 1 .. 6
    ctr.copy_(torch.tensor([1, -1], dtype=torch.int64))
    (oa, ca), (ob, cb) = buffers(), buffers()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ops.dns_sample_into(oa, Ut, It, ip, ix, step_dev=ctr, parity=0, cands=ca, **kw)
            ops.dns_sample_into(ob, Ut, It, ip, ix, step_dev=ctr, parity=1, cands=cb, **kw)
    torch.cuda.synchronize()
    assert ctr.tolist() == [1, -1]                                    # capturing runs nothing
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert same(oa, ca, direct[2 * k]) and same(ob, cb, direct[2 * k + 1]), k
        assert ctr[0].item() == 2 * k + 3


# ---- 7. determinism --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, M", [(32, 256), (256, 5)])
def test_two_calls_are_bit_equal(dev, d, M):
    U, I = dr.gaussian_tables(d)
    pop = dr.pop_matrix()
    a = run(dev, U, I, 600, M, min(M, 3), head=dr.HEAD_POP, pop=pop, slots=SLOTS)
    b = run(dev, U, I, 600, M, min(M, 3), head=dr.HEAD_POP, pop=pop, slots=SLOTS)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---- 8. through the sampler ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from pda_amd import synthetic
    root = tmp_path_factory.mktemp("dns_data")
    synthetic.write_dataset(str(root / "toy"), n_users=400, n_items=300, mean_hist=20)
    return str(root) + "/"


def _argv(toy, save, train, extra=()):
    return ["--data_path", toy, "--dataset", "toy", "--train", train, "--test", train, "--epoch", "2", "--log_interval", "1",
            "--batch_size", "256", "--lr", "1e-2", "--regs", "1e-2", "--valid_set", "valid", "--pop_exp", "0.22",
            "--save_dir", save, "--Ks", "[20,50]", "--save_flag", "0", "--saveID", "t", "--cuda", "0", "--eval_block", "128"] + list(extra)


def written_bytes(u, p, n):
    """The bytes of a triplet plan that the plan kernel writes: where two plans laid over different fillings agree."""
    from pda_amd import ops
    nb = ops.triplet_plan_bytes(u.numel())
    a = ops.triplet_plan(u, p, n, out=torch.zeros((1, nb), dtype=torch.uint8, device=u.device))[0]
    b = ops.triplet_plan(u, p, n, out=torch.full((1, nb), 255, dtype=torch.uint8, device=u.device))[0]
    return a, a == b


@pytest.mark.parametrize("config", ["with_pop", "with_plan"])
def test_the_device_sampler_is_the_call_on_the_tables_as_they_stood(dev, toy, tmp_path, config):
    from pda_amd import ops
    from pda_amd import train_new_api as t
    from pda_amd.sampler import DeviceSampler
    with_pop = config == "with_pop"
    t.configure(_argv(toy, str(tmp_path) + "/", "s_condition" if with_pop else "normal"))
    a, data = t.args, t.data
    if with_pop:
        data.add_expo_popularity(np.power(t.get_popularity_from_load(t.load_popularity(a)), a.pop_exp))
    M, topn, d, B = 16, 2, 64, data.batch_size
    s = DeviceSampler(data, dev, with_pop, mode="dns", n_cands=M, topn=topn)
    with pytest.raises(ValueError, match="set_tables"):
        s.batch()
    s.step = 0
    s.with_plan = not with_pop
    assert s.distinct_users == (B <= s.pool.numel())
    gen = torch.Generator(device=dev).manual_seed(3)
    tables = {"U": torch.randn(data.n_users, d, device=dev, generator=gen), "I": torch.randn(data.n_items, d, device=dev, generator=gen)}
    s.set_tables(lambda: (tables["U"], tables["I"]))
    negs = []
    for step in (1, 2, 3):
        got = s.batch()
        want = ops.dns_sample(tables["U"], tables["I"], s.indptr, s.indices, B, n_cands=M, topn=topn, head=ops.HEAD_POP if with_pop else ops.HEAD_RAW,
                              seed=s.seed, step=step, neg_range=(0, data.n_items), user_pool=s.pool, n_pool=s.pool.numel(),
                              train_slots=s.slots if with_pop else None, pop_matrix=s.pop)
        assert len(got) == (5 if with_pop else 3)
        for g, w in zip(got, want):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32)), step
        if with_pop:
            assert s.plan is None
        else:
            plan, written = written_bytes(*got[:3])
            assert written.float().mean() > 0.5 and torch.equal(s.plan[written], plan[written])
        negs.append(got[2].clone())
        tables["U"] = tables["U"] + 0.5 * torch.randn(data.n_users, d, device=dev, generator=gen)      # the tables move: new tensors, new values
        tables["I"].add_(0.5 * torch.randn(data.n_items, d, device=dev, generator=gen))
    uni = DeviceSampler(data, dev, with_pop, ahead=1)
    assert not torch.equal(negs[0], uni.batch()[2])                   # (M = 16: not the uniform sampler's negatives)


# ---- 9. through the CLI ----------------------------------------------------------------------------------------------------------------------------
def _cli(toy, save, train, extra):
    r = subprocess.run([sys.executable, "-m", "pda_amd.train_new_api"] + _argv(toy, save, train, extra), cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _figures(out):
    """The lines of a run that carry losses and metrics, the wall-clock seconds of the epoch lines taken out."""
    keep = [re.sub(r"^(Epoch \d+) \[[^\]]*\]", r"\1", ln) for ln in out.splitlines() if ln.startswith("Epoch ") or ln.startswith("||---")]
    return [ln for ln in keep if "time:" not in ln]


@pytest.mark.parametrize("train", ["normal", "s_condition"])
def test_cli_one_candidate_is_the_uniform_run_and_sixteen_train(dev, toy, tmp_path, train):
    base = _figures(_cli(toy, str(tmp_path / "a") + "/", train, ("--deterministic", "1")))
    one = _figures(_cli(toy, str(tmp_path / "b") + "/", train, ("--deterministic", "1", "--neg_sampler", "dns", "--dns_candidates", "1")))
    assert len([ln for ln in base if ln.startswith("Epoch ")]) == 2 and any("recall=[" in ln for ln in base)
    assert one == base
    out = _cli(toy, str(tmp_path / "c") + "/", train, ("--neg_sampler", "dns", "--dns_candidates", "16"))
    losses = [[float(x) for x in m.groups()] for m in re.finditer(r"Epoch \d+ \[[^\]]*\]: train==\[([-\d.]+)=([-\d.]+) \+ ([-\d.]+)\]", out)]
    assert len(losses) == 2 and np.isfinite(losses).all(), out[-2000:]
    assert "recall=[" in out and _figures(out) != base                # hard negatives: another run
