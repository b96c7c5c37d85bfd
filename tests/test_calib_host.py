"""CPU suite for calibrated popularity (`python -m pda_amd.calib`, include/pda_hip_calib.h): the binding against the header, the entry points'
argument checks (all before any HIP call), the popularity groups, the reference of tests/calib_ref.py itself (counts by hand, the grid, the
fragile flag and its margin, invariants), the merge property the kernel rests on (the naive selection equals the G-way merge of the group
sub-lists), UPD, the flags and the driver's refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import calib_cases as cc
from calib_ref import (MARGIN, calib_ref, divergences, list_counts_ref, merge_row, profile_ref, quantise, valid_prefix)
from test_abi import declared_in

ERR_ARG = -1
f32 = np.float32
NAMES = ["pda_calib_list_counts", "pda_calib_profile", "pda_calib_rerank"]


# ---- the binding ---------------------------------------------------------------------------------------------------------------------------
def test_binding_equals_the_header():
    from pda_amd import _lib
    assert declared_in("pda_hip_calib.h") == sorted(_lib.CALIB_SIGNATURES) == NAMES
    for name in dir(_lib):
        if name.endswith("SIGNATURES") and name != "CALIB_SIGNATURES":
            assert not set(NAMES) & set(getattr(_lib, name)), name
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    for h in sorted(os.listdir(inc)):
        if h != "pda_hip_calib.h":
            assert not set(NAMES) & set(declared_in(h)), h                     # declared once
    lib = _lib.load()
    for name in NAMES:
        assert getattr(lib, name).argtypes == _lib.CALIB_SIGNATURES[name][1] and getattr(lib, name).restype is C.c_int
    text = open(os.path.join(inc, "pda_hip_calib.h")).read()
    consts = (("MAX_G", _lib.CALIB_MAX_G), ("MAX_K", _lib.CALIB_MAX_K), ("MAX_N", _lib.CALIB_MAX_N), ("MAX_KS", _lib.CALIB_MAX_KS),
              ("JS", _lib.CALIB_JS), ("KL", _lib.CALIB_KL))
    for name, value in consts:
        assert "#define PDA_CALIB_%s %d " % (name, value) in text or "#define PDA_CALIB_%s %d\n" % (name, value) in text
    assert tuple(v for _, v in consts) == (8, 64, 1024, 8, 0, 1)
    # the signatures, argument by argument, from the header's own text
    code = text[text.index("#define PDA_CALIB_KL"):]
    import re
    code = re.sub(r"/\*.*?\*/", "", code, flags=re.S)
    for name in NAMES:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).split(",")
        kinds = [C.c_void_p if "*" in a else C.c_double if "double" in a else C.c_int for a in args]
        assert kinds == _lib.CALIB_SIGNATURES[name][1], name


def test_entry_points_check_arguments_without_gpu():
    from pda_amd import _lib
    lib = _lib.load()
    keep = C.create_string_buffer(4096)
    b, null = C.c_void_p(C.addressof(keep)), C.c_void_p(None)
    ks = (C.c_int32 * 2)(20, 50)

    def rerank(idx=b, val=b, rows=4, N=100, prof=b, grp=b, items=500, G=3, lam=0.5, variant=0, alpha=0.01, K=50, oi=b, ov=b, od=b):
        return lib.pda_calib_rerank(idx, val, rows, N, prof, grp, items, G, lam, variant, alpha, K, oi, ov, od, null)

    for name in ("idx", "val", "prof", "grp", "oi", "ov"):
        assert rerank(**{name: null}) == ERR_ARG, name
    assert rerank(rows=0) == ERR_ARG and rerank(rows=-3) == ERR_ARG
    assert rerank(items=0) == ERR_ARG
    assert rerank(N=0) == ERR_ARG and rerank(N=1025) == ERR_ARG
    assert rerank(K=0) == ERR_ARG and rerank(K=65, N=1000) == ERR_ARG and rerank(K=51, N=50) == ERR_ARG and rerank(K=2, N=1) == ERR_ARG
    assert rerank(G=1) == ERR_ARG and rerank(G=9) == ERR_ARG and rerank(G=0) == ERR_ARG and rerank(G=-2) == ERR_ARG
    assert rerank(lam=-0.001) == ERR_ARG and rerank(lam=1.001) == ERR_ARG and rerank(lam=float("nan")) == ERR_ARG and rerank(lam=float("inf")) == ERR_ARG
    assert rerank(variant=2) == ERR_ARG and rerank(variant=-1) == ERR_ARG
    for alpha in (0.0, 1.0, -0.5, 1.5, float("nan")):
        assert rerank(variant=1, alpha=alpha) == ERR_ARG, alpha

    def profile(users=b, indptr=b, indices=b, mode=0, rows=4, grp=b, items=500, G=3, prof=b):
        return lib.pda_calib_profile(users, indptr, indices, mode, rows, grp, items, G, prof, null)

    assert profile(grp=null) == ERR_ARG and profile(prof=null) == ERR_ARG
    assert profile(rows=0) == ERR_ARG and profile(items=0) == ERR_ARG and profile(G=1) == ERR_ARG and profile(G=9) == ERR_ARG
    assert profile(indices=null) == ERR_ARG and profile(mode=2) == ERR_ARG and profile(mode=-1) == ERR_ARG
    assert profile(mode=1, users=null) == ERR_ARG                                # a history by user id without the user ids

    def counts(idx=b, rows=4, K=50, grp=b, items=500, G=3, Ks=ks, nK=2, cnt=b):
        return lib.pda_calib_list_counts(idx, rows, K, grp, items, G, Ks, nK, cnt, null)

    for name in ("idx", "grp", "cnt"):
        assert counts(**{name: null}) == ERR_ARG, name
    assert counts(Ks=None) == ERR_ARG
    assert counts(rows=0) == ERR_ARG and counts(items=0) == ERR_ARG and counts(G=1) == ERR_ARG and counts(G=9) == ERR_ARG
    assert counts(K=0) == ERR_ARG and counts(K=1025) == ERR_ARG and counts(K=49) == ERR_ARG          # a cut-off behind the last column
    assert counts(nK=0) == ERR_ARG and counts(nK=9) == ERR_ARG
    assert counts(Ks=(C.c_int32 * 2)(50, 20)) == ERR_ARG and counts(Ks=(C.c_int32 * 2)(20, 20)) == ERR_ARG and counts(Ks=(C.c_int32 * 2)(0, 20)) == ERR_ARG
    del keep


def test_ops_refuses_bad_arguments_before_the_library():
    import torch
    from pda_amd import ops
    with pytest.raises((ValueError, TypeError)):
        ops.calib_rerank(torch.zeros((4, 100), dtype=torch.int32), torch.zeros((4, 100)), torch.zeros((4, 3), dtype=torch.int32),
                         torch.zeros(500, dtype=torch.uint8), 3, 0.5)           # host memory
    with pytest.raises((ValueError, TypeError)):
        ops.calib_profile(torch.zeros(500, dtype=torch.uint8), 3, 4)
    with pytest.raises((ValueError, TypeError)):
        ops.calib_list_counts(torch.zeros((4, 50), dtype=torch.int32), torch.zeros(500, dtype=torch.uint8), 3, [20, 50])
    assert (ops.CALIB_MAX_G, ops.CALIB_MAX_K, ops.CALIB_MAX_N, ops.CALIB_MAX_KS) == (8, 64, 1024, 8) and ops.CALIB_DIVERGENCES == {"js": 0, "kl": 1}
    assert ops.calib_ks([20, 50], 50) == (20, 50)
    for bad in ([], [0, 5], [5, 5], [50, 20], [20, 51], list(range(1, 10))):
        with pytest.raises(ValueError):
            ops.calib_ks(bad, 50)


# ---- the popularity groups ------------------------------------------------------------------------------------------------------------------
def test_cut_groups_with_one_cut_is_the_short_head():
    from pda_amd.calib import cut_groups
    from pda_amd.xquad import head_items
    rng = np.random.default_rng(7)
    for trial in range(30):
        counts = cc.long_tail_counts(rng, 400) if trial % 2 else rng.integers(0, 6, 50)
        for share in (0.2, 0.5, 0.8, 0.999, 1e-9, float(rng.random())):
            g = cut_groups(counts, [share])
            assert g.dtype == np.uint8 and set(g.tolist()) <= {0, 1}
            np.testing.assert_array_equal(g == 0, head_items(counts, share) == 1)
    assert cut_groups([2, 5, 3], [0.5]).tolist() == [1, 0, 1]                   # 5 of 10 reached exactly by the first item


def test_cut_groups_by_hand_empty_groups_and_errors():
    from pda_amd.calib import cut_groups, parse_cuts
    c = [3, 3, 5, 1, 0, 2, 1]                                                   # order: 2 | 0 1 | 5 | 3 6 | 4; cum_before 0 5 8 11 13 14 15 of 15
    assert cut_groups(c, [0.2, 0.8]).tolist() == [1, 1, 0, 2, 2, 1, 2]         # cuts at 3 and 12
    assert cut_groups(c, "[0.2,0.8]").tolist() == [1, 1, 0, 2, 2, 1, 2]
    assert cut_groups(c, [0.1, 0.2, 0.3]).tolist() == [3, 3, 0, 3, 3, 3, 3]    # cuts at 1.5, 3, 4.5: groups 1 and 2 are empty
    assert cut_groups([10, 0, 0], [0.5]).tolist() == [0, 1, 1]                 # items without a train entry: the last group
    seven = [i / 8 for i in range(1, 8)]
    assert sorted(set(cut_groups(np.ones(64, np.int64), seven).tolist())) == list(range(8))
    with pytest.raises(ValueError, match="without interactions"):
        cut_groups([0, 0, 0], [0.5])
    with pytest.raises(ValueError):
        cut_groups([1, -1], [0.5])
    for bad in ([], [0.0, 0.5], [0.5, 1.0], [0.5, 0.5], [0.8, 0.2], [i / 9 for i in range(1, 9)], "0.5", "[a]", [float("nan")]):
        with pytest.raises(ValueError):
            parse_cuts(bad)
    assert parse_cuts("[0.2,0.8]") == (0.2, 0.8) and parse_cuts((0.5,)) == (0.5,)


# ---- the reference itself: counts ------------------------------------------------------------------------------------------------------------
def test_profile_and_list_counts_by_hand():
    item_group = np.array([0, 1, 2, 0, 1, 3, 255, 2], np.uint8)                # items 5 and 6 have no group when G = 3
    rows = [[0, 0, 3, 1, 7, 7, 7], [5, 6, 6], [], [-1, 8, 100, 2], [4, 5, 1, 0]]
    assert profile_ref(rows, item_group, 3).tolist() == [[2, 1, 1], [0, 0, 0], [0, 0, 0], [0, 0, 1], [1, 2, 0]]
    assert profile_ref(rows, item_group, 4).tolist() == [[2, 1, 1, 0], [0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 1, 0], [1, 2, 0, 1]]
    idx = np.array([[0, 3, 1, 5, 2, -1], [6, 6, 8, -1, -1, -1], [7, 2, 2, 0, 4, 1]], np.int32)
    got = list_counts_ref(idx, item_group, 3, [1, 4, 6])
    assert got.tolist() == [[[1, 0, 0], [2, 1, 0], [2, 1, 1]], [[0, 0, 0]] * 3, [[0, 0, 1], [1, 0, 3], [1, 2, 3]]]
    assert valid_prefix(idx, np.zeros(idx.shape, f32), item_group, 3).tolist() == [3, 0, 6]
    assert valid_prefix(idx, np.zeros(idx.shape, f32), item_group, 4).tolist() == [5, 0, 6]


# ---- the reference itself: the grid and the fragile flag ----------------------------------------------------------------------------------
def test_quantisation_zero_clamping_ties_and_a_flagged_boundary():
    d32, fr = quantise(np.array([0.0, -0.0, -1e-3, 1e-9, 2.0 ** -20, 7.9, 8.0, 9.5, 1e30]))
    assert d32.tolist() == [0.0, 0.0, 0.0, 0.0, 2.0 ** -20, float(f32(round(7.9 * 2 ** 20) * 2.0 ** -20)), 8.0, 8.0, 8.0]
    assert not np.signbit(d32).any() and d32.dtype == np.float32 and not fr.any()
    # halfway between two grid points: ties go to even, and the value is fragile
    d32, fr = quantise(np.array([0.5, 1.5, 2.5, 1000.5]) * 2.0 ** -20)
    assert (d32 * 2.0 ** 20).tolist() == [0.0, 2.0, 2.0, 1000.0] and fr.all()
    # a constructed boundary value: 2^-41 beside the boundary is flagged, 2^-39 is not
    D = 12345.5 * 2.0 ** -20
    for delta, flagged in ((2.0 ** -41, True), (-2.0 ** -41, True), (2.0 ** -39, False), (-2.0 ** -39, False)):
        assert quantise(np.array([D + delta]))[1][0] == flagged, delta
    assert MARGIN == 2.0 ** -20                                                # of D 2^20: 2^-40 of D
    # the selection carries the flag of the row that met it: a profile and a list that put D_c exactly on a boundary cannot be built by hand,
    # so the flag's way out of calib_ref is checked through a patched quantise
    import calib_ref as ref
    real = ref.quantise
    try:
        ref.quantise = lambda D: (real(D)[0], np.broadcast_to((np.arange(D.shape[0]) == 1)[:, None], D.shape))
        idx, val = cc.candidates(np.random.default_rng(0), 3, 10)
        out = ref.calib_ref(idx, val, np.ones((3, 2), np.int64), np.zeros(cc.N_ITEMS, np.uint8), 2, 0.5, 4)
    finally:
        ref.quantise = real
    assert out[3].tolist() == [False, True, False]


def test_float64_divergences_lie_within_2_pow_minus_44_of_longdouble():
    """The margin of the fragile flag: a divergence within 2^-40 of a grid boundary.  The float64 values of the reference differ from the same
    expressions in np.longdouble by at most 2^-44 over every case of the generator (every state n the selection of that case runs through),
    which leaves a factor of 16 for what the device's log / log2, a couple of ulps, adds on top.  (Where long double is no wider than double
    the comparison is vacuous and the margin rests on the math library's error bound alone.)"""
    worst = 0.0
    for c in cc.CASES:
        d = cc.case(*c)
        gb = np.minimum(np.asarray(d["item_group"])[np.clip(d["want"][0], 0, None)], d["G"] - 1)
        n = np.zeros((cc.ROWS, d["G"]), np.int64)
        for t in range(d["K"]):
            D64 = divergences(d["prof"], n, t, d["div"], cc.ALPHA)
            DL = divergences(d["prof"], n, t, d["div"], cc.ALPHA, dtype=np.longdouble)
            worst = max(worst, float(np.abs(DL - D64.astype(np.longdouble)).max()))
            picked = d["want"][0][:, t] >= 0
            n[np.nonzero(picked)[0], gb[picked, t]] += 1
    print("largest |float64 - longdouble| over the cases: %.3g (2^-44 = %.3g)" % (worst, 2.0 ** -44))
    assert worst <= 2.0 ** -44


def test_the_reference_flags_at_most_two_rows_of_a_case():
    flagged = [int(cc.case(*c)["fragile"].sum()) for c in cc.CASES]
    print("fragile rows over %d cases: %d, at most %d in one" % (len(cc.CASES), sum(flagged), max(flagged)))
    assert max(flagged) <= cc.MAX_FRAGILE
    changed = sum(int((cc.case(*c)["want"][0] != cc.case(*c)["idx"][:, :c[1]]).any(axis=1).sum()) for c in cc.CASES)
    assert changed > len(cc.CASES) * cc.ROWS // 3, "the cases should change the order of many rows"
    for c in cc.CASES:
        if c[4] > 0 and c[0] >= 50 and c[1] >= 20:
            assert (cc.case(*c)["want"][0] != cc.case(*c)["idx"][:, :c[1]]).any(), c


# ---- the merge property --------------------------------------------------------------------------------------------------------------------
def _random_row(rng, N, n_items, G):
    kind = rng.integers(0, 7)
    val = np.sort(rng.standard_normal(N).astype(f32))[::-1].copy()
    if kind == 1:
        val = (np.round(val * 2) / 2).astype(f32)                             # ties
    elif kind == 2:
        val[:] = f32(0.25)                                                    # rng = 0
    idx = rng.permutation(n_items)[:N].astype(np.int32)
    item_group = rng.choice(G, n_items, p=rng.dirichlet(np.ones(G) * 0.7)).astype(np.uint8)
    if kind == 3:
        nv = int(rng.integers(0, N + 1))
        idx[nv:] = -1
        val[nv:] = -np.inf
    elif kind == 4 and N > 1:
        val[int(rng.integers(0, N))] = np.nan
    elif kind == 5:
        item_group[idx[int(rng.integers(0, N))]] = G + int(rng.integers(0, 200))      # an item of no group ends the prefix
    prof = rng.integers(0, 12, G) * (rng.random(G) < 0.7)
    return idx, val, item_group, prof


def test_naive_selection_equals_the_merge_of_the_group_lists():
    rng = np.random.default_rng(2018)
    n_items, changed = 400, 0
    for case in range(400):
        N = int(rng.choice([1, 2, 3, 17, 50, 64, 65, 130, 257]))
        K = int(min(N, rng.choice([1, 5, 20, 64])))
        G = int(rng.choice([2, 3, 5, 8]))
        lam = float(rng.choice([0.0, 0.1, 0.5, 0.9, 1.0]))
        div = cc.DIVS[case & 1]
        idx, val, item_group, prof = _random_row(rng, N, n_items, G)
        wi, wv, wd, _ = calib_ref(idx[None], val[None], prof[None], item_group, G, lam, K, div, 0.01)
        mi, mv, md = merge_row(idx, val, prof, item_group, G, lam, K, div, 0.01)
        np.testing.assert_array_equal(mi, wi[0])
        np.testing.assert_array_equal(mv.view(np.int32), wv[0].view(np.int32))
        np.testing.assert_array_equal(md.view(np.int32), wd[0].view(np.int32))
        nv = int((wi[0] >= 0).sum())
        changed += int((wi[0, :nv] != idx[:nv]).any())
    assert changed >= 100, "the rows should include many whose order the calibration changes"


# ---- invariants ----------------------------------------------------------------------------------------------------------------------------
def test_reference_by_hand():
    """Four candidates of groups 0 0 1 1, values 3 2 1 0, a profile half and half, lambda 0.6, JS: after the first pick of group 0 a second
    one costs D = JS((.5, .5), (1, 0)) = 0.311, one of group 1 costs 0: the third candidate (0.4 / 3) overtakes the second (0.8 / 3 - 0.6 D)."""
    item_group = np.array([0, 0, 1, 1], np.uint8)
    idx, val = np.array([[0, 1, 2, 3]], np.int32), np.array([[3, 2, 1, 0]], f32)
    wi, wv, wd, fr = calib_ref(idx, val, [[3, 3]], item_group, 2, 0.6, 4, "js")
    assert wi.tolist() == [[0, 2, 1, 3]] and not fr.any()
    L, W = f32(0.6), f32(1.0 - 0.6)
    js = 0.5 * (0.5 * np.log2(0.5 / 0.75) + 1.0 * np.log2(1.0 / 0.75) + 0.5 * np.log2(0.5 / 0.25))      # JS((.5, .5), (1, 0)) = 0.3113
    d1 = f32(np.rint(js * 2 ** 20) * 2.0 ** -20)
    js3 = 0.5 * (0.5 * np.log2(0.5 / (7 / 12)) + (2 / 3) * np.log2((2 / 3) / (7 / 12)) + 0.5 * np.log2(0.5 / (5 / 12)) + (1 / 3) * np.log2((1 / 3) / (5 / 12)))
    d3 = f32(np.rint(js3 * 2 ** 20) * 2.0 ** -20)
    assert wd[0].tolist() == [float(d1), 0.0, float(d3), 0.0]
    p = (val[0] / f32(3)).astype(f32)
    want = [f32(W * p[0]) - f32(L * d1), f32(W * p[2]) - f32(0), f32(W * p[1]) - f32(L * d3), f32(0)]
    np.testing.assert_array_equal(wv[0], np.array(want, f32))
    # a short row: -1, -inf and -inf behind the valid prefix, which ends at the first invalid position whatever follows it
    wi, wv, wd, _ = calib_ref(np.array([[0, 9, 2, 3]], np.int32), val, [[3, 3]], item_group, 2, 0.5, 3, "kl")
    assert wi.tolist() == [[0, -1, -1]] and np.isneginf(wv[0, 1:]).all() and np.isneginf(wd[0, 1:]).all() and np.isfinite(wd[0, 0])


def test_lambda_zero_and_an_empty_profile_keep_the_candidates_order():
    rng = np.random.default_rng(3)
    for G in cc.GROUPS:
        counts = cc.long_tail_counts(rng)
        item_group = cc.groups_of(counts, G)
        idx, val = cc.candidates(rng, 20, 200)
        prof = profile_ref(cc.histories(rng, 20, counts), item_group, G)
        for div in cc.DIVS:
            wi, wv, wd, _ = calib_ref(idx, val, prof, item_group, G, 0.0, 50, div)
            np.testing.assert_array_equal(wi, idx[:, :50])
            wi, wv, wd, fr = calib_ref(idx, val, np.zeros_like(prof), item_group, G, 0.7, 50, div)
            np.testing.assert_array_equal(wi, idx[:, :50])
            assert not wd.any() and not fr.any()


def test_lambda_one_with_equal_values_picks_by_divergence_then_position():
    rng = np.random.default_rng(4)
    counts = cc.long_tail_counts(rng)
    item_group = cc.groups_of(counts, 3)
    idx, val = cc.candidates(rng, 30, 120)
    val[:] = f32(2.5)
    prof = profile_ref(cc.histories(rng, 30, counts), item_group, 3)
    for div in cc.DIVS:
        wi, wv, wd, _ = calib_ref(idx, val, prof, item_group, 3, 1.0, 40, div)
        for r in range(30):
            avail, n = list(range(120)), np.zeros((1, 3), np.int64)
            for t in range(40):
                d32 = quantise(divergences(prof[r:r + 1], n, t, div))[0][0]
                best = min(avail, key=lambda v: (d32[item_group[idx[r, v]]], v))      # the smallest divergence, then the smallest position
                assert wi[r, t] == idx[r, best] and wd[r, t] == d32[item_group[idx[r, best]]] and wv[r, t] == -d32[item_group[idx[r, best]]]
                avail.remove(best)
                n[0, item_group[idx[r, best]]] += 1


def test_js_reference_lies_in_0_1_and_vanishes_on_equal_mixes():
    rng = np.random.default_rng(5)
    for G in (2, 3, 8):
        prof = rng.integers(0, 30, (200, G)) * (rng.random((200, G)) < 0.6)
        n = rng.integers(0, 20, (200, G)) * (rng.random((200, G)) < 0.6)
        t = 63
        D = divergences(prof, n, t, "js")
        assert (D >= -1e-15).all() and (D <= 1.0 + 1e-15).all()
        assert (divergences(prof, n, t, "kl") >= -1e-12).all()
    # the list (1, 1 + 1) / 3 against the profile (1, 2) / 3: the divergence of adding group 1 is 0
    D = divergences(np.array([[1, 2]]), np.array([[1, 1]]), 2, "js")
    assert D[0, 1] == 0.0 and D[0, 0] > 0.0
    assert abs(divergences(np.array([[1, 2]]), np.array([[1, 1]]), 2, "kl", 0.01)[0, 1]) < 1e-15


# ---- UPD -----------------------------------------------------------------------------------------------------------------------------------
def test_upd_by_hand_and_rows_without_a_history_are_left_out():
    from pda_amd.calib import upd
    prof = np.array([[1, 1], [2, 0], [0, 0], [3, 1]])
    cnt = np.array([[[1, 0], [1, 1]], [[1, 0], [2, 0]], [[1, 0], [1, 1]], [[0, 0], [0, 2]]])
    got, rows = upd(prof, cnt)
    js_half_one = 0.5 * (0.5 * np.log2(0.5 / 0.75) + 1.0 * np.log2(1.0 / 0.75) + 0.5 * np.log2(0.5 / 0.25))
    p, q = np.array([0.75, 0.25]), np.array([0.0, 1.0])
    m = 0.5 * (p + q)
    js_last = 0.5 * (p[0] * np.log2(p[0] / m[0]) + p[1] * np.log2(p[1] / m[1]) + q[1] * np.log2(q[1] / m[1]))
    assert rows.tolist() == [2, 3] and rows.dtype == np.int64 and got.dtype == np.float64      # row 2: no history; row 3: an empty list at the first cut-off
    np.testing.assert_allclose(got, [(js_half_one + 0.0) / 2, (0.0 + 0.0 + js_last) / 3], rtol=0, atol=1e-15)
    got, rows = upd(np.zeros((3, 2), int), cnt[:3])
    assert got.tolist() == [0.0, 0.0] and rows.tolist() == [0, 0]
    with pytest.raises(ValueError):
        upd(prof, cnt[:, :, :1])


def test_calibration_lowers_upd_on_the_synthetic_candidates():
    """lambda = 0.9 over 1 000 synthetic candidates: the reference's lists deviate less from the users' popularity mix than the first K."""
    from pda_amd.calib import upd
    rng = np.random.default_rng(9)
    counts = cc.long_tail_counts(rng)
    item_group = cc.groups_of(counts, 3)
    idx, val = cc.candidates(rng, 40, 1000, ties=False)
    prof = profile_ref(cc.histories(rng, 40, counts), item_group, 3)
    first = upd(prof, list_counts_ref(idx[:, :50], item_group, 3, [20, 50]))[0]
    for div in cc.DIVS:
        wi = calib_ref(idx, val, prof, item_group, 3, 0.9, 50, div)[0]
        cp = upd(prof, list_counts_ref(wi, item_group, 3, [20, 50]))[0]
        print(div, "upd of the first K", first, "calibrated", cp)
        assert (cp < first).all()


# ---- flags and the driver ------------------------------------------------------------------------------------------------------------------
def test_flags_default_to_the_documented_values():
    from pda_amd.parse import parse_args, reference_flag_names
    a = parse_args([])
    assert (a.cp_lambda, a.cp_candidates, a.cp_cuts, a.cp_div, a.cp_alpha) == (0.5, 1000, "[0.2,0.8]", "js", 0.01)
    a = parse_args(["--cp_lambda", "0.25", "--cp_candidates", "300", "--cp_cuts", "[0.5]", "--cp_div", "kl", "--cp_alpha", "0.1"])
    assert (a.cp_lambda, a.cp_candidates, a.cp_cuts, a.cp_div, a.cp_alpha) == (0.25, 300, "[0.5]", "kl", 0.1)
    for name in ("cp_lambda", "cp_candidates", "cp_cuts", "cp_div", "cp_alpha"):
        assert name not in reference_flag_names()


def _toy(tmp_path):
    from pda_amd import synthetic
    toy = str(tmp_path / "data") + "/"
    synthetic.write_dataset(toy + "toy", n_users=60, n_items=40, mean_hist=6)
    return toy


def test_cli_refusals_without_a_device(tmp_path):
    from pda_amd import calib
    toy = _toy(tmp_path)
    save = str(tmp_path / "save") + "/"
    base = ["--data_path", toy, "--dataset", "toy", "--save_dir", save, "--Ks", "[20,50]", "--regs", "0.01", "--lr", "0.002", "--saveID", "x",
            "--pop_exp", "0.22"]
    with pytest.raises(NotImplementedError, match=r"^Not implement this training method\.\.\.\.\.$"):
        calib.main(base + ["--train", "s_condition"])
    with pytest.raises(NotImplementedError):
        calib.main(base + ["--train", "normal", "--model", "lightgcn"])
    with pytest.raises(ValueError, match="cp_lambda"):
        calib.main(base + ["--train", "normal", "--cp_lambda", "1.5"])
    with pytest.raises(ValueError, match="cp_candidates"):
        calib.main(base + ["--train", "normal", "--cp_candidates", "49"])
    with pytest.raises(ValueError, match="cp_candidates"):
        calib.main(base + ["--train", "normal", "--cp_candidates", "1025"])
    with pytest.raises(ValueError, match="cp_cuts"):
        calib.main(base + ["--train", "normal", "--cp_cuts", "[0.8,0.2]"])
    with pytest.raises(ValueError, match="cp_cuts"):
        calib.main(base + ["--train", "normal", "--cp_cuts", "[0.1,0.2,0.3,0.4,0.5,0.6,0.7,0.8]"])
    with pytest.raises(ValueError, match="cp_div"):
        calib.main(base + ["--train", "normal", "--cp_div", "hellinger"])
    with pytest.raises(ValueError, match="cp_alpha"):
        calib.main(base + ["--train", "normal", "--cp_div", "kl", "--cp_alpha", "1.0"])
    with pytest.raises(ValueError, match="at most 64"):
        calib.main(base[:6] + ["--Ks", "[20,65]"] + base[8:] + ["--train", "normal"])
    with pytest.raises(NotImplementedError, match="rank_report"):
        calib.main(base + ["--train", "normal", "--rank_report", "1"])
    want = save + "mf_toy_checkpoint/wd_0.01_lr_0.002_a_0.001_xpop_exp-0.22_train_normal/best_ckpt.ckpt"
    with pytest.raises(FileNotFoundError) as e:
        calib.main(base + ["--train", "normal", "--bias_report", "1"])
    assert want in str(e.value)
    for train, suffix in (("dice", ""), ("ips", "ips"), ("ssm", "ssm"), ("ials", "ials"), ("pcc", "pcc"), ("dau", "dau")):
        with pytest.raises(FileNotFoundError) as e:
            calib.main(base + ["--train", train])
        assert "xpop_exp-0.22%s_train_%s/best_ckpt.ckpt" % (suffix, train) in str(e.value)
    assert not os.path.exists(save)


def test_calib_model_refuses_other_heads_item_subsets_and_shards():
    from pda_amd import calib

    class _Rec:
        n_items = 6

    class _Model:
        input_type, Recommender, device = "without_pop", _Rec(), "cpu"

    grp = np.array([0, 0, 1, 1, 2, 2], np.uint8)
    cp = calib.Calib_model(_Model(), 2, 0.5, 4, grp, 3)
    with pytest.raises(NotImplementedError, match="main_branch"):
        cp.recommend_device(np.arange(2), None, "pda_branch")
    with pytest.raises(NotImplementedError, match="full catalogue"):
        cp.recommend_device(np.arange(2), np.arange(3), "main_branch")
    sharded = _Model()
    sharded._shard = object()
    with pytest.raises(NotImplementedError, match="shard"):
        calib.Calib_model(sharded, 2, 0.5, 4, grp, 3)
    popular = _Model()
    popular.input_type = "with_pop"
    with pytest.raises(NotImplementedError):
        calib.Calib_model(popular, 2, 0.5, 4, grp, 3)
    for kw in (dict(lam=1.5), dict(div="x"), dict(alpha=0.0), dict(G=9), dict(topk=5), dict(n_candidates=7), dict(item_group=grp[:5])):
        a = dict(model=_Model(), topk=2, lam=0.5, n_candidates=4, item_group=grp, G=3, div="js", alpha=0.01)
        a.update(kw)
        with pytest.raises(ValueError):
            calib.Calib_model(**a)
