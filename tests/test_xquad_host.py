"""CPU suite for xQuAD (`python -m pda_amd.xquad`, include/pda_hip_xquad.h): the binding against the header, the entry point's argument
checks (all before any HIP call), the short head, the merge property the kernel rests on (the naive selection of tests/xquad_ref.py equals
the merge of the two category sub-lists), the search for the end of the valid prefix, the flags and the driver's refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from test_abi import declared_in
from xquad_ref import merge_row, prefix_end_search, xquad_ref

ERR_ARG = -1
f32 = np.float32


# ---- the binding ---------------------------------------------------------------------------------------------------------------------------
def test_binding_equals_the_header():
    from pda_amd import _lib
    assert declared_in("pda_hip_xquad.h") == sorted(_lib.XQUAD_SIGNATURES) == ["pda_xquad_rerank"]
    others = [_lib.SIGNATURES, _lib.TEMP_POP_SIGNATURES, _lib.PC_SIGNATURES, _lib.DET_SIGNATURES, _lib.DEEP_SIGNATURES]
    for d in others:
        assert not set(_lib.XQUAD_SIGNATURES) & set(d)
    for h in ("pda_hip.h", "pda_hip_experimental.h", "pda_hip_temp_pop.h", "pda_hip_pc.h", "pda_hip_det.h", "pda_hip_deep.h"):
        assert "pda_xquad_rerank" not in declared_in(h)
    lib = _lib.load()
    assert lib.pda_xquad_rerank.argtypes == _lib.XQUAD_SIGNATURES["pda_xquad_rerank"][1]
    assert lib.pda_xquad_rerank.restype is C.c_int
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pda_hip_xquad.h")).read()
    for name, value in (("MAX_K", _lib.XQUAD_MAX_K), ("MAX_N", _lib.XQUAD_MAX_N), ("BINARY", _lib.XQUAD_BINARY), ("SMOOTH", _lib.XQUAD_SMOOTH)):
        assert "#define PDA_XQUAD_%s %d " % (name, value) in text or "#define PDA_XQUAD_%s %d\n" % (name, value) in text
    assert (_lib.XQUAD_MAX_K, _lib.XQUAD_MAX_N, _lib.XQUAD_BINARY, _lib.XQUAD_SMOOTH) == (64, 1024, 0, 1)


def test_entry_point_checks_arguments_without_gpu():
    from pda_amd import _lib
    lib = _lib.load()
    keep = C.create_string_buffer(4096)
    b, null = C.c_void_p(C.addressof(keep)), C.c_void_p(None)

    def call(idx=b, val=b, rows=4, N=100, head=b, items=500, users=b, indptr=null, indices=null, mode=0, lam=0.5, variant=1, K=50, oi=b, ov=b):
        return lib.pda_xquad_rerank(idx, val, rows, N, head, items, users, indptr, indices, mode, lam, variant, K, oi, ov, null)

    for name in ("idx", "val", "head", "oi", "ov"):
        assert call(**{name: null}) == ERR_ARG, name
    assert call(rows=0) == ERR_ARG and call(rows=-3) == ERR_ARG
    assert call(items=0) == ERR_ARG
    assert call(N=0) == ERR_ARG and call(N=1025, K=50) == ERR_ARG
    assert call(K=0) == ERR_ARG and call(K=65, N=1000) == ERR_ARG and call(K=51, N=50) == ERR_ARG and call(K=2, N=1) == ERR_ARG
    assert call(lam=-0.001) == ERR_ARG and call(lam=1.001) == ERR_ARG and call(lam=float("nan")) == ERR_ARG and call(lam=float("inf")) == ERR_ARG
    assert call(variant=2) == ERR_ARG and call(variant=-1) == ERR_ARG
    assert call(indptr=b, indices=b, mode=1, users=null) == ERR_ARG           # a history by user id without the user ids
    assert call(indptr=b, indices=null) == ERR_ARG
    assert call(indptr=b, indices=b, mode=2) == ERR_ARG
    del keep


def test_ops_refuses_bad_arguments_before_the_library():
    import torch
    from pda_amd import ops
    with pytest.raises((ValueError, TypeError)):
        ops.xquad_rerank(torch.zeros((4, 100), dtype=torch.int32), torch.zeros((4, 100)), torch.zeros(500, dtype=torch.uint8), 0.5)   # host memory
    assert ops.XQUAD_MAX_K == 64 and ops.XQUAD_MAX_N == 1024 and ops.XQUAD_VARIANTS == {"binary": 0, "smooth": 1}


# ---- the short head ------------------------------------------------------------------------------------------------------------------------
def test_head_items_by_hand():
    from pda_amd.xquad import head_items
    # counts 5 3 3 2 1 1 0, total 15: 0.5 -> 7.5 needs 5 + 3 (item 1 before item 2: the tie goes to the lower id)
    c = [3, 3, 5, 1, 0, 2, 1]                                                  # order: 2 | 0 1 | 5 | 3 6 | 4
    assert head_items(c, 0.5).tolist() == [1, 0, 1, 0, 0, 0, 0] and head_items(c, 0.5).dtype == np.uint8
    assert head_items(c, 0.6).tolist() == [1, 1, 1, 0, 0, 0, 0]               # 9 reached by 5 + 3 + 3 = 11
    assert head_items(c, 0.2).tolist() == [0, 0, 1, 0, 0, 0, 0]               # 3 reached by the first item
    assert head_items([2, 5, 3], 0.5).tolist() == [0, 1, 0]                   # 5 of 10 reached exactly by the first item
    assert head_items([4, 3, 2, 1], 0.75).tolist() == [1, 1, 1, 0]
    assert head_items(c, 0.999).tolist() == [1, 1, 1, 1, 0, 1, 1]             # items without a train entry stay tail
    assert head_items([0, 0, 0], 0.8).tolist() == [0, 0, 0]                   # an empty train set has no head
    assert head_items([], 0.8).tolist() == []
    for share in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            head_items(c, share)


class _Data:
    n_items = 5
    train_item_list = {0: [1, 2], 2: [4, 4, 4], 4: [0]}


def test_train_counts_count_entries():
    from pda_amd.xquad import train_counts
    assert train_counts(_Data()).tolist() == [2, 0, 3, 0, 1]


def test_aplt_is_the_long_tail_share():
    import torch
    from pda_amd.xquad import aplt
    is_head = torch.tensor([1, 0, 0, 1, 0], dtype=torch.uint8)
    idx = torch.tensor([[0, 1, 2, 3], [4, 3, -1, -1], [3, 0, 1, 2]], dtype=torch.int32)
    got = aplt(idx, is_head, [1, 2, 4])
    np.testing.assert_array_equal(got, [(0 + 1 + 0) / 3.0, (1 + 1 + 0) / 2.0 / 3.0, (2 + 1 + 2) / 4.0 / 3.0])


# ---- the merge property --------------------------------------------------------------------------------------------------------------------
def _random_row(rng, N, n_items):
    kind = rng.integers(0, 6)
    val = np.sort(rng.standard_normal(N).astype(f32))[::-1].copy()
    if kind == 1:
        val = (np.round(val * 2) / 2).astype(f32)                             # ties
    elif kind == 2:
        val[:] = f32(0.25)                                                    # rng = 0
    idx = rng.permutation(n_items)[:N].astype(np.int32)
    nv = N
    if kind == 3:
        nv = int(rng.integers(0, N + 1))
        idx[nv:] = -1
        val[nv:] = -np.inf
    elif kind == 4 and N > 1:
        nv = int(rng.integers(0, N))
        val[nv] = np.nan
    hist = rng.integers(0, n_items, rng.integers(0, 30))
    return idx, val, hist


def test_naive_selection_equals_the_merge_of_two_category_lists():
    rng = np.random.default_rng(2019)
    n_items, changed = 400, 0
    for case in range(400):
        N = int(rng.choice([1, 2, 3, 17, 50, 64, 65, 130, 257]))
        K = int(min(N, rng.choice([1, 5, 20, 64])))
        lam = float(rng.choice([0.0, 0.1, 0.5, 0.9, 1.0]))
        variant = ("smooth", "binary")[case & 1]
        is_head = (rng.random(n_items) < rng.choice([0.0, 0.2, 0.5, 1.0])).astype(np.uint8)
        idx, val, hist = _random_row(rng, N, n_items)
        widx, wval = xquad_ref(idx[None], val[None], is_head, [hist], lam, K, variant)
        midx, mval = merge_row(idx, val, is_head, hist, lam, K, variant)
        np.testing.assert_array_equal(midx, widx[0])
        np.testing.assert_array_equal(mval, wval[0])
        nv = int((widx[0] >= 0).sum())
        changed += int((widx[0, :nv] != idx[:nv]).any())
    assert changed >= 40, "the rows should include many whose order xQuAD changes"


def test_reference_by_hand():
    """Four candidates, head head tail tail, values 3 2 1 0; the profile is half head, half tail; lambda 0.5, binary: the first tail item
    overtakes the second head item."""
    is_head = np.array([1, 1, 0, 0, 1, 0], np.uint8)
    idx = np.array([[0, 1, 2, 3]], np.int32)
    val = np.array([[3, 2, 1, 0]], f32)
    widx, wval = xquad_ref(idx, val, is_head, [[4, 5, 5]], 0.5, 4, "binary")
    # p = 1, 2/3, 1/3, 0; x = 0.5 p + 0.5 * 0.5 * cov: step 0 picks item 0 (0.75); then the head bonus is gone: item 1 0.3333, item 2 0.1667 + 0.25
    assert widx.tolist() == [[0, 2, 1, 3]]
    p = (val[0] / f32(3)).astype(f32)
    want = [f32(f32(0.5) * p[0]) + f32(0.25), f32(f32(0.5) * p[2]) + f32(0.25), f32(f32(0.5) * p[1]), f32(0)]
    np.testing.assert_array_equal(wval[0], np.array(want, f32))
    # without a profile, or with lambda = 0, nothing moves
    assert xquad_ref(idx, val, is_head, None, 0.5, 4, "smooth")[0].tolist() == [[0, 1, 2, 3]]
    assert xquad_ref(idx, val, is_head, [[4, 5]], 0.0, 3, "smooth")[0].tolist() == [[0, 1, 2]]
    # a short row: -1 and -inf behind the valid prefix, which ends at the first invalid position whatever follows it
    idx2 = np.array([[0, 9, 2, 3]], np.int32)
    widx, wval = xquad_ref(idx2, val, is_head, [[4, 5]], 0.5, 3, "smooth")
    assert widx.tolist() == [[0, -1, -1]] and np.isneginf(wval[0, 1:]).all() and wval[0, 0] == f32(0.25)   # one candidate: rng = 0


def test_search_for_the_end_of_the_prefix():
    for N in (65, 100, 128, 129, 257, 1000, 1023, 1024):
        for base in range(64, N, 64):
            ends = set(range(base, min(N, base + 40) + 1)) | {N - 1, N} | set(range(base, N + 1, 37))
            for nv in ends:
                valid = np.arange(N) < nv
                assert prefix_end_search(valid, base) == nv, (N, base, nv)


# ---- flags and the driver ------------------------------------------------------------------------------------------------------------------
def test_flags_default_to_the_documented_values():
    from pda_amd.parse import parse_args, reference_flag_names
    a = parse_args([])
    assert (a.xq_lambda, a.xq_candidates, a.xq_head_share, a.xq_variant) == (0.5, 1000, 0.8, "smooth")
    a = parse_args(["--xq_lambda", "0.25", "--xq_candidates", "300", "--xq_head_share", "0.6", "--xq_variant", "binary"])
    assert (a.xq_lambda, a.xq_candidates, a.xq_head_share, a.xq_variant) == (0.25, 300, 0.6, "binary")
    for name in ("xq_lambda", "xq_candidates", "xq_head_share", "xq_variant"):
        assert name not in reference_flag_names()


def _toy(tmp_path):
    from pda_amd import synthetic
    toy = str(tmp_path / "data") + "/"
    synthetic.write_dataset(toy + "toy", n_users=60, n_items=40, mean_hist=6)
    return toy


def test_cli_refusals_without_a_device(tmp_path):
    from pda_amd import xquad
    toy = _toy(tmp_path)
    save = str(tmp_path / "save") + "/"
    base = ["--data_path", toy, "--dataset", "toy", "--save_dir", save, "--Ks", "[20,50]", "--regs", "0.01", "--lr", "0.002", "--saveID", "x",
            "--pop_exp", "0.22"]
    with pytest.raises(NotImplementedError, match=r"^Not implement this training method\.\.\.\.\.$"):
        xquad.main(base + ["--train", "s_condition"])
    with pytest.raises(ValueError, match="xq_lambda"):
        xquad.main(base + ["--train", "normal", "--xq_lambda", "1.5"])
    with pytest.raises(ValueError, match="xq_candidates"):
        xquad.main(base + ["--train", "normal", "--xq_candidates", "49"])
    with pytest.raises(ValueError, match="xq_candidates"):
        xquad.main(base + ["--train", "normal", "--xq_candidates", "1025"])
    with pytest.raises(ValueError, match="xq_head_share"):
        xquad.main(base + ["--train", "normal", "--xq_head_share", "1.0"])
    with pytest.raises(ValueError, match="xq_variant"):
        xquad.main(base + ["--train", "normal", "--xq_variant", "product"])
    want = save + "mf_toy_checkpoint/wd_0.01_lr_0.002_a_0.001_xpop_exp-0.22_train_normal/best_ckpt.ckpt"
    with pytest.raises(FileNotFoundError) as e:
        xquad.main(base + ["--train", "normal"])
    assert want in str(e.value)
    assert not os.path.exists(save)
