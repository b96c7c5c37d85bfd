"""CPU suite for BPR-PC (`python -m pda_amd.bpr_pc`): the oracle of tests/pc_ref.py against a line-by-line transcription of the reference's
graph, the moment identity the library's statistics rest on, the popularity, the driver's host logic and the C entry points' argument checks."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from pc_ref import counts_matrix, finish_stats, pc_lists, stats_direct, stats_moments, transcription

f32 = np.float32


def case(rng, kind, nU=12, N=70, d=16):
    U = (rng.standard_normal((nU, d)) * 0.3).astype(f32)
    I = (rng.standard_normal((N, d)) * 0.3).astype(f32)
    pop = rng.integers(1, 40, N).astype(np.float64)
    users = np.arange(nU, dtype=np.int32)
    hist = [np.sort(rng.choice(N, rng.integers(1, 9), replace=False)) for _ in range(nU)]
    if kind == "dups":
        hist[0] = np.sort(np.concatenate([hist[0], hist[0][:2]]))               # c = 2
        hist[1] = np.sort(np.concatenate([hist[1], [hist[1][0]] * 2]))          # c = 3
    elif kind == "empty":
        hist[2] = np.zeros(0, np.int64)
    elif kind == "near_full":
        hist[3] = np.delete(np.arange(N), 17)                                    # all but one item: the list is filled with listed ones
        rest = np.delete(np.arange(N), [5, 9])
        hist[4] = np.sort(np.concatenate([rest, rest, [1]]))                    # two unmasked, the others listed twice (item 1: 3 times)
    return U, I, users, hist, pop


KINDS = ["plain", "dups", "empty", "near_full"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("alpha, beta", [(0.1, 0.1), (2.0, 0.3), (0.5, 1.0), (0.0, 0.0)])
def test_oracle_equals_the_transcription_of_the_graph(kind, alpha, beta):
    rng = np.random.default_rng(len(kind) + int(10 * beta))
    U, I, users, hist, pop = case(rng, kind)
    s = (U[users].astype(np.float64) @ I.T.astype(np.float64)).astype(f32)    # any fp32 scores: both sides take the same s
    Un, Uc, k = finish_stats(*stats_direct(U, I, users, hist, pop, beta))
    tUn, tUc, tk, _, _ = transcription(s, hist, pop, alpha, beta, 50)
    np.testing.assert_allclose(tUn, Un, rtol=2e-6)
    np.testing.assert_allclose(tUc, Uc, rtol=2e-6)
    np.testing.assert_allclose(tk, k, rtol=4e-6)
    for K in (1, 20, 50):
        idx, val = pc_lists(s, hist, pop, k, alpha, beta, K, block=len(users))
        _, _, _, tidx, tval = transcription(s, hist, pop, alpha, beta, K, k=k)
        np.testing.assert_array_equal(idx, tidx)
        np.testing.assert_array_equal(val, tval)
    if kind == "near_full":
        assert (val[3, 1:] == 0).all() and idx[3, 0] == 17                     # one unmasked item, then the listed ones by id
        assert (val[4, :2] > 0).all() and (val[4, 2:] < 0).all()               # listed twice: -g, ranked by g ascending


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("beta", [0.0, 0.3, 1.0])
def test_moment_form_equals_the_direct_sums(kind, beta):
    rng = np.random.default_rng(7 + len(kind))
    U, I, users, hist, pop = case(rng, kind)
    A, Bc, n = stats_direct(U, I, users, hist, pop, beta)
    A2, Bc2, n2 = stats_moments(U, I, users, hist, pop, beta)
    np.testing.assert_array_equal(n, n2)
    # relative to the sums over the whole catalogue, which the moment form starts from: a near-full history cancels most of them
    A0, B0, _ = stats_direct(U, I, users, [[]] * len(users), pop, beta)
    assert (np.abs(A2 - A) <= 1e-12 * A0).all() and (np.abs(Bc2 - Bc) <= 1e-12 * B0).all()
    keep = np.array([len(h) < I.shape[0] // 2 for h in hist])
    np.testing.assert_allclose(A2[keep], A[keep], rtol=1e-12)
    np.testing.assert_allclose(Bc2[keep], Bc[keep], rtol=1e-12)


def test_empty_complement_gives_k_zero():
    """The deviation: n_u = 0 (every item listed) gives k_u = 0, where the reference divides by zero."""
    rng = np.random.default_rng(3)
    U, I, users, hist, pop = case(rng, "plain")
    hist[0] = np.arange(I.shape[0])
    Un, Uc, k = finish_stats(*stats_moments(U, I, users, hist, pop, 0.3))
    assert Un[0] == 0 and Uc[0] == 0 and k[0] == 0 and (k[1:] > 0).all()


def test_one_minimum_per_block_of_rows():
    rng = np.random.default_rng(5)
    U, I, users, hist, pop = case(rng, "plain", nU=10)
    s = (U @ I.T).astype(f32)
    k = finish_stats(*stats_direct(U, I, users, hist, pop, 0.2))[2]
    idx, val = pc_lists(s, hist, pop, k, 0.4, 0.2, 20, block=4)
    for b0 in (0, 4, 8):
        sl = slice(b0, b0 + 4)
        _, _, _, tidx, tval = transcription(s[sl], hist[sl], pop, 0.4, 0.2, 20, k=k[sl])
        np.testing.assert_array_equal(idx[sl], tidx)
        np.testing.assert_array_equal(val[sl], tval)


def test_counts_matrix_counts_duplicates():
    c = counts_matrix([[1, 1, 3], []], 5)
    assert c.tolist() == [[0, 2, 0, 1, 0], [0, 0, 0, 0, 0]]


class _Data:
    def __init__(self):
        self.n_items = 5
        self.train_item_list = {0: [1, 2], 2: [4, 4, 4], 4: [0]}


def test_popularity_counts_entries_plus_one(capsys):
    from pda_amd.bpr_pc import get_dataset_tot_popularity_for_PC
    pop = get_dataset_tot_popularity_for_PC(_Data())
    assert pop.dtype == np.float64 and pop.tolist() == [3.0, 1.0, 4.0, 1.0, 2.0]
    assert "popularity information-- mean:" in capsys.readouterr().out


def test_eval_block_rounds_down_to_reference_blocks():
    from pda_amd.bpr_pc import pc_eval_block
    assert [pc_eval_block(b) for b in (1, 2048, 3000, 4096, 262144, 262143)] == [2048, 2048, 2048, 4096, 262144, 260096]


def _toy(tmp_path):
    from pda_amd import synthetic
    toy = str(tmp_path / "data") + "/"
    synthetic.write_dataset(toy + "toy", n_users=60, n_items=40, mean_hist=6)
    return toy


def test_cli_refuses_other_training_methods(tmp_path):
    from pda_amd import bpr_pc
    toy = _toy(tmp_path)
    with pytest.raises(NotImplementedError, match=r"^Not implement this training method\.\.\.\.\.$"):
        bpr_pc.main(["--data_path", toy, "--dataset", "toy", "--train", "s_condition"])


def test_cli_names_the_checkpoint_that_train_normal_writes(tmp_path):
    from pda_amd import bpr_pc
    from pda_amd import train_new_api as t
    toy = _toy(tmp_path)
    save = str(tmp_path / "save") + "/"
    argv = ["--data_path", toy, "--dataset", "toy", "--train", "normal", "--save_dir", save, "--regs", "0.01", "--fregs", "0.5",
            "--lr", "0.002", "--saveID", "x", "--pop_exp", "0.22"]
    # train_new_api.main (--train normal): saveID += pop_exp-{:.2f}, wd = regs, and this directory
    fmt = '"{}_{}_checkpoint/wd_{}_lr_{}_a_{}_{}_train_{}/".format(\n        args.model, args.dataset, args.wd, args.lr, args.alpha, args.saveID, args.train)'
    assert fmt in inspect.getsource(t.main)
    want = save + "mf_toy_checkpoint/wd_0.01_lr_0.002_a_0.001_xpop_exp-0.22_train_normal/best_ckpt.ckpt"
    with pytest.raises(FileNotFoundError) as e:
        bpr_pc.main(argv)
    assert want in str(e.value)
    assert not os.path.exists(save)


def test_set_clicked_value_type():
    from pda_amd.train_new_api import evaluation
    ev = evaluation.__new__(evaluation)
    ev.set_clicked_value_type("inf")
    ev.set_clicked_value_type("pc")
    assert ev.value_type == "pc"
    with pytest.raises(ValueError):
        ev.set_clicked_value_type("zero")


def test_pc_entry_points_check_arguments_without_gpu():
    from pda_amd import _lib
    lib = _lib.load()
    null, fake = C.c_void_p(None), C.c_void_p(0x100000)
    assert set(_lib.PC_SIGNATURES) == {"pda_pc_moments_workspace_bytes", "pda_pc_item_moments_f32", "pda_pc_user_stats_f32",
                                       "pda_pc_score_workspace_bytes", "pda_pc_score_topk_f32"}
    assert not set(_lib.PC_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.TEMP_POP_SIGNATURES))
    ERR_ARG, ERR_UNSUPPORTED = -1, -2
    # moments
    assert lib.pda_pc_item_moments_f32(null, fake, 100, 64, fake, fake, null) == ERR_ARG
    assert lib.pda_pc_item_moments_f32(fake, fake, 100, 32, fake, fake, null) == ERR_UNSUPPORTED
    assert lib.pda_pc_moments_workspace_bytes(100, 32) == 0 and lib.pda_pc_moments_workspace_bytes(100, 64) > 0
    # user stats
    st = lambda *p, d=64, beta=0.1: lib.pda_pc_user_stats_f32(*p, 16, 100, d, null, null, 0, beta, fake, fake, fake, null)
    assert st(fake, fake, fake, null, fake) == ERR_ARG
    assert st(fake, fake, fake, fake, fake, d=32) == ERR_UNSUPPORTED
    assert st(fake, fake, fake, fake, fake, beta=float("nan")) == ERR_ARG
    # score
    def sc(U=fake, scale=fake, out=fake, d=64, K=50, alpha=0.1, beta=0.1, rpm=2048, ws=fake):
        return lib.pda_pc_score_topk_f32(U, fake, fake, scale, fake, 16, 100, d, null, null, 0, alpha, beta, rpm, K, out, fake, ws, null)
    assert sc(U=null) == ERR_ARG and sc(scale=null) == ERR_ARG and sc(out=null) == ERR_ARG and sc(ws=null) == ERR_ARG
    assert sc(d=32) == ERR_UNSUPPORTED
    assert sc(K=51) == ERR_ARG and sc(K=0) == ERR_ARG
    assert sc(alpha=float("inf")) == ERR_ARG and sc(beta=float("nan")) == ERR_ARG and sc(rpm=0) == ERR_ARG
    assert lib.pda_pc_score_workspace_bytes(2048, 100, 64, 51) == 0 and lib.pda_pc_score_workspace_bytes(2048, 100, 64, 50) > 0


def test_ops_refuses_bad_arguments_before_the_library():
    import torch
    from pda_amd import ops
    cpu = torch.zeros((4, 64))
    with pytest.raises((ValueError, TypeError)):
        ops.recommend_topk_pc(cpu, cpu, torch.zeros(4, dtype=torch.int32), torch.ones(4), torch.ones(4), 0.1, 0.1, 2)
    with pytest.raises(TypeError, match="bf16"):
        ops.pc_item_moments(torch.zeros((4, 64), dtype=torch.bfloat16), torch.ones(4))
