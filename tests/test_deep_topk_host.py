"""CPU suite for deep lists (include/pda_hip_deep.h, `--topk_max`): the binding against its header, the entry points' argument checks (all of
them happen before any HIP call), the workspace size, the flag and the refusals of the command line."""
import ctypes as C
import os
import subprocess

import pytest

from test_abi import ROOT, declared_in

ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -4
OTHER_HEADERS = ["pda_hip.h", "pda_hip_experimental.h", "pda_hip_temp_pop.h", "pda_hip_pc.h", "pda_hip_det.h"]


def _buf(n_bytes=4096):
    """A host buffer: good enough for an argument that must only be non-null (every check happens before any HIP call)."""
    b = C.create_string_buffer(n_bytes)
    return b, C.c_void_p(C.addressof(b))


def test_binding_matches_the_header():
    from pda_amd import _lib
    assert declared_in("pda_hip_deep.h") == sorted(_lib.DEEP_SIGNATURES)
    assert _lib.DEEP_MAX_K == 1024
    text = open(os.path.join(ROOT, "include", "pda_hip_deep.h")).read()
    assert "#define PDA_DEEP_MAX_K 1024" in text


def test_every_symbol_is_exported():
    from pda_amd import _lib
    lib = _lib.load()
    for name in _lib.DEEP_SIGNATURES:
        assert getattr(lib, name).argtypes == _lib.DEEP_SIGNATURES[name][1], name
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if out.returncode == 0:
        exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
        assert set(_lib.DEEP_SIGNATURES) <= exported


def test_no_overlap_with_the_other_surfaces():
    from pda_amd import _lib
    deep = set(_lib.DEEP_SIGNATURES)
    for other in (_lib.SIGNATURES, _lib.TEMP_POP_SIGNATURES, _lib.PC_SIGNATURES, _lib.DET_SIGNATURES):
        assert not deep & set(other)
    for h in OTHER_HEADERS:
        assert not deep & set(declared_in(h)), h


def _call(lib, bufs, fn="pda_deep_topk_f32", **kw):
    null = C.c_void_p(None)
    p = dict(U=bufs, I=bufs, pop=null, users=bufs, nu=300, off=0, nloc=5000, d=64, K=100, head=0, keys=null, idx=bufs, val=bufs, ws=bufs, wsb=None)
    p.update(kw)
    if p["wsb"] is None:
        p["wsb"] = lib.pda_deep_topk_workspace_bytes(p["nu"], p["nloc"], 64, max(1, min(p["K"], 1024)))
    return getattr(lib, fn)(p["U"], p["I"], p["pop"], p["users"], p["nu"], p["off"], p["nloc"], p["d"], null, null, 0, p["K"], p["head"],
                            p["keys"], p["idx"], p["val"], p["ws"], p["wsb"], null)


@pytest.mark.parametrize("fn", ["pda_deep_topk_f32", "pda_deep_topk_bf16"])
def test_argument_checks_without_gpu(fn):
    from pda_amd import _lib
    lib = _lib.load()
    keep, b = _buf()
    null = C.c_void_p(None)
    call = lambda **kw: _call(lib, b, fn, **kw)
    assert call(U=null) == ERR_ARG and call(I=null) == ERR_ARG and call(users=null) == ERR_ARG
    assert call(keys=null, idx=null, val=null) == ERR_ARG
    assert call(ws=null) == ERR_ARG
    assert call(K=0) == ERR_ARG and call(K=1025) == ERR_ARG
    assert call(K=200, nloc=199) == ERR_ARG                       # K > n_items_local
    assert call(head=2) == ERR_ARG
    assert call(head=1) == ERR_ARG                                # the popularity head without a popularity
    assert call(d=48) == ERR_UNSUPPORTED
    need = lib.pda_deep_topk_workspace_bytes(300, 5000, 64, 100)
    assert need > 0
    assert call(wsb=need - 1) == ERR_WORKSPACE
    assert call(wsb=0) == ERR_WORKSPACE
    del keep


def test_metrics_argument_checks_without_gpu():
    from pda_amd import _lib
    lib = _lib.load()
    keep, b = _buf()
    null = C.c_void_p(None)
    m = lambda k_cols, topk=b, sums=b: lib.pda_metrics_deep(topk, 10, k_cols, b, b, b, 2, sums, null, null)
    assert m(0) == ERR_ARG and m(1025) == ERR_ARG and m(-3) == ERR_ARG
    assert m(100, topk=null) == ERR_ARG and m(100, sums=null) == ERR_ARG
    assert lib.pda_metrics_deep_workspace_bytes(1000, 4) > 0 and lib.pda_metrics_deep_workspace_bytes(0, 4) == 0
    assert lib.pda_metrics_deep_workspace_bytes(1000, 4) == lib.pda_metrics_ordered_workspace_bytes(1000, 4)
    # the short-list entry points keep their 64 columns
    assert lib.pda_metrics(b, 10, 65, b, b, b, 2, b, null) == ERR_ARG
    del keep


def test_workspace_size_is_monotone():
    from pda_amd import _lib
    lib = _lib.load()
    ws = lib.pda_deep_topk_workspace_bytes
    assert ws(0, 5000, 64, 100) == 0 and ws(300, 5000, 64, 0) == 0 and ws(300, 5000, 64, 1025) == 0
    for nloc in (1999, 5000, 200000, 3000000):
        for K in (1, 55, 100, 1000, 1024):
            prev = 0
            for nu in list(range(1, 3000, 37)) + list(range(3000, 300000, 4099)):
                b = ws(nu, nloc, 128, K)
                assert b >= prev > -1, (nloc, K, nu, b, prev)
                prev = b
        for nu in (1, 173, 8192, 70000):
            prev = 0
            for K in range(1, min(nloc, 1024) + 1):
                b = ws(nu, nloc, 128, K)
                assert b >= prev and b > 0, (nloc, nu, K, b, prev)
                prev = b
    # two buffers of at least 2 K keys per row would already be more than this at the deepest list: the size is a bounded slice per user
    assert ws(262144, 200000, 128, 1000) <= 262144 * (2048 * 8 + 64) + 4096


def test_ops_chunks_the_users_within_the_budget():
    from pda_amd import ops
    nu, nloc, d, K = 262144, 200000, 128, 1000
    chunk = ops.deep_chunk_users(nu, nloc, d, K)
    assert 0 < chunk < nu and chunk % 128 == 0
    assert ops.deep_workspace_bytes(chunk, nloc, d, K) <= ops.DEEP_WORKSPACE_BUDGET < ops.deep_workspace_bytes(chunk + 128, nloc, d, K)
    assert ops.deep_chunk_users(300, 5000, 64, 100) == 300
    assert ops.deep_chunk_users(5000, 5000, 64, 1000, budget=1) == 128      # never less than one tile


def test_identity_word_decodes():
    from pda_amd import ops
    for d in (32, 64, 128, 256):
        for head in (0, 1):
            for bf in (0, 1):
                w = (8 << 28) | (bf << 14) | (head << 13) | (d // 64)
                assert ops.deep_kernel_identity(w) == {"generation": ops.DEEP_GENERATION, "head": head, "bf16": bool(bf), "d": d}
                assert ops.deep_kernel_identity(w - (1 << 32)) == ops.deep_kernel_identity(w)      # (read back as a signed int32)


def test_ops_refuses_bad_arguments_before_the_library():
    import torch
    from pda_amd import ops
    cpu = torch.zeros((4, 64))
    with pytest.raises((ValueError, TypeError)):
        ops.recommend_topk_deep(cpu, cpu, torch.zeros(4, dtype=torch.int32), 2)
    with pytest.raises((ValueError, TypeError)):
        ops.metrics_sums_deep(torch.zeros((4, 100), dtype=torch.int32), torch.zeros(5, dtype=torch.int64), torch.zeros(1, dtype=torch.int32),
                              torch.zeros(1, dtype=torch.int32))


def test_topk_max_flag():
    from pda_amd.parse import parse_args, reference_flag_names
    assert parse_args([]).topk_max == 50 and parse_args([]).export_out == ""
    a = parse_args(["--topk_max", "300", "--export_out", "x.npz"])
    assert a.topk_max == 300 and a.export_out == "x.npz"
    assert "topk_max" not in reference_flag_names() and "export_out" not in reference_flag_names()


def _toy(tmp_path):
    from pda_amd import synthetic
    toy = str(tmp_path / "data") + "/"
    synthetic.write_dataset(toy + "toy", n_users=60, n_items=40, mean_hist=6)
    return toy


def test_topk_max_range_and_refusals():
    from pda_amd import train_new_api as t
    from pda_amd.parse import parse_args
    assert t.check_topk_max(parse_args([])) == 50
    assert t.check_topk_max(parse_args(["--topk_max", "54", "--train", "temp_pop"]), topk_shard=object()) == 54
    assert t.check_topk_max(parse_args(["--topk_max", "1024"])) == 1024
    for bad in ("0", "1025", "-5"):
        with pytest.raises(ValueError, match="topk_max"):
            t.check_topk_max(parse_args(["--topk_max", bad]))
    with pytest.raises(NotImplementedError, match="bias head"):
        t.check_topk_max(parse_args(["--topk_max", "55", "--train", "temp_pop"]))
    with pytest.raises(NotImplementedError, match="item shards"):
        t.check_topk_max(parse_args(["--topk_max", "55"]), topk_shard=object())
    # the model refuses before it builds anything
    with pytest.raises(NotImplementedError, match="item shards"):
        t.DatasetApi_Model(parse_args(["--topk_max", "100"]), {"n_users": 4, "n_items": 200}, 4, None, topk_shard=object())
    with pytest.raises(NotImplementedError, match="bias head"):
        t.DatasetApi_Model(parse_args(["--topk_max", "100", "--train", "temp_pop"]), {"n_users": 4, "n_items": 200}, 4, None)


def test_cli_refusals(tmp_path):
    from pda_amd import bpr_pc, export_topk
    from pda_amd import train_new_api as t
    toy = _toy(tmp_path)
    base = ["--data_path", toy, "--dataset", "toy", "--save_dir", str(tmp_path / "save") + "/"]
    with pytest.raises(NotImplementedError, match="BPR-PC ranks at most 50"):
        bpr_pc.main(base + ["--train", "normal", "--topk_max", "55"])
    with pytest.raises(NotImplementedError, match="bias head"):
        t.main(base + ["--train", "temp_pop", "--test", "temp_pop", "--topk_max", "100"])
    with pytest.raises(NotImplementedError, match="export_topk restores"):
        export_topk.main(base + ["--train", "temp_pop", "--topk_max", "20", "--export_out", str(tmp_path / "x.npz")])
    with pytest.raises(ValueError, match="topk_max"):
        export_topk.main(base + ["--train", "normal", "--topk_max", "2000", "--export_out", str(tmp_path / "x.npz")])
    assert not os.path.exists(str(tmp_path / "save"))
