"""CPU suite for the bit-reproducible training path (`--deterministic 1`): the C surface of include/pda_hip_det.h against the ctypes
binding, its argument checks, the flag, and the combinations a model refuses when it is built -- all without a GPU."""
import ctypes as C
import types

import pytest

from test_abi import declared_in


def test_library_exports_the_deterministic_header_and_the_binding_matches():
    from pda_amd import _lib
    lib = _lib.load()
    names = declared_in("pda_hip_det.h")
    assert names == ["pda_adam_step_plan_f32", "pda_bpr_grad_plan_f32", "pda_bpr_grad_plan_scratch_bytes", "pda_metrics_ordered",
                     "pda_metrics_ordered_workspace_bytes"]
    for n in names:
        assert hasattr(lib, n), "libpda_hip.so does not export " + n
    assert sorted(_lib.DET_SIGNATURES) == names, "ctypes binding and header disagree"
    for other in (_lib.SIGNATURES, _lib.TEMP_POP_SIGNATURES, _lib.PC_SIGNATURES):
        assert not set(other) & set(names)
    for h in ("pda_hip.h", "pda_hip_experimental.h", "pda_hip_temp_pop.h", "pda_hip_pc.h"):
        assert not set(declared_in(h)) & set(names), h


def _buf(n_bytes=4096):
    """A host buffer: good enough for an argument that must only be non-null (every check happens before any HIP call)."""
    b = C.create_string_buffer(n_bytes)
    return b, C.c_void_p(C.addressof(b))


def test_argument_checks_without_gpu():
    from pda_amd import _lib
    lib = _lib.load()
    null = C.c_void_p(None)
    keep, p = _buf()
    ARG, UNSUPPORTED = -1, -2

    def grad(U=p, I=p, users=p, pos=p, neg=p, pp=null, pn=null, B=8, d=64, reg_div=8.0, plan=p, scratch=p, gU=p, tagU=p, gI=p, tagI=p):
        return lib.pda_bpr_grad_plan_f32(U, I, users, pos, neg, pp, pn, B, d, 1e-2, reg_div, plan, scratch, gU, tagU, gI, tagI, 1, null, null)

    for kw in ({"U": null}, {"I": null}, {"users": null}, {"pos": null}, {"neg": null}, {"plan": null}, {"scratch": null}, {"gU": null},
               {"gI": null}, {"B": 0}, {"B": -3}, {"reg_div": 0.0}, {"pp": p}, {"tagU": null}, {"tagI": null}):
        assert grad(**kw) == ARG, kw
    assert grad(d=48) == UNSUPPORTED and grad(d=512) == UNSUPPORTED

    def step(U=p, mU=p, vU=p, gU=p, tagU=p, nU=10, I=p, mI=p, vI=p, gI=p, tagI=p, nI=10, users=p, B=8, d=64, tag=1, policy=0, plan=p, scratch=p):
        return lib.pda_adam_step_plan_f32(U, mU, vU, gU, tagU, nU, I, mI, vI, gI, tagI, nI, users, p, p, null, null, B, d, 1e-2, 8.0, tag, 1e-3, 0.9,
                                          0.999, 1e-8, policy, plan, scratch, null, null)

    for kw in ({"U": null}, {"mU": null}, {"vU": null}, {"gU": null}, {"tagU": null}, {"nU": 0}, {"I": null}, {"mI": null}, {"vI": null},
               {"gI": null}, {"tagI": null}, {"nI": 0}, {"users": null}, {"B": 0}, {"tag": 0}, {"policy": 3}, {"policy": -1}, {"plan": null},
               {"scratch": null}):
        assert step(**kw) == ARG, kw
    assert step(d=48) == UNSUPPORTED

    def metrics(topk=p, n_rows=4, k_cols=50, ptr=p, idx=p, Ks=p, n_ks=2, sums=p, ws=p):
        return lib.pda_metrics_ordered(topk, n_rows, k_cols, ptr, idx, Ks, n_ks, sums, ws, null)

    for kw in ({"topk": null}, {"ptr": null}, {"idx": null}, {"Ks": null}, {"sums": null}, {"ws": null}, {"n_rows": 0}, {"n_ks": 0},
               {"k_cols": 0}, {"k_cols": 65}):
        assert metrics(**kw) == ARG, kw
    del keep


def test_workspace_sizes():
    from pda_amd import _lib
    lib = _lib.load()
    for B, d in ((1024, 64), (2048, 128), (32768, 64)):
        assert lib.pda_bpr_grad_plan_scratch_bytes(B, d) == lib.pda_bpr_step_plan_scratch_bytes(B, d) >= (B * (d + 2)) * 4
    assert lib.pda_bpr_grad_plan_scratch_bytes(0, 64) == 0
    # one float64 per wave (four per 256-row workgroup) and sum
    assert lib.pda_metrics_ordered_workspace_bytes(100000, 2) == 4 * 2 * 4 * ((100000 + 255) // 256) * 8
    assert lib.pda_metrics_ordered_workspace_bytes(1, 1) == 4 * 4 * 8
    assert lib.pda_metrics_ordered_workspace_bytes(0, 2) == 0 == lib.pda_metrics_ordered_workspace_bytes(5, 0)


def test_flag_parses_and_defaults_to_off():
    from pda_amd.parse import parse_args, reference_flag_names
    assert parse_args([]).deterministic == 0
    assert parse_args(["--deterministic", "1"]).deterministic == 1
    assert "deterministic" not in reference_flag_names()


def _args(**kw):
    from pda_amd.parse import parse_args
    a = parse_args(["--deterministic", "1", "--batch_size", "256"])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


CFG = {"n_users": 400, "n_items": 300}


@pytest.mark.parametrize("kw, words", [
    ({"table_dtype": "bf16"}, "bf16"),
    ({"table_dtype": "bf16", "optimizer": "lazy_adam"}, "bf16"),
    ({"optimizer": "sgd_fused"}, "hogwild"),
    ({"embed_size": 48}, "embed_size"),
    ({"embed_size": 512}, "embed_size"),
    ({"batch_size": 401}, "with replacement"),
    ({"gpus": 2}, "one GPU"),
])
def test_refused_combinations_raise_before_anything_touches_a_gpu(kw, words):
    from pda_amd import model_api
    for cls in (model_api.BPRMF, model_api.ConditionalBPRMF):
        with pytest.raises(NotImplementedError, match=words):
            cls(_args(**kw), CFG, device="cuda")


def test_temp_pop_and_the_item_parallel_step_are_refused():
    import torch
    from pda_amd import dist, model_api
    with pytest.raises(NotImplementedError, match="temp_pop"):
        model_api.BPRMFTempPop(_args(train="temp_pop"), dict(CFG, temp_num=3), device="cuda")
    with pytest.raises(NotImplementedError, match="temp_pop"):
        model_api.check_deterministic(_args(train="temp_pop"), CFG)
    U, I = torch.zeros(8, 32), torch.zeros(4, 32)
    with pytest.raises(NotImplementedError, match="one GPU"):
        dist.ItemShardedBPR(U, I, 0, regs=1e-2, lr=1e-2, global_batch=8, deterministic=True)


def test_accepted_combinations_pass_the_check():
    from pda_amd import model_api
    for kw in ({}, {"optimizer": "lazy_adam"}, {"optimizer": "sgd"}, {"optimizer": "sgd", "table_dtype": "bf16"}, {"adam_sweep": "replay"},
               {"embed_size": 32}, {"embed_size": 256}, {"batch_size": 400}):
        model_api.check_deterministic(_args(**kw), CFG)


def test_the_trainer_asks_the_device_sampler_for_plans(monkeypatch):
    """DatasetApi_Model sets with_plan for every optimiser under --deterministic 1 (without the flag: --optimizer sgd only)."""
    from pda_amd import train_new_api as t
    monkeypatch.setattr(t, "BPRMF", lambda *a, **k: types.SimpleNamespace())
    for det, opt, want in ((1, "adam", True), (1, "lazy_adam", True), (0, "adam", False), (0, "sgd", True), (1, "sgd", True)):
        a = _args(optimizer=opt, deterministic=det, train="normal")
        sampler = types.SimpleNamespace(distinct_users=True, with_plan=False)
        t.DatasetApi_Model(a, CFG, 256, sampler, device="cuda")
        assert sampler.with_plan is want, (det, opt)
