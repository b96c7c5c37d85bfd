"""CPU suite for the LightGCN backbone (`--model lightgcn`, include/pda_hip_gcn.h): the graph build and the work list of pda_amd.ops against the
restatement of tests/lightgcn_ref.py, the fp32 emulation of the kernels inside the a-priori bound in three summation orders, every mutant outside
it, the closed-form gradient against autograd, the binding against the header, the entry points' argument checks (before any HIP call), the
refusals, the flag row and the checkpoint.

Observed on the shared cases (records, not thresholds): emulation err / bound at most 0.43 on a product or a propagation (0.29 on `small`, 0.43 on
`hub`, L = 1), 0.16 at L = 3; the mutants leave the bound by factors of 1.5e5 (dup_edges) to 1.2e7 (backward_no_scale)."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
import torch

import lightgcn_ref as lr
from test_abi import declared_in

ERR_ARG, ERR_UNSUPPORTED = -1, -2
CONFIG = {"n_users": 9, "n_items": 12}


def make_args(**over):
    from pda_amd.parse import parse_args
    a = parse_args(["--model", "lightgcn", "--embed_size", "64", "--batch_size", "16"])
    for k, v in over.items():
        setattr(a, k, v)
    return a


def arrays(name):
    from pda_amd import ops
    c = lr.graph_case(name)
    return ops.gcn_graph_arrays(*c["pairs"], c["n_users"], c["n_items"])


def ratio(got, ref, bound):
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(bound, 1e-300)).max())


# ---- the graph ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lr.GRAPHS)
def test_graph_is_symmetric_deduplicated_and_weighted_by_the_formula(name):
    c, ga = lr.graph_case(name), arrays(name)
    g, nu, ni = c["g"], c["n_users"], c["n_items"]
    N = nu + ni
    assert len(set(zip(*c["pairs"]))) == len(g["edges"]) == len(ga["edge_w"]) and (name != "small" or len(c["pairs"][0]) > len(g["edges"]))
    assert list(zip(ga["edge_users"].tolist(), ga["edge_items"].tolist())) == g["edges"]          # duplicates collapsed, sorted by (u, i)
    want = (1.0 / np.sqrt((ga["deg_u"][ga["edge_users"]] * ga["deg_i"][ga["edge_items"]]).astype(np.float64))).astype(np.float32)
    assert ga["edge_w"].dtype == np.float32 and np.array_equal(ga["edge_w"], want) and np.array_equal(ga["edge_w"], g["w"])      # bit-equal
    assert np.array_equal(np.concatenate([ga["deg_u"], ga["deg_i"]]), g["deg"]) and np.array_equal(np.diff(ga["indptr"]), g["deg"])
    assert ga["indptr"].dtype == np.int64 and ga["indices"].dtype == np.int32 and ga["w"].dtype == np.float32
    A = np.zeros((N, N))
    rows = np.repeat(np.arange(N), np.diff(ga["indptr"]))
    A[rows, ga["indices"]] = ga["w"]
    assert np.array_equal(A, A.T) and np.array_equal(A, g["A"])
    assert (A[:nu, :nu] == 0).all() and (A[nu:, nu:] == 0).all()
    for r in range(N):                                           # ascending inside each row
        assert (np.diff(ga["indices"][ga["indptr"][r]:ga["indptr"][r + 1]]) > 0).all()
    iso = np.flatnonzero(g["deg"] == 0)
    assert len(iso) >= 2 and (A[iso] == 0).all()
    if name == "small":
        assert g["deg"][0] == 0 and g["deg"][nu + 5] == 0 and g["deg"][1] == 1 and g["deg"][nu + 6] == 1 and g["deg"][nu - 1] > 0 and g["deg"][N - 1] > 0
    else:
        assert tuple(g["deg"][nu:nu + 4]) == lr.HUB_DEGREES


def test_ids_outside_the_tables_are_refused_once_on_the_host():
    from pda_amd import ops
    for u, i in (([0, 9], [0, 1]), ([0, 1], [0, 12]), ([-1, 1], [0, 1]), ([0, 1], [0, -2])):
        with pytest.raises(ValueError, match="outside the tables"):
            ops.gcn_graph_arrays(u, i, 9, 12)
    with pytest.raises(ValueError, match="one id per train pair"):
        ops.gcn_graph_arrays([0, 1], [0], 9, 12)
    g = ops.gcn_graph_arrays([], [], 9, 12)                     # a graph without edges: every row one empty entry
    assert g["work"].shape == (21, 4) and (g["work"][:, 1] == g["work"][:, 2]).all() and g["n_slots"] == 0


@pytest.mark.parametrize("name", lr.GRAPHS)
def test_work_list_covers_every_edge_once_in_chunks_of_a_fixed_order(name):
    from pda_amd import _lib, ops
    ga = arrays(name)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pda_hip_gcn.h")).read()
    assert int(re.search(r"#define PDA_GCN_CHUNK (\d+)", header).group(1)) == _lib.GCN_CHUNK == ops.GCN_CHUNK == lr.CHUNK
    work, longs, N = ga["work"], ga["long_rows"], len(ga["indptr"]) - 1
    seen = np.zeros(len(ga["indices"]), dtype=np.int64)
    for row, e0, e1, slot in work:
        assert ga["indptr"][row] <= e0 <= e1 <= ga["indptr"][row + 1] and e1 - e0 <= lr.CHUNK
        seen[e0:e1] += 1
    assert (seen == 1).all()
    assert (np.diff(work[:, 2] - work[:, 1]) <= 0).all()                                  # by falling length
    per_row = np.bincount(work[:, 0], minlength=N)
    assert (per_row >= 1).all() and np.array_equal(per_row, np.maximum(1, -(-np.diff(ga["indptr"]) // lr.CHUNK)))
    single = work[work[:, 3] < 0]
    assert (np.bincount(single[:, 0], minlength=N) == (per_row == 1)).all()               # whole rows: one entry, no slot
    slots = []
    for row, s0, n in longs:                                                                # cut rows: consecutive slots in edge order
        mine = work[work[:, 0] == row]
        mine = mine[np.argsort(mine[:, 1])]
        assert n == len(mine) >= 2 and list(mine[:, 3]) == list(range(s0, s0 + n)) and (mine[:-1, 2] == mine[1:, 1]).all()
        assert (mine[:-1, 2] - mine[:-1, 1] == lr.CHUNK).all()
        slots += list(range(s0, s0 + n))
    assert slots == list(range(ga["n_slots"])) and len(work) == N - len(longs) + ga["n_slots"]
    again = arrays(name)
    assert all(np.array_equal(ga[k], again[k]) for k in ("work", "long_rows", "indptr", "indices", "w"))
    if name == "hub":
        nu = ga["n_users"]
        assert [tuple(x) for x in longs] == [(nu + 2, 0, 2), (nu + 3, 2, 5)]              # chunk - 1 and chunk: one entry; chunk + 1: two; > 4 chunk: five
    else:
        assert len(longs) == 0
    small = ops.gcn_graph_arrays(*lr.graph_case("small")["pairs"], 301, 200, chunk=16)      # (the builder at another chunk length: the same rules)
    assert (small["work"][:, 2] - small["work"][:, 1]).max() == 16 and small["n_slots"] > 0


# ---- emulation inside the bound, mutants outside ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lr.GRAPHS)
def test_emulation_stays_inside_the_bound_in_three_orders(name):
    c, ga = lr.graph_case(name), arrays(name)
    g, d = c["g"], 32
    E0, G = lr.table(name, d), lr.table(name, d, seed=5, scale=1e-3)
    worst = {}
    for L in (1, 3):
        _, Fr = lr.propagate(g["A"], E0, L)
        _, Hr = lr.backward(g["A"], G, L)
        bF, bH = lr.propagate_bound(g, E0, L), lr.backward_bound(g, G, L)
        for order in lr.ORDERS:
            worst["F L=%d %s" % (L, order)] = ratio(lr.emulate_propagate(ga, E0, L, order), Fr, bF)
            worst["H L=%d %s" % (L, order)] = ratio(lr.emulate_backward(ga, G, L, order), Hr, bH)
    print("lightgcn emulation err / bound on %s: %s" % (name, {k: round(v, 3) for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0
    assert np.array_equal(lr.emulate_propagate(ga, E0, 0), E0)
    assert min(worst.values()) > 1e-3                           # (a bound a thousand times the error would hold nothing)


def test_fused_forms_and_the_regulariser_in_emulation():
    c, ga = lr.graph_case("hub"), arrays("hub")
    g, d = c["g"], 32
    X, add, S = lr.table("hub", d), lr.table("hub", d, seed=2), lr.table("hub", d, seed=3)
    y = g["A"] @ X.astype(np.float64)
    for order in lr.ORDERS:
        got, _ = lr.emulate_spmm(ga, X, add=add, scale=0.25, order=order)
        assert ratio(got, 0.25 * (add + y), lr.fused_bound(g, X, add=add, scale=0.25)[0]) <= 1.0
        gy, gs = lr.emulate_spmm(ga, X, sum_in=S, scale=1.0 / 3, order=order)
        by, bs = lr.fused_bound(g, X, sum_in=S, scale=1.0 / 3)
        assert ratio(gy, y, by) <= 1.0 and ratio(gs, (S + y) / 3, bs) <= 1.0
    mc = lr.model_case("small", 64, 300)
    b, nu = mc["batch"], mc["n_users"]
    R = lr.model(mc, 2, True)["R"].astype(np.float32)
    add, occ, _ = lr.reg_terms(mc["E0"], nu, b["users"], b["pos"], b["neg"], mc["regs"], mc["reg_div"])
    bound, _ = lr.reg_bound(mc["E0"], nu, b["users"], b["pos"], b["neg"], mc["regs"], mc["reg_div"], R.astype(np.float64))
    assert occ.max() > 50                                        # hot rows
    for order in lr.ORDERS:
        got = lr.emulate_reg(mc["E0"], nu, b["users"], b["pos"], b["neg"], mc["regs"], mc["reg_div"], R, order)
        r = ratio(got, R.astype(np.float64) + add, bound)
        print("lightgcn reg emulation err / bound (%s): %.3f" % (order, r))
        assert r <= 1.0


@pytest.mark.parametrize("pop", [False, True])
def test_closed_form_gradient_equals_autograd(pop):
    for name, d, B, L in (("small", 32, 37, 3), ("small", 64, 300, 2), ("small", 32, 1, 1), ("small", 32, 37, 0)):
        mc = lr.model_case(name, d, B)
        r = lr.model(mc, L, pop)
        g, loss = lr.autograd_grad(mc, L, pop)
        np.testing.assert_allclose(r["grad"], g, rtol=1e-10, atol=1e-15)
        np.testing.assert_allclose(r["loss"], loss, rtol=1e-12, atol=0)
        assert np.abs(r["grad"]).max() > 1e-4


MUTANT_CASE = ("small", 64, 37, 3)          # the named case: every mutant leaves the bound by more than 10 x here, with both heads


@pytest.mark.parametrize("mut", sorted(lr.MUTANTS))
@pytest.mark.parametrize("pop", [False, True])
def test_every_mutant_is_outside_the_bound_by_more_than_ten(mut, pop):
    name, d, B, L = MUTANT_CASE
    mc = lr.model_case(name, d, B)
    b = mc["batch"]
    ref, m = lr.model(mc, L, pop), lr.model(mc, L, pop, mut)
    q = lr.MUTANTS[mut][1]
    if q == "F":
        bound = lr.propagate_bound(mc["g"], mc["E0"], L)
    else:
        bound = lr.backward_bound(mc["g"], ref["G"], L) + lr.reg_bound(mc["E0"], mc["n_users"], b["users"], b["pos"], b["neg"], mc["regs"], mc["reg_div"],
                                                                       ref["R"])[0]
    # where the bound is far below the values (rows that take part): not a ratio against a bound of zero
    live = bound > 1e-3 * bound.max()
    r = float((np.abs(m[q] - ref[q])[live] / bound[live]).max())
    print("lightgcn mutant %s (%s): off by %.3g bounds" % (mut, q, r))
    assert r > 10.0
    assert lr.model(mc, L, pop, None)[q] is not None and np.array_equal(lr.model(mc, L, pop)[q], ref[q])


# ---- the binding and the argument checks ---------------------------------------------------------------------------------------------------------
def test_binding_equals_the_header():
    from pda_amd import _lib
    names = ["pda_gcn_reg_f32", "pda_gcn_spmm_f32", "pda_gcn_spmm_workspace_bytes"]
    assert declared_in("pda_hip_gcn.h") == sorted(_lib.GCN_SIGNATURES) == names
    for d in (_lib.SIGNATURES, _lib.TEMP_POP_SIGNATURES, _lib.PC_SIGNATURES, _lib.DET_SIGNATURES, _lib.DEEP_SIGNATURES, _lib.XQUAD_SIGNATURES,
              _lib.DICE_SIGNATURES, _lib.IPS_SIGNATURES, _lib.MACR_SIGNATURES):
        assert not set(names) & set(d)
    assert not set(names) & (set(declared_in("pda_hip.h")) | set(declared_in("pda_hip_experimental.h")))
    lib = _lib.load()
    for n in names:
        assert getattr(lib, n).argtypes == _lib.GCN_SIGNATURES[n][1]
    assert lib.pda_gcn_spmm_workspace_bytes(7, 64) == 7 * 64 * 4 and lib.pda_gcn_spmm_workspace_bytes(0, 64) == 0
    assert lib.pda_gcn_spmm_workspace_bytes(7, 48) == 0


def test_entry_points_check_arguments_without_gpu():
    from pda_amd import _lib
    lib = _lib.load()
    keep, keep2, keep3 = (C.create_string_buffer(4096) for _ in range(3))
    b, b2, b3 = (C.c_void_p(C.addressof(k)) for k in (keep, keep2, keep3))
    null = C.c_void_p(None)

    def spmm(indptr=b, work=b, X=b, Y=b2, add=null, sin=null, sout=null, longs=null, n_rows=10, n_work=10, n_long=0, n_slots=0, d=64, scale=1.0,
             ws=null, ws_bytes=0):
        return lib.pda_gcn_spmm_f32(indptr, b, b, n_rows, work, n_work, longs, n_long, n_slots, X, d, add, Y, sin, sout, scale, ws, ws_bytes, null)

    assert spmm(indptr=null) == ERR_ARG and spmm(work=null) == ERR_ARG and spmm(X=null) == ERR_ARG and spmm(Y=null) == ERR_ARG
    assert spmm(n_rows=0) == ERR_ARG and spmm(n_rows=1 << 31) == ERR_ARG and spmm(n_work=9) == ERR_ARG and spmm(n_work=11) == ERR_ARG
    assert spmm(sin=b3) == ERR_ARG and spmm(sout=b3) == ERR_ARG                                   # the running sum comes as a pair
    assert spmm(Y=b) == ERR_ARG and spmm(sin=b3, sout=b) == ERR_ARG and spmm(add=b2) == ERR_ARG   # X aliases an output; add aliases Y
    assert spmm(sin=b3, sout=b2) == ERR_ARG                                                        # Y aliases sum_out
    assert spmm(scale=float("nan")) == ERR_ARG and spmm(scale=float("inf")) == ERR_ARG
    assert spmm(n_long=1, n_slots=2, n_work=11, ws=b3, ws_bytes=4096) == ERR_ARG                   # cut rows without their list
    assert spmm(n_long=1, n_slots=1, n_work=10, longs=b3, ws=b3, ws_bytes=4096) == ERR_ARG         # a cut row has at least two chunks
    assert spmm(n_long=1, n_slots=2, n_work=11, longs=b3) == ERR_ARG                               # no workspace
    assert spmm(n_long=1, n_slots=2, n_work=11, longs=b3, ws=b3, ws_bytes=2 * 64 * 4 - 1) == ERR_ARG
    assert spmm(n_slots=2, n_work=12) == ERR_ARG                                                   # slots without cut rows
    assert spmm(d=16) == ERR_UNSUPPORTED and spmm(d=48) == ERR_UNSUPPORTED and spmm(d=512) == ERR_UNSUPPORTED

    def reg(U0=b, users=b, gU=b2, B=8, d=32, regs=1e-3, reg_div=8.0, nu=9, ni=12):
        return lib.pda_gcn_reg_f32(U0, b, nu, ni, users, b, b, B, d, regs, reg_div, gU, b2, null, null)

    assert reg(U0=null) == ERR_ARG and reg(users=null) == ERR_ARG and reg(gU=null) == ERR_ARG and reg(B=0) == ERR_ARG and reg(reg_div=0.0) == ERR_ARG
    assert reg(reg_div=float("nan")) == ERR_ARG and reg(regs=float("inf")) == ERR_ARG and reg(nu=0) == ERR_ARG and reg(ni=1 << 31) == ERR_ARG
    assert reg(d=16) == ERR_UNSUPPORTED and reg(d=96) == ERR_UNSUPPORTED
    del keep, keep2, keep3


def test_ops_refuses_bad_tensors_before_the_library():
    from pda_amd import ops
    g = ops.GcnGraph([0, 1, 2], [0, 1, 1], 9, 12, "cpu")
    assert g.n_rows == 21 and g.n_edges == 3
    U, I = torch.zeros(9, 32), torch.zeros(12, 32)
    i4 = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="HBM"):
        ops.gcn_propagate(g, U, I, 2)
    with pytest.raises(ValueError, match="HBM"):
        ops.gcn_backward(g, U, I, 2)
    with pytest.raises(ValueError, match="HBM"):
        ops.gcn_spmm(g, torch.zeros(21, 32))
    with pytest.raises(ValueError, match="HBM"):
        ops.gcn_reg(U, I, i4, i4, i4, U, I, regs=1e-3, reg_div=4)
    with pytest.raises(ValueError, match="0 .. 4"):
        ops.gcn_propagate(g, U, I, 5)
    with pytest.raises(ValueError, match="chunks of 512"):
        ops.GcnGraph([0], [0], 9, 12, "cpu", chunk=64)


# ---- flags and refusals ----------------------------------------------------------------------------------------------------------------------------
def test_the_flag_row_and_the_reference_rows():
    from pda_amd import parse
    a = parse.parse_args([])
    assert a.gcn_layers == 3 and type(a.gcn_layers) is int and a.model == "mf"
    ext = {f[0]: f for f in parse._EXTENSION_FLAGS}
    assert ext["gcn_layers"][1] is int and ext["gcn_layers"][2] == 3 and "0 .. 4" in ext["gcn_layers"][3]
    assert "gcn_layers" not in parse.reference_flag_names()
    ref = {f[0]: f for f in parse._REFERENCE_FLAGS}
    assert ref["model"][1] is None and ref["model"][2] == "mf" and "lightgcn" in ref["model"][3]
    b = parse.parse_args("--model lightgcn --gcn_layers 2 --train s_condition --test s_condition".split())
    assert (b.model, b.gcn_layers, b.train, b.test) == ("lightgcn", 2, "s_condition", "s_condition")


REFUSED = [({"train": "temp_pop", "test": "temp_pop"}, "--model lightgcn --train temp_pop"), ({"train": "dice"}, "--model lightgcn --train dice"),
           ({"train": "ips"}, "--model lightgcn --train ips"), ({"train": "macr", "test": "macr"}, "--model lightgcn --train macr"),
           ({"optimizer": "sgd"}, "--model lightgcn --optimizer sgd"), ({"optimizer": "lazy_adam"}, "--model lightgcn --optimizer lazy_adam"),
           ({"table_dtype": "bf16"}, "--model lightgcn --table_dtype bf16"), ({"deterministic": 1}, "--model lightgcn --deterministic 1"),
           ({"gpus": 2}, "--model lightgcn --gpus 2"), ({"test": "s_condition"}, "--model lightgcn --train normal --test s_condition"),
           ({"embed_size": 48}, "--model lightgcn --embed_size 48")]


@pytest.mark.parametrize("over, names", REFUSED)
def test_refused_combinations_are_named_before_anything_is_built(over, names, monkeypatch):
    from pda_amd import train_new_api as t
    from pda_amd.model_api import ConditionalLightGCN, LightGCN, check_lightgcn
    with pytest.raises(NotImplementedError, match=names):
        check_lightgcn(make_args(**over))
    for cls in (LightGCN, ConditionalLightGCN):
        with pytest.raises(NotImplementedError, match=names):
            cls(make_args(**over), CONFIG, device="cpu")
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(**over)))
    with pytest.raises(NotImplementedError, match=names):        # the trainer: before the data is read
        t.main([])


def test_layers_outside_the_range_and_unknown_models(monkeypatch):
    from pda_amd import train_new_api as t
    from pda_amd.model_api import check_lightgcn
    for L in (-1, 5):
        with pytest.raises(ValueError, match="--gcn_layers"):
            check_lightgcn(make_args(gcn_layers=L))
    for ok in ({}, {"gcn_layers": 0}, {"gcn_layers": 4}, {"train": "s_condition", "test": "s_condition"}, {"train": "s_condition", "test": "normal"}):
        check_lightgcn(make_args(**ok))
    monkeypatch.setattr(t, "configure", lambda argv=None: setattr(t, "args", make_args(model="ngcf")))
    with pytest.raises(NotImplementedError, match="--model ngcf"):
        t.main([])


def test_the_other_entry_points_keep_refusing_the_backbone():
    import inspect
    from pda_amd import bpr_pc, export_topk, xquad
    assert 'args.model != "mf"' in inspect.getsource(export_topk.restore)
    assert 'args.model == "mf"' in inspect.getsource(bpr_pc) and 'args.model == "mf"' in inspect.getsource(xquad)


# ---- the model and its checkpoint --------------------------------------------------------------------------------------------------------------------
def test_model_tables_graph_and_checkpoint():
    from pda_amd.model_api import BPRMF, ConditionalLightGCN, LightGCN, gcn_train_pairs
    pairs = gcn_train_pairs({0: [1, 2, 2], 3: [], 4: [11], 8: [0, 1]})
    assert pairs[0].tolist() == [0, 0, 0, 4, 8, 8] and pairs[1].tolist() == [1, 2, 2, 11, 0, 1]
    cfg = dict(CONFIG, gcn_train_pairs=pairs)
    a = LightGCN(make_args(gcn_layers=2), cfg, device="cpu", seed=1)
    ref = BPRMF(make_args(model="mf"), CONFIG, device="cpu", seed=1)
    for k in ("user_embedding", "item_embedding"):              # Xavier exactly as _MFBase.init_weights, from the same seed
        assert torch.equal(a.weights[k], ref.weights[k]) and a.weights[k].is_contiguous()
    assert a.weights["user_embedding"].data_ptr() + 9 * 64 * 4 == a.weights["item_embedding"].data_ptr()      # one stacked buffer
    assert a.graph.n_edges == 5 and a.gcn_layers == 2 and [f.name for f in (a.opt, a.loss, a.mf_loss, a.reg_loss)] == ["opt", "loss", "mf_loss", "reg_loss"]
    assert ConditionalLightGCN(make_args(train="s_condition", test="s_condition"), CONFIG, device="cpu").with_pop is True
    with pytest.raises(ValueError, match="train pairs"):
        LightGCN(make_args(), CONFIG, device="cpu").score_tables()
    z = LightGCN(make_args(gcn_layers=0), CONFIG, device="cpu")
    assert z.score_tables()[0] is z.weights["user_embedding"]                           # L = 0: the ego tables themselves
    st = a._opt_state()
    gen = torch.Generator().manual_seed(4)
    for k in ("mU", "vU", "mI", "vI"):
        st[k].copy_(torch.rand(st[k].shape, generator=gen))
    a._t = 17
    buf = io.BytesIO()
    torch.save(a.state_dict(), buf)
    sd = torch.load(io.BytesIO(buf.getvalue()))
    assert set(sd) == {"format", "model", "gcn_layers", "embed_size", "n_users", "n_items", "optimizer", "table_dtype", "user_embedding",
                       "item_embedding", "adam_t", "mU", "vU", "mI", "vI"}
    assert (sd["format"], sd["model"], sd["gcn_layers"], sd["adam_t"]) == ("pda_amd/2", "lightgcn", 2, 17)
    assert not any("graph" in k or "indptr" in k for k in sd)                           # the graph is rebuilt from the data
    b = LightGCN(make_args(gcn_layers=2), cfg, device="cpu", seed=5)
    b.load_state_dict(sd)
    assert b._t == 17 and all(torch.equal(b.weights[k], a.weights[k]) for k in a.weights) and all(torch.equal(b._state[k], st[k]) for k in st)
    # what load refuses
    with pytest.raises(ValueError, match="gcn_layers"):
        LightGCN(make_args(gcn_layers=3), cfg, device="cpu").load_state_dict(sd)
    with pytest.raises(ValueError, match="checkpoint of a lightgcn model"):
        ref.load_state_dict(sd)
    with pytest.raises(ValueError, match="checkpoint of a mf model"):
        b.load_state_dict(ref.state_dict())
    with pytest.raises(ValueError, match="n_users"):
        LightGCN(make_args(gcn_layers=2), {"n_users": 10, "n_items": 12}, device="cpu").load_state_dict(sd)
    with pytest.raises(ValueError, match="format"):
        b.load_state_dict(dict(sd, format="pda_amd/1"))
    with pytest.raises(ValueError, match="not a pda_amd checkpoint"):
        b.load_state_dict({"weights": 1})
    with pytest.raises(ValueError, match="shape"):
        b.load_state_dict(dict(sd, user_embedding=torch.zeros(9, 32)))
