"""tests/dirty_buffers.py itself, on CPU tensors, and the closure of the case table of tests/test_gpu_dirty_buffers.py: every function of
pda_amd.ops / model_api / sampler that allocates with torch.empty has a case there or a stated reason why it needs none."""
import numpy as np
import pytest
import torch

import dirty_buffers as db
from pda_amd import model_api, ops, sampler

# every dtype pda_amd/ops.py allocates (torch.empty with dtype=..., and empty_like of fp32 / bf16 tables)
DTYPES = [torch.uint8, torch.int32, torch.int64, torch.float32, torch.float64, torch.bfloat16]


def _alloc(n):
    """Stands for a function of pda_amd: the allocation is made through what pda_amd.ops sees as `torch` (its module global)."""
    return ops.torch.empty(n, dtype=ops.torch.uint8)


@pytest.mark.parametrize("fill", db.FILLS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_fill_shape_dtype_and_layout_are_those_asked_for(fill, dtype):
    with db.dirty(fill) as d:
        for size in ((7,), (3, 5), ((2, 3, 4),), (0,), (1,)):
            t = ops.torch.empty(*size, dtype=dtype)
            plain = torch.empty(*size, dtype=dtype)
            assert t.shape == plain.shape and t.dtype == plain.dtype and t.stride() == plain.stride() and t.device == plain.device
            assert t.is_contiguous()
            assert t.data_ptr() % 64 == 0 or t.numel() == 0
            raw = t.reshape(-1).view(torch.uint8)
            assert raw.numel() == plain.numel() * plain.element_size()
            assert bool((raw == fill).all())
        # the other two spellings, and a transposed (dense, non-contiguous) model for empty_like
        src = torch.zeros((4, 6), dtype=dtype).t()
        for t, plain in ((ops.torch.empty_like(src), torch.empty_like(src)), (model_api.torch.empty_like(src[0]), torch.empty_like(src[0])),
                         (sampler.torch.empty((2, 2), dtype=dtype), torch.empty((2, 2), dtype=dtype))):
            assert t.shape == plain.shape and t.dtype == plain.dtype and t.stride() == plain.stride()
            assert bool((t.contiguous().reshape(-1).view(torch.uint8) == fill).all())
        assert len(d.allocations) == 8
        d.check_guards()


def test_what_the_fills_mean():
    with db.dirty(0xFF):
        assert bool(torch.isnan(ops.torch.empty(4, dtype=torch.float32)).all())
        assert bool(torch.isnan(ops.torch.empty(4, dtype=torch.bfloat16).float()).all())
        assert ops.torch.empty(4, dtype=torch.int32).tolist() == [-1] * 4 and ops.torch.empty(2, dtype=torch.int64).tolist() == [-1] * 2
    with db.dirty(0x3F):
        np.testing.assert_allclose(ops.torch.empty(3, dtype=torch.float32).numpy(), 0.747, atol=1e-3)
        assert ops.torch.empty(1, dtype=torch.int32).item() == 0x3F3F3F3F
    with db.dirty(0x00):
        assert ops.torch.empty(5, dtype=torch.float64).tolist() == [0.0] * 5


def test_guards_lie_directly_around_the_requested_bytes():
    with db.dirty(0x00) as d:
        t = ops.torch.empty(13, dtype=torch.uint8)         # 13: no rounded size
        a = d.allocations[0]
        assert a.nbytes == 13 and a.raw.numel() == db.FRONT_GUARD + 13 + db.BACK_GUARD
        assert t.data_ptr() == a.raw.data_ptr() + db.FRONT_GUARD
        g = db.guard_byte(0x00)
        assert g != 0x00 and bool((a.raw[:db.FRONT_GUARD] == g).all()) and bool((a.raw[db.FRONT_GUARD + 13:] == g).all())
    for fill in range(256):
        assert db.guard_byte(fill) != fill


@pytest.mark.parametrize("where", ["one_past_the_end", "last_guard_byte", "one_before_the_start"])
def test_a_write_outside_the_buffer_is_reported_with_its_call_site(where):
    import inspect
    line = inspect.getsourcelines(_alloc)[1] + 2           # the line of the torch.empty in _alloc
    with db.dirty(0xFF) as d:
        ok = _alloc(100)
        t = _alloc(13)
        ok.fill_(1)
        t.fill_(1)                                         # writing the buffer itself touches nothing
        d.check_guards()
        a = d.allocations[1]
        at = {"one_past_the_end": db.FRONT_GUARD + 13, "last_guard_byte": a.raw.numel() - 1, "one_before_the_start": db.FRONT_GUARD - 1}[where]
        a.raw[at] = 0xFF if where != "one_past_the_end" else 0x00
        with pytest.raises(AssertionError) as e:
            d.check_guards()
    msg = str(e.value)
    assert "test_dirty_buffers_host.py:%d" % line in msg and "_alloc" in msg and "13-byte" in msg
    assert ("front" if where == "one_before_the_start" else "back") in msg
    assert msg.count("allocated at") == 1                  # the intact neighbour is not named
    assert {"one_past_the_end": "byte +13", "last_guard_byte": "byte +%d" % (13 + db.BACK_GUARD - 1), "one_before_the_start": "byte -1"}[where] in msg


def test_nothing_stays_patched():
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty, "new_empty" in torch.Tensor.__dict__)
    with pytest.raises(RuntimeError):
        with db.dirty(0x3F):
            assert ops.torch is not torch and ops.torch.float32 is torch.float32 and ops.torch.zeros(2).tolist() == [0.0, 0.0]
            raise RuntimeError("leaving by an exception")
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty, "new_empty" in torch.Tensor.__dict__) == before
    assert ops.torch is torch and model_api.torch is torch and sampler.torch is torch
    assert ops.torch.empty is torch.empty


def test_new_empty_is_dirty_for_pda_amd_only():
    src = torch.zeros(4, dtype=torch.int32)
    with db.dirty(0xFF) as d:
        assert src.new_empty((2, 3)).shape == (2, 3) and not d.allocations       # called from this file: the plain one
        code = compile("out = src.new_empty((2, 3))", ops.__file__, "exec")      # called from a line of pda_amd/ops.py
        env = {"src": src}
        exec(code, env)
        assert env["out"].tolist() == [[-1] * 3] * 2 and env["out"].dtype == torch.int32 and len(d.allocations) == 1
        d.check_guards()


def test_without_guards_only_the_fill():
    with db.dirty(0x3F, guard=False) as d:
        t = ops.torch.empty(9, dtype=torch.uint8)
        assert d.allocations[0].raw.numel() == 9 and bool((t == 0x3F).all())
        d.check_guards()


def test_fresh_caches_empties_every_cache():
    saved = {name: dict(getattr(ops, name)) for name in db.CACHES}
    try:
        for name in db.CACHES:
            getattr(ops, name)["probe"] = 1
        db.fresh_caches()
        assert all(not getattr(ops, name) for name in db.CACHES)
    finally:
        for name in db.CACHES:
            getattr(ops, name).clear()
            getattr(ops, name).update(saved[name])


def test_the_recorder_sees_results_and_arguments_and_compares_bit_for_bit():
    def run(x):
        with db.Recorder() as r:
            assert ops.unpack_keys is not db_unwrapped
            ops.unpack_keys(x)
        assert ops.unpack_keys is db_unwrapped
        return r.records
    db_unwrapped = ops.unpack_keys
    a = torch.tensor([[5, 7]], dtype=torch.int64)
    ra, rb, rc = run(a), run(a.clone()), run(a + 1)
    assert [n for n, _ in ra] == ["unpack_keys"] and "keys" in ra[0][1] and any(k.startswith("return") for k in ra[0][1])
    db.same_records(ra, rb, "equal")
    with pytest.raises(AssertionError, match="differs with the fill"):
        db.same_records(ra, rc, "unequal")
    nan1 = [("f", {"x": torch.tensor([float("nan"), 1.0])})]
    nan2 = [("f", {"x": torch.tensor([float("nan"), 1.0 + 1e-7])})]
    db.same_records(nan1, nan1, "nan")
    with pytest.raises(AssertionError):
        db.same_records(nan1, nan2, "bits")
    # a tolerance is for the atomically summed steps, and for calls whose inputs already differ -- nothing else
    with pytest.raises(AssertionError, match="differs with the fill"):
        db.same_records(nan1, nan2, "a deterministic call on equal inputs", rtol=1e-6, atol=0)
    step = lambda r: [("bpr_step", r[0][1])]                                                    # noqa: E731
    assert "bpr_step" in db.ATOMIC_STEPS and "f" not in db.ATOMIC_STEPS
    db.same_records(step(nan1), step(nan2), "an atomic step", rtol=1e-6, atol=0)
    with pytest.raises(AssertionError, match="is outside"):
        db.same_records(step(nan1), step(nan2), "an atomic step, too far", rtol=1e-9, atol=0)
    fed = lambda r, v: [("f", dict(r[0][1], **{"in:x": torch.tensor([v])}))]                     # noqa: E731
    db.same_records(fed(nan1, 1.0), fed(nan2, 1.0 + 1e-7), "a deterministic call on inputs that differ", rtol=1e-6, atol=0)
    with pytest.raises(AssertionError, match="differs with the fill"):
        db.same_records(fed(nan1, 1.0), fed(nan2, 1.0), "a deterministic call on equal inputs", rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# closure: a torch.empty in pda_amd without a case fails here
ACCEPTED = ("overwritten by torch", "measurement tool")


def test_every_allocating_function_has_a_case_or_a_reason():
    import test_gpu_dirty_buffers as g
    sites = db.alloc_sites()
    assert len(sites) > 40 and "ops.recommend_topk_deep" in sites and "sampler.DeviceSampler._refill" in sites     # the parser finds them
    covered = set()
    for name, case in g.CASES.items():
        unknown = set(case.functions) - set(sites)
        assert not unknown, "case %s names %s, which allocate nothing (renamed?)" % (name, sorted(unknown))
        covered |= set(case.functions)
    for fn, reason in g.EXEMPT.items():
        assert fn in sites, "EXEMPT names %s, which allocates nothing" % fn
        assert fn not in covered, "%s is exempt and has a case: drop the exemption" % fn
        assert reason.startswith(ACCEPTED) and "\n" not in reason, "not an accepted reason for %s: %r" % (fn, reason)
    missing = sorted(set(sites) - covered - set(g.EXEMPT))
    assert not missing, "these functions allocate with torch.empty and have no case in tests/test_gpu_dirty_buffers.py: %s" % missing


def test_the_gpu_module_runs_every_case():
    import test_gpu_dirty_buffers as g
    params = [m for m in g.test_the_call_does_not_depend_on_what_its_buffers_held.pytestmark if m.name == "parametrize"]
    assert len(params) == 1 and list(params[0].args[1]) == list(g.CASES)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the C caller's view
def test_python_clears_nothing_on_the_library_s_behalf():
    """A .zero_() / .fill_() of a buffer pda_amd allocated with torch.empty is a clear a caller of the C ABI would have to know about: the
    library clears what it needs itself, stream-ordered (recommend_topk_deep's 32 header bytes went into pda_deep_topk_* with this test)."""
    assert db.python_clears() == []


def test_every_size_function_of_the_headers_has_a_case():
    import test_gpu_dirty_buffers as g
    exported = db.exported_size_functions()
    assert len(exported) >= 18 and "pda_deep_topk_workspace_bytes" in exported and "pda_dice_rows_ws_words" in exported, exported
    held = {fn for c in g.CASES.values() for fn in c.sizes}
    assert held <= set(exported), sorted(held - set(exported))
    assert not set(exported) - held, "no case hands over a buffer of exactly %s" % sorted(set(exported) - held)
    sites = db.alloc_sites()
    assert set(g.SIZE_SITE) == set(exported) and all(f in sites for f in g.SIZE_SITE.values())
    for name, c in g.CASES.items():
        for fn in c.sizes:
            assert g.SIZE_SITE[fn] in c.functions or g.SIZE_SITE[fn] == "ops._metrics_deep" or name.startswith("score_"), (name, fn)


def test_the_clear_finder_finds_a_clear(tmp_path, monkeypatch):
    (tmp_path / "pda_amd").mkdir()
    for name in ("ops", "model_api", "sampler"):
        (tmp_path / "pda_amd" / (name + ".py")).write_text("import torch\n")
    (tmp_path / "pda_amd" / "ops.py").write_text(
        "import torch\n\ndef f(n):\n    ws = torch.empty(n)\n    out = torch.zeros(n)\n    out.zero_()\n    ws[:32].zero_()\n    return ws, out\n")
    monkeypatch.setattr(db, "ROOT", str(tmp_path))
    assert db.python_clears() == [("ops.f", 7)]
