"""Dirty, guarded allocations for pda_amd (a helper module: it holds no test).

    with dirty(0xFF) as db:
        fresh_caches()
        out = ops.recommend_topk(...)
        db.check_guards()

While the block is active every torch.empty / torch.empty_like / Tensor.new_empty performed by pda_amd.ops, pda_amd.model_api and
pda_amd.sampler returns memory whose every byte is `fill`, lying between two guard bands of another byte: FRONT_GUARD bytes in front
(512: the alignment the caching allocator gives is kept) and BACK_GUARD bytes behind, the latter starting at the first byte past the
REQUESTED size (not past a rounded one), so that a kernel writing one element beyond a short row or a *_workspace_bytes that is a few
bytes short lands in it. Shape, dtype, strides and device are those of the plain call. Nothing stays patched after the block.

The three fills of the suite (FILLS): 0x00 is what a fresh process mostly sees; 0xFF is NaN as fp32 and bf16, -1 as int32/int64 and an
all-ones key; 0x3F is 0.747 as fp32, a large positive integer and a plausible-looking key.
"""
import contextlib
import os
import sys

import numpy as np
import torch

FILLS = (0x00, 0xFF, 0x3F)
FRONT_GUARD = 512
BACK_GUARD = 4096

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "pda_amd") + os.sep
PATCHED_MODULES = ("pda_amd.ops", "pda_amd.model_api", "pda_amd.sampler")
CACHES = ("_PREP_CACHE", "_ORDER_CACHE", "_PREP_ORD_CACHE", "_POP_OK", "_FUNNEL_ORDER", "_PLAN_WS", "_METRICS_WS", "_DEEP_WS", "_EXPOSURE_KS")

_real_empty = torch.empty
_real_empty_like = torch.empty_like
_real_new_empty = torch.Tensor.new_empty


def fresh_caches():
    """Empty every cache of pda_amd.ops that holds device buffers, so that they are allocated again (under the current fill)."""
    from pda_amd import ops
    for name in CACHES:
        getattr(ops, name).clear()


def guard_byte(fill: int) -> int:
    return 0xA5 if fill != 0xA5 else 0x5A


def _call_site():
    """file:line of the innermost frame that lies in pda_amd (the torch.empty itself); the direct caller when there is none."""
    f = sys._getframe(1)
    while f.f_back is not None and os.path.abspath(f.f_code.co_filename) == os.path.abspath(__file__):
        f = f.f_back
    first = f
    while f is not None:
        fn = os.path.abspath(f.f_code.co_filename)
        if fn.startswith(PKG_DIR):
            return "%s:%d" % (os.path.relpath(fn, ROOT), f.f_lineno), f.f_code.co_name
        f = f.f_back
    return "%s:%d" % (first.f_code.co_filename, first.f_lineno), first.f_code.co_name


class Allocation:
    __slots__ = ("raw", "nbytes", "site", "func")

    def __init__(self, raw, nbytes, site, func):
        self.raw, self.nbytes, self.site, self.func = raw, nbytes, site, func


class _TorchProxy:
    """What a patched module sees as `torch`: the real module, except for the two allocating functions."""

    def __init__(self, mgr):
        self.__dict__["_mgr"] = mgr

    def __getattr__(self, name):
        return getattr(torch, name)

    def __setattr__(self, name, value):
        setattr(torch, name, value)

    def empty(self, *size, **kw):
        return self._mgr._empty(size, kw)

    def empty_like(self, t, **kw):
        return self._mgr._empty_like(t, kw)


class Dirty:
    def __init__(self, fill: int, guard: bool = True):
        assert 0 <= fill <= 255
        self.fill, self.guard = fill, guard
        self.gbyte = guard_byte(fill)
        self.allocations = []          # every buffer handed out (kept alive: a freed guard cannot be checked)
        self.active = False

    # -- allocation ---------------------------------------------------------------------------------------------------------------
    def _from_meta(self, meta, device, pin=False):
        """A dirty buffer with the shape, dtype and strides of `meta` (a tensor on the meta device) on `device`."""
        site, func = _call_site()
        esz = meta.element_size()
        n = meta.numel()
        # torch.empty and empty_like give dense memory: the extent is numel elements
        span = 0 if n == 0 else 1 + sum((s - 1) * st for s, st in zip(meta.shape, meta.stride()))
        assert span == n, "not a dense layout: %s %s" % (tuple(meta.shape), meta.stride())
        nbytes = n * esz
        front = FRONT_GUARD if self.guard else 0
        back = BACK_GUARD if self.guard else 0
        raw = _real_empty(front + nbytes + back, dtype=torch.uint8, device=device, pin_memory=pin)
        if self.guard:
            raw[:front].fill_(self.gbyte)
            raw[front + nbytes:].fill_(self.gbyte)
        body = raw[front:front + nbytes]
        body.fill_(self.fill)
        self.allocations.append(Allocation(raw, nbytes, site, func))
        return body.view(meta.dtype).as_strided(tuple(meta.shape), meta.stride())

    def _empty(self, size, kw):
        kw = dict(kw)
        if not self.active or kw.get("out") is not None or kw.get("layout", torch.strided) is not torch.strided:
            return _real_empty(*size, **kw)
        device = torch.device(kw.pop("device", None) or torch.get_default_device())
        pin = bool(kw.pop("pin_memory", False))
        requires_grad = bool(kw.pop("requires_grad", False))
        out = self._from_meta(_real_empty(*size, device="meta", **kw), device, pin)
        return out.requires_grad_() if requires_grad else out

    def _empty_like(self, t, kw):
        kw = dict(kw)
        if not self.active or kw.get("layout", torch.strided) is not torch.strided or t.layout is not torch.strided:
            return _real_empty_like(t, **kw)
        device = torch.device(kw.pop("device", None) or t.device)
        pin = bool(kw.pop("pin_memory", False))
        requires_grad = bool(kw.pop("requires_grad", False))
        out = self._from_meta(_real_empty_like(t, device="meta", **kw), device, pin)
        return out.requires_grad_() if requires_grad else out

    def _new_empty(self, t, size, kw):
        kw = dict(kw)
        device = torch.device(kw.pop("device", None) or t.device)
        pin = bool(kw.pop("pin_memory", False))
        requires_grad = bool(kw.pop("requires_grad", False))
        kw.setdefault("dtype", t.dtype)
        out = self._from_meta(_real_empty(*size, device="meta", **kw), device, pin)
        return out.requires_grad_() if requires_grad else out

    # -- checks -------------------------------------------------------------------------------------------------------------------
    def touched(self):
        """[(Allocation, 'front'|'back', first touched offset relative to the band)] over everything handed out so far."""
        if any(a.raw.is_cuda for a in self.allocations):
            torch.cuda.synchronize()
        bad = []
        if not self.guard:
            return bad
        for a in self.allocations:
            for name, band in (("front", a.raw[:FRONT_GUARD]), ("back", a.raw[FRONT_GUARD + a.nbytes:])):
                hit = band != self.gbyte
                if bool(hit.any()):
                    bad.append((a, name, int(hit.nonzero()[0, 0])))
        return bad

    def check_guards(self):
        bad = self.touched()
        assert not bad, "guard bytes overwritten (fill 0x%02X): " % self.fill + "; ".join(
            "%s guard of the %d-byte buffer allocated at %s (in %s), first at byte %+d" % (
                name, a.nbytes, a.site, a.func, off - FRONT_GUARD if name == "front" else a.nbytes + off)
            for a, name, off in bad)

    def sites(self):
        return sorted({a.site for a in self.allocations})

    def funcs(self):
        """The alloc_sites() names of the functions whose allocations were handed out."""
        table = alloc_sites()
        return {site_function(s, table) for s in self.sites()} - {None}


@contextlib.contextmanager
def dirty(fill: int, guard: bool = True):
    """See the module docstring. Yields the Dirty manager (allocations, check_guards(), sites(), funcs())."""
    import importlib
    mgr = Dirty(fill, guard)
    proxy = _TorchProxy(mgr)
    mods = [importlib.import_module(m) for m in PATCHED_MODULES]
    saved = [m.__dict__["torch"] for m in mods]
    pkg_files = {os.path.abspath(m.__file__) for m in mods}
    own_new_empty = "new_empty" in torch.Tensor.__dict__

    def new_empty(t, *size, **kw):
        if mgr.active and os.path.abspath(sys._getframe(1).f_code.co_filename) in pkg_files:
            return mgr._new_empty(t, size, kw)
        return _real_new_empty(t, *size, **kw)

    try:
        for m in mods:
            m.torch = proxy
        torch.Tensor.new_empty = new_empty
        mgr.active = True
        yield mgr
    finally:
        mgr.active = False
        if own_new_empty:
            torch.Tensor.new_empty = _real_new_empty
        elif "new_empty" in torch.Tensor.__dict__:
            del torch.Tensor.new_empty           # inherited before: leave no shadowing attribute behind
        for m, t in zip(mods, saved):
            m.torch = t


# -- which functions of pda_amd allocate (the closure check of tests/test_dirty_buffers_host.py and the case table's self-check) -----
ALLOCATORS = ("empty", "empty_like", "new_empty")


def alloc_sites():
    """{"ops.recommend_topk_deep": [(first line, last line), ...], ...}: every function (qualified inside its module, the module without
    its package) of the patched modules that calls torch.empty / torch.empty_like / Tensor.new_empty, with the line span of each such call."""
    import ast
    found = {}
    for mod in PATCHED_MODULES:
        short = mod.split(".")[-1]
        path = os.path.join(ROOT, *mod.split(".")) + ".py"
        with open(path) as f:
            tree = ast.parse(f.read(), path)

        def visit(node, qual):
            for child in ast.iter_child_nodes(node):
                q = qual
                if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                    q = qual + [child.name]
                elif isinstance(child, ast.Call) and isinstance(child.func, ast.Attribute) and child.func.attr in ALLOCATORS:
                    base = child.func.value
                    if child.func.attr == "new_empty" or (isinstance(base, ast.Name) and base.id == "torch"):
                        found.setdefault(".".join([short] + (qual or ["<module>"])), []).append((child.lineno, child.end_lineno))
                visit(child, q)

        visit(tree, [])
    return found


def site_function(site: str, sites=None):
    """The alloc_sites() key of a recorded call site 'pda_amd/ops.py:1950' (None when the line lies in no allocating call)."""
    path, line = site.rsplit(":", 1)
    short, line = os.path.splitext(os.path.basename(path))[0], int(line)
    for name, spans in (sites or alloc_sites()).items():
        if name.split(".")[0] == short and any(lo <= line <= hi for lo, hi in spans):
            return name
    return None


# -- the C caller's view: a workspace of exactly the size the library reports ----------------------------------------------------------
SIZE_FUNCTION = r"\bsize_t\s+(pda_\w+?(?:_workspace_bytes|_ws_words|_scratch_bytes))\s*\("


def exported_size_functions():
    """Every *_workspace_bytes / *_ws_words / *_scratch_bytes function the headers of include/ declare."""
    import glob
    import re
    names = set()
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        with open(path) as f:
            names |= set(re.findall(SIZE_FUNCTION, f.read()))
    return sorted(names)


@contextlib.contextmanager
def reported_sizes():
    """While active, every size function of the loaded library records what it reported: yields {name: [bytes, ...]} (words as bytes)."""
    from pda_amd import _lib
    lib = _lib.load()
    seen, saved = {}, {}

    def wrap(name, fn):
        unit = 4 if name.endswith("_ws_words") else 1

        def wrapper(*a):
            v = fn(*a)
            seen.setdefault(name, []).append(int(v) * unit)
            return v
        return wrapper

    try:
        for name in exported_size_functions():
            saved[name] = getattr(lib, name)
            setattr(lib, name, wrap(name, saved[name]))
        yield seen
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)


def python_clears():
    """[(function, line)]: every in-place clear (.zero_() / .fill_()) that a function of the patched modules applies to a name it bound to
    torch.empty / empty_like / new_empty (or to a slice of it): a clear on the library's behalf that a C caller would have to know about."""
    import ast
    found = []
    for mod in PATCHED_MODULES:
        path = os.path.join(ROOT, *mod.split(".")) + ".py"
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for fn in ast.walk(tree):
            if not isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
                continue
            bound = set()
            for node in ast.walk(fn):
                if isinstance(node, ast.Assign) and any(isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute) and c.func.attr in ALLOCATORS
                                                        for c in ast.walk(node.value)):
                    for t in node.targets:
                        bound |= {n.id for n in ast.walk(t) if isinstance(n, ast.Name)}
            for node in ast.walk(fn):
                if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in ("zero_", "fill_"):
                    base = node.func.value
                    while isinstance(base, (ast.Subscript, ast.Attribute)):
                        base = base.value
                    if isinstance(base, ast.Name) and base.id in bound:
                        found.append(("%s.%s" % (mod.split(".")[-1], fn.name), node.lineno))
    return found


# -- what a call left behind, fill by fill ---------------------------------------------------------------------------------------------
# Arguments that are workspaces: their contents after a call are the library's business and may depend on what they held before.
SCRATCH_ARGS = frozenset(("ws", "workspace", "scratch", "z_ws", "rows_ws", "barrier_ws", "bufs", "prep", "prep_ord", "prep7", "keep", "plan"))
# ... and functions that hand a workspace back (for reuse): their return value is not an output.
WORKSPACE_RETURNS = frozenset(("bpr_step_plan", "bpr_grad_plan", "adam_step_plan", "inbatch_workspace", "fullsm_workspace", "dau_workspace",
                               "dice_rows_ws", "pcc_workspace"))
# Diagnostics that depend on the order in which workgroups publish their thresholds, not on the inputs alone: measured on an MI355X, the
# generation-4 sweeps' count of exactly rescored pairs differs by a few in 10^4 between two runs under ONE fill (every other counter, the error
# word and the identity word are equal run after run and are compared).
TIMING_STATS = frozenset(("pairs_rescored",))
# Attributes that are not yet an output: MacrItemPrep.beta holds the bias of the c asked for last, and nothing before the first bias(c).
NOT_YET_WRITTEN = {("MacrItemPrep", "beta"): lambda obj: obj.c is None}
# Functions that return an item prep: one uint8 blob of fields with alignment gaps between them that belong to nobody.  The blob is not
# compared as a whole; tests/test_gpu_dirty_buffers.py compares every byte the layout names (prep_ref.named_bytes) in its prep case.
# A triplet plan is such a blob too: header, segments and flags in front of capacity for the worst case (2 B segments) that nobody reads;
# its used part is held by tests/test_gpu_bpr_plan.py's segmentation check under every fill, and the steps that read it are compared.
BLOB_RETURNS = frozenset(("item_prep", "item_prep_ordered", "item_prep4", "item_prep7", "triplet_plan"))


class Recorder:
    """While active, every public function defined in pda_amd.ops is wrapped: after each call the tensors it returned and the tensors among
    its arguments (also one level inside tuples, lists, dicts and plain objects; SCRATCH_ARGS left out) are cloned into `records` as
    (function name, {label: tensor}).  Two runs of the same deterministic test under two fills must leave equal records (same_records)."""

    def __init__(self, fill=None):
        self.records = []
        self.fill = fill
        self._saved = {}

    def _tensors(self, label, v, out, depth=0):
        if isinstance(v, torch.Tensor):
            out[label] = v.detach().clone()
        elif isinstance(v, np.ndarray) and v.dtype.kind in "biuf" and v.dtype.itemsize in (1, 2, 4, 8):
            a = np.array(v, copy=True, order="C")
            out[label] = torch.from_numpy(a.view("i%d" % a.dtype.itemsize) if a.dtype.kind == "u" and a.dtype.itemsize > 1 else a)
        elif depth < 2 and isinstance(v, (tuple, list)):
            for i, x in enumerate(v):
                self._tensors("%s[%d]" % (label, i), x, out, depth + 1)
        elif depth < 2 and isinstance(v, dict):
            for k, x in v.items():
                if k not in SCRATCH_ARGS and k not in TIMING_STATS:
                    self._tensors("%s[%r]" % (label, k), x, out, depth + 1)
        elif depth < 1 and (hasattr(v, "__dict__") or hasattr(v, "__slots__")) and not isinstance(v, type) and not callable(v):
            attrs = vars(v) if hasattr(v, "__dict__") else {k: getattr(v, k, None) for k in v.__slots__}
            for k, x in attrs.items():
                skip = NOT_YET_WRITTEN.get((type(v).__name__, k))
                if k not in SCRATCH_ARGS and not k.startswith("_") and not (skip and skip(v)):
                    self._tensors("%s.%s" % (label, k), x, out, depth + 1)

    def _wrap(self, name, fn):
        import functools
        import inspect
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def wrapper(*a, **kw):
            # what the call was handed ("in:" labels), so that same_records can tell a call whose inputs already differ from one that makes the
            # difference itself; a buffer still holding nothing but the fill is an output buffer, not an input
            pre, snap = {}, {}
            for k, v in sig.bind(*a, **kw).arguments.items():
                if k not in SCRATCH_ARGS and not (name == "triplet_plan" and k == "out"):
                    self._tensors("in:" + k, v, pre)
            for k, v in pre.items():
                if self.fill is None or not v.numel() or not bool((_bits(v) == self.fill).all()):
                    snap[k] = v
            ret = fn(*a, **kw)
            for k, v in sig.bind(*a, **kw).arguments.items():
                if k not in SCRATCH_ARGS and not (name == "triplet_plan" and k == "out"):       # (the caller's plan buffer: the same blob)
                    self._tensors(k, v, snap)
            if name not in WORKSPACE_RETURNS:
                self._tensors("return", ret, snap)
            if name in BLOB_RETURNS:
                snap = {k: v for k, v in snap.items() if not (k.startswith("return") and v.dtype == torch.uint8)}
            self.records.append((name, snap))
            return ret
        return wrapper

    def __enter__(self):
        import types
        from pda_amd import ops
        for name, fn in list(vars(ops).items()):
            if isinstance(fn, types.FunctionType) and fn.__module__ == ops.__name__ and not name.startswith("_"):
                self._saved[name] = fn
                setattr(ops, name, self._wrap(name, fn))
        return self

    def __exit__(self, *exc):
        from pda_amd import ops
        for name, fn in self._saved.items():
            setattr(ops, name, fn)
        self._saved = {}
        return False


def _bits(t):
    flat = t.contiguous().reshape(-1)
    if flat.numel() <= 1:                  # (an expanded scalar keeps stride 0 through contiguous())
        flat = flat.clone().as_strided((flat.numel(),), (1,))
    return flat.view(torch.uint8)


# The entry points that sum floats with atomics (gradient accumulators, loss words, the unordered metrics): the same inputs give results that
# differ in the last bits run after run, under ONE fill (measured on an MI355X: 1e-8 .. 3e-6).  Only these, and calls whose inputs already
# differ because of them, are compared at a tolerance; every other call with equal inputs must give equal bits under every fill.
ATOMIC_STEPS = frozenset((
    "bpr_step", "bpr_step_bf16", "bpr_step_shard", "sgd_step_exact", "apply_user_grads", "adam_step", "adam_lazy", "adam_lazy_dev",
    "bpr_step_and_sample", "bpr_train_steps", "temp_pop_grads", "temp_pop_adam_step", "dice_grads", "dice_adam_step", "ips_grads",
    "ips_adam_step", "macr_grads", "macr_adam_step", "ssm_step", "ssm_adam_step", "inbatch_step", "inbatch_adam_step", "fullsm_step",
    "fullsm_adam_step", "dau_step", "dau_adam_step", "pcc_grads", "pcc_adam_step", "gcn_reg", "metrics_sums", "metrics_sums_deep"))


def same_records(a, b, what, rtol=None, atol=None, outliers=None):
    """Asserts that two Recorder.records agree: the same calls in the same order, integer tensors equal, floating tensors equal bit for bit
    (NaN payloads included) or, with rtol / atol given (a result reduced with float atomics), within that tolerance.
    outliers = (largest fraction of elements outside the tolerance, largest error of any element): tests/test_gpu_bpr_step.py's adam_close, for
    tables behind Adam steps on atomically summed gradients (a gradient component of the size of Adam's epsilon turns the order of the adds
    into 1e-5 .. 1e-4 of the element)."""
    assert [n for n, _ in a] == [n for n, _ in b], "%s: the two runs made different calls" % what
    found = []                             # every difference (the first dozen are reported), not the first alone
    for i, ((name, x), (_, y)) in enumerate(zip(a, b)):
        for k in set(x) ^ set(y):          # (an output buffer that held nothing but the fill in one run only: no input in either)
            if k.startswith("in:"):
                x.pop(k, None), y.pop(k, None)
        assert sorted(x) == sorted(y), "%s: call %d (%s) recorded %s and %s" % (what, i, name, sorted(x), sorted(y))
        inputs_equal = all(x[k].shape == y[k].shape and x[k].dtype == y[k].dtype and torch.equal(_bits(x[k]), _bits(y[k]))
                           for k in x if k.startswith("in:"))
        tolerant = rtol is not None and (name in ATOMIC_STEPS or not inputs_equal)
        for label in x:
            if label.startswith("in:"):
                continue
            s, t = x[label], y[label]
            where = "%s: call %d, %s(...) %s" % (what, i, name, label)
            assert s.shape == t.shape and s.dtype == t.dtype, where
            if tolerant and s.is_floating_point():
                try:
                    torch.testing.assert_close(t.double(), s.double(), rtol=rtol, atol=atol, equal_nan=True)
                except AssertionError as e:
                    if outliers is not None and bool((torch.isnan(s) == torch.isnan(t)).all()) and bool((torch.isinf(s) == torch.isinf(t)).all()):
                        err = torch.nan_to_num((t.double() - s.double()).abs(), nan=0.0, posinf=0.0, neginf=0.0)
                        out = err > atol + rtol * torch.nan_to_num(s.double().abs(), nan=0.0, posinf=0.0)
                        if float(out.double().mean()) < outliers[0] and float(err.max()) < outliers[1]:
                            continue
                    found.append("%s is outside rtol %g, atol %g: %s" % (where, rtol, atol, " ".join(str(e).split())[:300]))
            elif not torch.equal(_bits(s), _bits(t)):
                diff = (_bits(s) != _bits(t)).nonzero().reshape(-1) // max(1, s.element_size())
                idx = torch.unique(diff)[:8].tolist()
                flat_s, flat_t = s.contiguous().reshape(-1), t.contiguous().reshape(-1)
                found.append("%s differs with the fill at %d of %d elements; first at flat index %s: %s vs %s" % (
                    where, torch.unique(diff).numel(), s.numel(), idx, flat_s[idx].tolist(), flat_t[idx].tolist()))
    assert not found, "%d differences:\n  " % len(found) + "\n  ".join(found[:12])
