"""The item prep image, restated: layouts, decoders, float64 reference conditions and an fp32 emulation of both preps.  Shared by
test_prep_host.py (CPU) and test_gpu_item_prep.py (GPU).  No tests in here.

The prep blob is what makes the pre-filter of generation 3, generation 4, the huge geometry and the funnel rigorous: padded norms, rounding-residual
norms, 1/pop rounded down, per-half-tile and suffix maxima, null items in the padding, the bf16 / fp16 images at the swizzled places the MFMA waves
read.  check_prep4 / check_prep3 hold every field of a decoded blob to a condition computed from (I, pop, order) alone, in float64 where the
condition is an inequality and bit for bit where the field is a rounding or a maximum of stored values.

Layouts: prep4_layout restates pda_amd/csrc/pda_v4_shared.h:prep4_layout, prep3_layout restates pda_amd/csrc/pda_score_prep.hip:prep_layout.  They
are interfaces between kernels and can only be restated; their totals are held to the library's *_bytes entry points on the CPU.

The caps (none is hand-picked):
  PAD = 1.0009765625 * 1.0001, the pad every kernel and decided_tail_cases.padded_norm state.
  cap(d) = PAD * sqrt(1 + gamma_d) * (1 + u)^4 with u = 2^-24 and gamma_d = d u / (1 - d u): in a d-term fp32 sum of squares every term meets one
  rounding of its square and at most d - 1 roundings of additions whatever the order of summation (a fused multiply-add only removes roundings), so
  the computed sum is at most (1 + gamma_d) times the exact one; the square root, the two multiplications by the pad's factors and the rounding of
  1.0001 to fp32 are one (1 + u) each.
  Gradual underflow: a square below 2^-126 is rounded to a multiple of 2^-149, an ABSOLUTE error of at most 2^-150 per term.  The rows scaled by
  1e-18 have such squares (and every row has such squared residuals), so the sum of squares is compared with quantum(d) = d 2^-149 of absolute slack:
  at most 6e-22 in a norm at d = 256.  Overflow or underflow of the SUM of squares is out of scope (include/pda_hip.h states the precondition).
  Products pop * norm * 1.000001f add two roundings and the rounding of the constant: below the 1.000002 the conditions allow.
"""
import collections
import zlib

import numpy as np

F = np.float32
U24 = 2.0 ** -24
PAD = 1.0009765625 * 1.0001
DIMS = (64, 128, 256)
LAYOUT_N = (1, 63, 64, 65, 4097, 65600)


def cap(d):
    """largest stored norm / exact norm of a correct fp32 prep (derivation: module docstring)"""
    g = d * U24 / (1.0 - d * U24)
    return PAD * np.sqrt(1.0 + g) * (1.0 + U24) ** 4


def quantum(d):
    return d * 2.0 ** -149


def norm_upper(x, d):
    """the tightness bound of a stored padded norm whose exact value is x (float64)"""
    return cap(d) * np.sqrt(x * x + quantum(d))


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------------------
def _al(x):
    return (x + 255) & ~255


def prep4_layout(n, d):
    """byte offsets of pda_item_prep4_* / pda_item_prep7_* blobs; a row of `rows` is 2 d + 48 bytes"""
    nt = (n + 63) // 64
    L = {"n_tiles": nt, "row_bytes": 2 * d + 48, "hdr": 0, "pos_of": 256}
    L["sufA"] = L["pos_of"] + _al(n * 4)
    L["sufB"] = L["sufA"] + _al(nt * 4)
    L["sufR"] = L["sufB"] + _al(nt * 4)
    L["rows"] = L["sufR"] + _al(nt * 4)
    L["rows5"] = _al(L["rows"] + nt * 64 * L["row_bytes"])
    L["meta5"] = L["rows5"] + _al(nt * 2 * 64 * d)
    L["pinfo"] = L["meta5"] + _al(nt * 2 * 16)
    L["total"] = L["pinfo"] + _al(nt * 64 * 16)
    return L


def gen3_planes(bf16, ordered):
    return (1 if ordered else 0) if bf16 else 2


def prep3_layout(n, d, ordered, n_planes):
    """byte offsets of pda_item_prep_* / pda_item_prep_ordered_* blobs"""
    plane, vec = _al(n * d * 2), _al(n * 4)
    L = {"n_tiles": (n + 31) // 32, "plane": plane, "norm": 0, "nmax": vec}
    off = vec + 256
    if ordered:
        tiles = _al(L["n_tiles"] * 4)
        L["pop_p"] = off
        L["order"] = L["pop_p"] + vec
        L["pos_of"] = L["order"] + vec
        L["sufA"] = L["pos_of"] + vec
        L["sufB"] = L["sufA"] + tiles
        off = L["sufB"] + tiles
    L["bex"] = off
    off += _al(n * 32)
    L["hi"], L["lo"] = off, off + plane
    L["total"] = off + n_planes * plane
    return L


def layout_total(entry, n, d):
    """the restated total behind each of the library's *_bytes entry points"""
    if entry == "pda_item_prep4_bytes":
        return prep4_layout(n, d)["total"]
    ordered, planes = {"pda_item_prep_bytes": (False, 2), "pda_item_prep_ordered_bytes": (True, 2), "pda_item_prep_bf16_bytes": (False, 0),
                       "pda_item_prep_ordered_bf16_bytes": (True, 1)}[entry]
    return prep3_layout(n, d, ordered, planes)["total"]


# ---- number formats --------------------------------------------------------------------------------------------------------------------------------
def bf16_to_f64(bits):
    return (np.asarray(bits).astype(np.uint32) << 16).view(F).astype(np.float64)


def bf16_to_f32(bits):
    return (np.asarray(bits).astype(np.uint32) << 16).view(F)


def f16_to_f64(bits):
    return np.asarray(bits, dtype=np.uint16).view(np.float16).astype(np.float64)


def bf16_rne(x):
    """fp32 -> bf16 bits, round to nearest even (finite x)"""
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_rtz(x):
    return (np.ascontiguousarray(x, dtype=F).view(np.uint32) >> 16).astype(np.uint16)


def bf16_up(x):
    """smallest bf16 >= x (x >= 0, finite)"""
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32)
    return ((u >> 16) + ((u & 0xFFFF) != 0)).astype(np.uint16)


def f16_rne_clamped(x, clamp=True):
    x = np.asarray(x, dtype=F)
    if clamp:
        x = np.minimum(np.maximum(x, F(-65504.0)), F(65504.0))
    with np.errstate(over="ignore"):
        return x.astype(np.float16).view(np.uint16)


def pieces_sum(p1, p2, p3):
    """the three bf16 pieces of (1/pop)' -> their exact sum (24 significant bits: exact in float64)"""
    return bf16_to_f64(p1) + bf16_to_f64(p2) + bf16_to_f64(p3)


def swizzle5(img, d):
    """[H, 32, d] u16 <-> the same half-tiles with the 16-byte chunk e of row r at chunk e ^ sw(r) (an involution: it swizzles and de-swizzles)"""
    H = img.shape[0]
    r = np.arange(32)
    sw = (r & 15) if d >= 128 else ((r >> 1) & 7)
    idx = np.arange(d // 8)[None, :] ^ sw[:, None]
    return img.reshape(H, 32, d // 8, 8)[:, r[:, None], idx].reshape(H, 32, d)


# ---- decoding --------------------------------------------------------------------------------------------------------------------------------------
def _view(blob, off, count, dtype):
    return np.frombuffer(blob, dtype=dtype, count=count, offset=off).copy()


def decode_prep4(blob, n, d):
    """every field the layout names, as plain arrays (blob: bytes / uint8 array of pda_item_prep4_bytes(n, d))"""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    L = prep4_layout(n, d)
    assert blob.size == L["total"], (blob.size, L["total"])
    nt, rb = L["n_tiles"], L["row_bytes"]
    rows = _view(blob, L["rows"], nt * 64 * rb, np.uint8).reshape(nt * 64, rb)
    f = {"hdr": _view(blob, L["hdr"], 4, np.int32), "pos_of": _view(blob, L["pos_of"], n, np.int32)}
    for k in ("sufA", "sufB", "sufR"):
        f[k] = _view(blob, L[k], nt, F)
    f["row"] = np.ascontiguousarray(rows[:, : 2 * d]).view(np.uint16)
    f["lo"] = np.ascontiguousarray(rows[:, 2 * d: 2 * d + 16]).view(np.uint16)
    f["hi"] = np.ascontiguousarray(rows[:, 2 * d + 16: 2 * d + 32]).view(np.uint16)
    f["tail"] = np.ascontiguousarray(rows[:, 2 * d + 32:]).view(np.uint32)
    f["rows5_raw"] = _view(blob, L["rows5"], nt * 2 * 32 * d, np.uint16).reshape(nt * 2, 32, d)
    f["meta5"] = _view(blob, L["meta5"], nt * 2 * 4, F).reshape(nt * 2, 4)
    f["pinfo"] = _view(blob, L["pinfo"], nt * 64 * 4, np.uint32).reshape(nt * 64, 4)
    return f


def decode_prep3(blob, n, d, bf16, ordered, with_pop):
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    planes = gen3_planes(bf16, ordered)
    L = prep3_layout(n, d, ordered, planes)
    assert blob.size == L["total"], (blob.size, L["total"])
    f = {"norm": _view(blob, L["norm"], n, F), "hdr": _view(blob, L["nmax"], 2, np.int32), "bex": _view(blob, L["bex"], n * 16, np.uint16).reshape(n, 16)}
    if ordered:
        if with_pop:
            f["pop_p"] = _view(blob, L["pop_p"], n, F)
        f["order"] = _view(blob, L["order"], n, np.int32)
        f["pos_of"] = _view(blob, L["pos_of"], n, np.int32)
        f["sufA"] = _view(blob, L["sufA"], L["n_tiles"], F)
        f["sufB"] = _view(blob, L["sufB"], L["n_tiles"], F)
    if planes > 0:
        f["hi_plane"] = _view(blob, L["hi"], n * d, np.uint16).reshape(n, d)
    if planes > 1:
        f["lo_plane"] = _view(blob, L["lo"], n * d, np.uint16).reshape(n, d)
    return f


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------
# kind: "prep4" (generation 4), "prep7" (the funnel's: no popularity, fp16 image), "gen3o" (generation 3 ordered), "gen3" (generation 3 in item order)
Case = collections.namedtuple("Case", "kind d bf16 n popk orderk plant")
POPS = (None, "pow", "zeros", "tiny", "nan", "ones")
ORDERS = (None, "random", "visiting")


def case_id(c):
    return "%s-d%d-%s-n%d-pop_%s-ord_%s%s" % (c.kind, c.d, "bf16" if c.bf16 else "f32", c.n, c.popk, c.orderk, "-" + c.plant if c.plant else "")


def gpu_cases():
    """A reasoned subset, not the product (about one hundred):
      every d x table type x n in {65, 4097} with a popularity and a random order, for each prep;
      n in {1, 63, 64} for every d (generation 4), at d = 64 for the other preps;
      every popularity kind and every order kind at d = 64 and once at d = 256;
      n = 65 600 (1 025 tiles of 64, 2 050 of 32) at d = 64 with the largest |pop| ||i|| planted at a chunk seam."""
    cs = []
    for d in DIMS:
        for bf in (False, True):
            for n in (65, 4097):
                cs += [Case("prep4", d, bf, n, "pow", "random", None), Case("prep7", d, bf, n, None, "random", None),
                       Case("gen3o", d, bf, n, "pow", "random", None)]
        for n in (1, 63, 64):
            cs.append(Case("prep4", d, False, n, "pow", "random", None))
    for n in (1, 63, 64):
        cs += [Case("prep7", 64, False, n, None, "random", None), Case("gen3o", 64, False, n, "pow", "random", None)]
    for n in (1, 63, 64, 65, 4097):
        cs.append(Case("gen3", 64, False, n, None, None, None))
    cs += [Case("gen3", 64, True, 65, None, None, None), Case("gen3", 128, False, 65, None, None, None), Case("gen3", 256, False, 4097, None, None, None)]
    for popk in (None, "zeros", "tiny", "nan", "ones"):
        cs += [Case("prep4", 64, False, 4097, popk, "random", None), Case("gen3o", 64, False, 4097, popk, "random", None),
               Case("prep4", 256, False, 65, popk, "random", None)]
    cs += [Case("prep4", 64, True, 65, "nan", "random", None), Case("gen3o", 64, True, 65, None, "random", None)]
    for orderk in (None, "visiting"):
        cs += [Case("prep4", 64, False, 4097, "pow", orderk, None), Case("prep4", 256, False, 4097, "pow", orderk, None)]
    cs += [Case("prep4", 64, False, 65, None, None, None), Case("prep4", 64, False, 4097, None, "visiting", None),
           Case("prep4", 64, False, 4097, "nan", "visiting", None),
           Case("prep7", 64, False, 4097, None, "visiting", None), Case("prep7", 256, False, 65, None, "visiting", None),
           Case("gen3o", 64, False, 4097, "pow", "visiting", None), Case("gen3o", 64, False, 4097, None, "visiting", None),
           Case("gen3o", 256, False, 65, "pow", "visiting", None)]
    # the seam of suffix_max4_kernel / suffix_max_kernel (two / three tiles per thread, threads left empty): the largest |pop| ||i|| in the last tile, in
    # tile 1 024 (generation 4: the last one too, its first position; generation 3: a tile of 32 in mid-catalogue) and at the end of the chunk in front
    for plant in ("last", "t1024", "t1023"):
        cs += [Case("prep4", 64, False, 65600, "pow", None, plant), Case("gen3o", 64, False, 65600, "pow", "identity", plant)]
    cs.append(Case("prep7", 64, False, 65600, None, "identity", "last"))
    assert len(set(cs)) == len(cs)
    return cs


def mutant_cases():
    """where the mutants are shown to fail: small, every mechanism present"""
    return [Case("prep4", 64, False, 65, "pow", "random", None), Case("prep4", 128, False, 4097, "zeros", "random", None),
            Case("prep4", 64, False, 4097, "tiny", "visiting", None), Case("prep4", 64, False, 4097, "nan", "random", None),
            Case("prep7", 64, False, 4097, None, "random", None), Case("gen3o", 64, False, 4097, "pow", "random", None)]


def plant_position(c):
    tile = 64 if c.kind in ("prep4", "prep7") else 32
    return {"last": c.n - 1, "t1024": 1024 * tile, "t1023": 1023 * tile + tile - 1}[c.plant]


def make_inputs(c):
    """-> dict(I32 [n, d] float32 values of the table, Ibits u16 [n, d] or None, pop f32 [n] or None, order i32 [n] or None ("visiting": the caller's))

    Rows: N(0, 0.1); from n = 8 on some rows exactly zero, some scaled by 1e-18, some by 1e4, one row with an entry of 7e4 (the fp16 clamp of prep7).
    The squares of the 1e-18 rows are partly subnormal (gradual underflow, see quantum()); their sum and the sums of the 1e4 rows stay normal: overflow
    and underflow of the sum of squares are out of scope."""
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
    n, d = c.n, c.d
    I = (rng.standard_normal((n, d)) * 0.1).astype(F)
    if c.plant is None and n >= 8:
        k = max(1, n // 50)
        pick = rng.permutation(n)
        I[pick[:k]] = 0.0
        I[pick[k: 2 * k]] *= F(1e-18)
        I[pick[2 * k: 3 * k]] *= F(1e4)
        I[pick[3 * k], rng.integers(d)] = F(7e4)
        I[pick[3 * k + 1], 0] = F(-7e4)
    pop = None
    if c.popk is not None:
        pop = (rng.random(n) ** 0.22).astype(F)
        few = rng.permutation(n)[: max(1, n // 20)]
        if c.popk == "zeros":
            pop[few] = 0.0
        elif c.popk == "tiny":
            pop[few] = (rng.random(len(few)) * 5e-7).astype(F)          # well below 1e-6 (1 - 2^-20): 1/pop is capped
            pop[few[0]] = F(1e-30)
        elif c.popk == "nan":
            pop[few] = np.nan
        elif c.popk == "ones":
            pop[:] = 1.0
    if c.plant is not None:                                              # position = item id (natural / identity order)
        p = plant_position(c)
        I[p] *= F(3.0)
        if pop is not None:
            pop[p] = 1.0
    bits = None
    if c.bf16:
        bits = bf16_rne(I)
        I = bf16_to_f32(bits)
    order = None
    if c.orderk == "random":
        order = rng.permutation(n).astype(np.int32)
    elif c.orderk == "identity":
        order = np.arange(n, dtype=np.int32)
    elif c.orderk == "visiting":
        order = "visiting"
    return {"I32": I, "Ibits": bits, "pop": pop, "order": order}


def host_visiting_order(I32, pop):
    """as ops.visiting_order chooses it: most popular first, largest norm first without a popularity (any permutation serves the checks)"""
    key = np.abs(pop) if pop is not None else np.sqrt((I32.astype(np.float64) ** 2).sum(1))
    return np.argsort(-np.nan_to_num(key, nan=np.inf), kind="stable").astype(np.int32)


# ---- fp32 emulation --------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("pad_dropped", "pad_twice", "norm_half_row", "suffix_exclusive", "tile_max_32_of_64", "ipop_nearest", "ipop_uncapped", "image_rtz",
           "image_unscaled", "residual_unscaled", "padding_pop_zero", "nan_ranked", "pos_of_off_by_one", "swizzle_omitted", "fp16_clamp_omitted",
           "meta5_other_half")


def sumsq32(X, d):
    """the kernels' fp32 sum of squares of a row: eight elements per thread, then an XOR butterfly over the row's d / 8 threads"""
    m, T = X.shape[0], d // 8
    Y = np.ascontiguousarray(X, dtype=F).reshape(m, T, 8)
    ss = np.zeros((m, T), F)
    with np.errstate(under="ignore"):
        for k in range(4):
            a, b = Y[:, :, k], Y[:, :, 4 + k]
            ss = ss + (a * a + b * b)
        lanes, o = np.arange(T), T // 2
        while o > 0:
            ss = ss + ss[:, lanes ^ o]
            o //= 2
    return ss[:, 0]


def padded32(ss, defect=None):
    v = np.sqrt(ss.astype(F))
    if defect == "pad_dropped":
        return v
    v = v * F(1.0009765625) * F(1.0001)
    return v * F(1.0009765625) * F(1.0001) if defect == "pad_twice" else v


def ipop_pieces(popv, defect=None):
    """(1/pop)' = min(fl(fl(1/pop) 0.9999995f), 1e6), 1e6 for pop <= 0 or NaN, split into three truncated bf16 pieces"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = F(1.0) / popv
        if defect != "ipop_nearest":
            q = q * F(0.9999995)
        if defect != "ipop_uncapped":
            q = np.minimum(q, F(1.0e6))
        ip = np.where(popv > 0, q, F(1.0e6)).astype(F)
        if defect == "ipop_uncapped":
            ip = np.minimum(ip, F(3.0e38))               # (finite, so that the split stays exact)
    b1 = ip.view(np.uint32) & 0xFFFF0000
    r1 = (ip - b1.view(F)).astype(F)
    b2 = r1.view(np.uint32) & 0xFFFF0000
    r2 = (r1 - b2.view(F)).astype(F)
    return (b1 >> 16).astype(np.uint16), (b2 >> 16).astype(np.uint16), (r2.view(np.uint32) >> 16).astype(np.uint16)


def test_operands(popv, v, real, has_pop, defect=None):
    """the 16 bf16 of the folded threshold test per position -> (lo [m, 8], hi [m, 8]); real: False on padding rows"""
    m = len(v)
    p1, p2, p3 = np.full(m, 0x3F80, np.uint16), np.zeros(m, np.uint16), np.zeros(m, np.uint16)
    k1, k2 = np.full(m, bf16_up(F(8.0e-6)), np.uint16), np.zeros(m, np.uint16)
    if has_pop:
        p1, p2, p3 = ipop_pieces(popv, defect)
        k1 = np.where(np.isnan(popv), 0xFF61, 0x3F80).astype(np.uint16)
        k2 = np.full(m, bf16_up(F(8.0e-6)), np.uint16)
    p1, p2, p3 = np.where(real, p1, 0x3F80), np.where(real, p2, 0), np.where(real, p3, 0)
    k1, k2 = np.where(real, k1, 0xFF61), np.where(real, k2, 0)
    z = np.zeros(m, np.uint16)
    lo = np.stack([p1, p2, p1, p2, p3, p1, p3, p2], 1).astype(np.uint16)
    hi = np.stack([k1, k2, np.where(real, bf16_up(v), 0), z, z, z, z, z], 1).astype(np.uint16)
    return lo, hi


def _fmax_tiles(x, tile, n_tiles, defect=None):
    """fmaxf over the tiles of a position array (NaN and padding contribute nothing), starting from 0"""
    y = np.zeros(n_tiles * tile, F)
    y[: len(x)] = x
    y = y.reshape(n_tiles, tile)
    if defect == "tile_max_32_of_64":
        y = y[:, : tile // 2]
    if defect == "nan_ranked":
        return np.maximum(y.max(1), F(0))                      # (max and maximum hand a NaN on)
    return np.fmax(np.nan_to_num(y, nan=0.0).max(1), F(0)).astype(F)


def _suffix(x, defect=None):
    s = np.maximum.accumulate(x[::-1])[::-1].astype(F)
    if defect == "suffix_exclusive":
        s = np.concatenate([s[1:], np.zeros(1, F)])
    return s


def emulate_prep4(I32, pop, order, d, f16img=False, defect=None):
    """pda_item_prep4_* (f16img: pda_item_prep7_*) in numpy fp32 -> the dict decode_prep4 returns"""
    n = I32.shape[0]
    nt = (n + 63) // 64
    m = nt * 64
    src = np.arange(n, dtype=np.int32) if order is None else np.asarray(order, dtype=np.int32)
    has_pop = pop is not None
    X = np.zeros((m, d), F)
    X[:n] = I32[src]
    real = np.arange(m) < n
    popv = np.ones(m, F)
    if has_pop:
        popv[:n] = pop[src]
    pv = np.where(np.isnan(popv), F(0), popv).astype(F)
    Xn = X.copy()
    if defect == "norm_half_row":
        Xn[:, d // 2:] = 0
    v = np.where(real, padded32(sumsq32(Xn, d), defect), F(0)).astype(F)
    with np.errstate(under="ignore", invalid="ignore"):
        Xs = X if defect == "image_unscaled" else (X * pv[:, None]).astype(F)
        Xr = X if defect == "residual_unscaled" else Xs
        if f16img:
            img = f16_rne_clamped(Xs, clamp=defect != "fp16_clamp_omitted")
            back = f16_rne_clamped(Xr, clamp=defect != "fp16_clamp_omitted").view(np.float16).astype(F)
        else:
            rnd = bf16_rtz if defect == "image_rtz" else bf16_rne
            img, back = rnd(Xs), bf16_to_f32(rnd(Xr))
        res = (Xr - back).astype(F)
        res = np.where(np.isfinite(res), res, F(0))
    rv = np.where(real, padded32(sumsq32(res, d)), F(0)).astype(F)
    f = {"hdr": np.array([0, int(has_pop), int(order is not None), int(f16img)], np.int32)}
    pos_of = np.zeros(n, np.int32)
    pos_of[src] = np.arange(n, dtype=np.int32) + (1 if defect == "pos_of_off_by_one" else 0)
    f["pos_of"] = pos_of
    f["row"] = np.where(real[:, None], bf16_rne(X), 0).astype(np.uint16)
    f["lo"], f["hi"] = test_operands(popv, v, real, has_pop, defect)
    tail = np.zeros((m, 4), np.uint32)
    tail[:, 0] = np.where(real, (popv if has_pop else np.ones(m, F)).view(np.uint32), 0 if defect == "padding_pop_zero" else 0x7FC00000)
    tail[:n, 1] = src
    tail[:, 2] = v.view(np.uint32)
    tail[:, 3] = rv.view(np.uint32)
    f["tail"] = tail
    f["pinfo"] = tail[:, [2, 3, 1, 0]].copy()
    logical = np.where(real[:, None], img, 0).astype(np.uint16).reshape(nt * 2, 32, d)
    f["rows5_raw"] = logical if defect == "swizzle_omitted" else swizzle5(logical, d)
    with np.errstate(under="ignore", invalid="ignore"):
        pn = (pv * v * F(1.000001)).astype(F)
        meta = np.zeros((nt * 2, 4), F)
        meta[:, 0] = _fmax_tiles(pv[:n], 32, nt * 2) if has_pop else 0
        meta[:, 1] = _fmax_tiles(pn[:n], 32, nt * 2)
        meta[:, 2] = _fmax_tiles(rv[:n], 32, nt * 2)
        f["meta5"] = meta.reshape(nt, 2, 4)[:, ::-1].reshape(nt * 2, 4).copy() if defect == "meta5_other_half" else meta
        tp = tail[:, 0].view(F)                                    # (the bound kernel reads the stored popularity: NaN on null items)
        ok = ~np.isnan(tp) if defect != "nan_ranked" else np.ones(m, bool)
        pa = np.abs(tp) if has_pop else np.zeros(m, F)
        if defect != "nan_ranked":
            pa = np.where(ok, pa, F(0))
        f["sufA"] = _suffix(_fmax_tiles(pa, 64, nt, defect), defect)
        f["sufB"] = _suffix(_fmax_tiles((pa * v * F(1.000001)).astype(F), 64, nt, defect), defect)
        f["sufR"] = _suffix(_fmax_tiles(np.where(ok, v, F(0)), 64, nt, defect), defect)
    return f


def emulate_prep3(I32, pop, order, d, bf16, defect=None):
    """pda_item_prep_* (order None, no popularity) / pda_item_prep_ordered_* in numpy fp32 -> the dict decode_prep3 returns"""
    n = I32.shape[0]
    ordered, has_pop = order is not None, pop is not None
    src = np.arange(n, dtype=np.int32) if order is None else np.asarray(order, dtype=np.int32)
    X = np.ascontiguousarray(I32[src], dtype=F)
    popv = pop[src].astype(F) if has_pop else np.ones(n, F)
    Xn = X.copy()
    if defect == "norm_half_row":
        Xn[:, d // 2:] = 0
    v = padded32(sumsq32(Xn, d), defect).astype(F)
    f = {"norm": v, "hdr": np.array([int(v.max().view(np.int32)), 0], np.int32)}
    lo, hi = test_operands(popv, v, np.ones(n, bool), has_pop, defect)
    f["bex"] = np.concatenate([lo, hi], 1)
    if ordered:
        if has_pop:
            f["pop_p"] = popv
        f["order"] = src.copy()
        pos_of = np.zeros(n, np.int32)
        pos_of[src] = np.arange(n, dtype=np.int32) + (1 if defect == "pos_of_off_by_one" else 0)
        f["pos_of"] = pos_of
        nt = (n + 31) // 32
        with np.errstate(under="ignore", invalid="ignore"):
            pa = np.abs(popv) if has_pop else np.zeros(n, F)
            pb = (pa * v * F(1.000001)).astype(F) if has_pop else v
            f["sufA"] = _suffix(_fmax_tiles(pa, 32, nt, defect), defect)
            f["sufB"] = _suffix(_fmax_tiles(pb, 32, nt, defect), defect)
    planes = gen3_planes(bf16, ordered)
    rnd = bf16_rtz if defect == "image_rtz" else bf16_rne
    if planes > 0:
        f["hi_plane"] = rnd(X)
    if planes > 1:
        f["lo_plane"] = bf16_rne((X - bf16_to_f32(f["hi_plane"])).astype(F))
    return f


def emulate(c, inp, order, defect=None):
    if c.kind in ("prep4", "prep7"):
        return emulate_prep4(inp["I32"], inp["pop"], order, c.d, f16img=c.kind == "prep7", defect=defect)
    return emulate_prep3(inp["I32"], inp["pop"], order, c.d, c.bf16, defect=defect)


# ---- the conditions --------------------------------------------------------------------------------------------------------------------------------
class Report:
    """failed conditions by name, and the smallest and largest observed ratio per field (recorded, never a threshold)"""

    def __init__(self):
        self.failed, self.ratio = {}, {}          # ratio: name -> (smallest, largest)

    def need(self, name, ok, detail=""):
        ok = np.asarray(ok)
        if not ok.all():
            where = np.argwhere(~ok)[:3].tolist() if ok.ndim else []
            self.failed.setdefault(name, "%s %d of %d first at %s" % (detail, int((~ok).sum()), ok.size, where))

    def worst(self, name, num, den):
        num, den = np.asarray(num, dtype=np.float64).ravel(), np.asarray(den, dtype=np.float64).ravel()
        sel = den > 0
        if sel.any():
            q, (lo, hi) = num[sel] / den[sel], self.ratio.get(name, (np.inf, 0.0))
            self.ratio[name] = (min(lo, float(q.min())), max(hi, float(q.max())))

    def line(self):
        return " ".join("%s %.7f..%.7f" % ((k,) + v) for k, v in sorted(self.ratio.items()))


def _bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def _same_f32(a, b):
    """bit-equal floats, any NaN equal to any NaN"""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def _tile_max64(x, tile, n_tiles):
    """float64 maximum per tile of a position array, NaN and padding contributing nothing, from 0"""
    y = np.zeros(n_tiles * tile)
    y[: len(x)] = np.nan_to_num(np.asarray(x, dtype=np.float64), nan=0.0)
    return y.reshape(n_tiles, tile).max(1)


def _suffix64(x):
    return np.maximum.accumulate(x[::-1])[::-1]


def _check_norm(R, v, true, d, what):
    v64 = v.astype(np.float64)
    R.need(what + ".sound", v64 >= true)
    R.need(what + ".tight", v64 <= norm_upper(true, d))
    R.need(what + ".zero", (v64 == 0) | (true > 0))
    R.worst(what + "/exact", v64, np.where(true > 1e-15, true, 0))          # (below: the quantum, not the pad, decides the ratio)


def _check_test_operands(R, lo, hi, popv, v, real, has_pop):
    """popv, v, real per position (popv: the popularity given, NaN as given)"""
    for a, b in ((2, 0), (3, 1), (5, 0), (6, 4), (7, 1)):
        R.need("pieces.layout", lo[:, a] == lo[:, b])
    R.need("pieces.layout", hi[:, 3:] == 0)
    S = pieces_sum(lo[:, 0], lo[:, 1], lo[:, 4])
    k8, k9, k10 = bf16_to_f64(hi[:, 0]), bf16_to_f64(hi[:, 1]), bf16_to_f64(hi[:, 2])
    eps_ok = lambda k: (k >= 8e-6) & (k < 8e-6 * (1 + 2.0 ** -7))
    v64 = v.astype(np.float64)
    if has_pop:
        p = popv.astype(np.float64)
        nan, pos = np.isnan(p) & real, real & (p > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where(pos, 1.0 / p, np.inf)
        R.need("ipop.le", ~real | (S <= inv))
        R.need("ipop.ge", ~(real & (p >= 1e-6)) | (S >= inv * (1 - 2.0 ** -20)))
        R.need("ipop.cap", ~real | (S <= 1e6))
        R.need("ipop.cap", ~(real & ~(p >= 1e-6 * (1 - 2.0 ** -20))) | (S == 1e6))      # 0, NaN, below 1e-6: the cap itself
        R.worst("S*pop", np.where(pos & (p >= 1e-6), S * p, 0), (pos & (p >= 1e-6)).astype(np.float64))
        R.need("k8", ~(real & ~nan) | (k8 == 1.0))
        R.need("k8", ~nan | (k8 <= -1e38))
        R.need("k9", ~real | eps_ok(k9))
    else:
        R.need("ipop.raw", ~real | (S == 1.0))
        R.need("k8", ~real | eps_ok(k8))
        R.need("k9", ~real | (k9 == 0))
    R.need("k8", real | (k8 <= -1e38))
    R.need("k9", real | (k9 == 0))
    R.need("ipop.raw", real | (S == 1.0))
    R.need("k10", ~real | ((k10 >= v64) & ((k10 < v64 * (1 + 2.0 ** -7)) | ((v64 == 0) & (k10 == 0)))))
    R.need("k10", real | (k10 == 0))


def _true_values(I32, pop, src, m, d, f16img):
    """float64 truths per visiting position 0 .. m - 1 (padding: zeros), from the inputs alone"""
    n = len(src)
    X = np.zeros((m, d), F)
    X[:n] = I32[src]
    popv = np.ones(m, F)
    if pop is not None:
        popv[:n] = pop[src]
    pv = np.where(np.isnan(popv), F(0), popv).astype(F)
    with np.errstate(under="ignore"):
        Xs = (X * pv[:, None]).astype(F)                                # i' = fl32(pop i)
    if f16img:
        img = f16_rne_clamped(Xs)
        back = f16_to_f64(img)
    else:
        img = bf16_rne(Xs)
        back = bf16_to_f64(img)
    X64 = X.astype(np.float64)
    res = Xs.astype(np.float64) - back
    return {"X": X, "popv": popv, "pv": pv, "img": img, "norm": np.sqrt((X64 * X64).sum(1)), "res2": (res * res).sum(1)}


def check_prep4(f, I32, pop, order, d, f16img=False):
    """every condition on a decoded generation-4 / funnel prep -> Report"""
    R = Report()
    n = I32.shape[0]
    nt = (n + 63) // 64
    m = nt * 64
    has_pop = pop is not None
    src = np.arange(n, dtype=np.int32) if order is None else np.asarray(order, dtype=np.int32)
    real = np.arange(m) < n
    T = _true_values(I32, pop, src, m, d, f16img)
    R.need("hdr", f["hdr"] == np.array([0, int(has_pop), int(order is not None), int(f16img)]), "header words")
    inv = np.zeros(n, np.int32)
    inv[src] = np.arange(n, dtype=np.int32)
    R.need("pos_of", f["pos_of"] == inv)
    tail = f["tail"]
    v, rv = tail[:, 2].view(F), tail[:, 3].view(F)
    # norms
    _check_norm(R, v[:n], T["norm"][:n], d, "norm")
    rv64, res2 = rv[:n].astype(np.float64), T["res2"][:n]
    R.need("rnorm.sound", rv64 >= np.sqrt(np.maximum(res2 - quantum(d), 0.0)))
    R.need("rnorm.tight", rv64 <= cap(d) * np.sqrt(res2 + quantum(d)))
    R.need("rnorm.zero", (rv64 == 0) | (res2 > 0))
    R.worst("rnorm/exact", rv64, np.where(res2 > 1e-30, np.sqrt(res2), 0))
    # images
    R.need("rows.bits", f["row"] == np.where(real[:, None], bf16_rne(T["X"]), 0))
    rows5 = swizzle5(f["rows5_raw"], d).reshape(m, d)
    R.need("image.bits", rows5 == np.where(real[:, None], T["img"], 0))
    dead = ~real | np.isnan(T["popv"])
    R.need("image.zero", (rows5[dead] & 0x7FFF) == 0)
    # the folded test's operands
    _check_test_operands(R, f["lo"], f["hi"], T["popv"], v, real, has_pop)
    # tail / pinfo
    R.need("tail.pop", ~real | _same_f32(tail[:, 0].view(F), T["popv"] if has_pop else np.ones(m, F)))
    R.need("tail.id", tail[:n, 1] == src.astype(np.uint32))
    R.need("tail.padding", real | ((tail[:, 0] & 0x7FFFFFFF) > 0x7F800000), "padding pop must be NaN")
    R.need("tail.padding", real[:, None] | (tail[:, 1:] == 0), "padding id and norms must be 0")
    R.need("pinfo", f["pinfo"] == tail[:, [2, 3, 1, 0]])
    # meta5 per 32-item half-tile
    meta = f["meta5"]
    pv64, norm = T["pv"].astype(np.float64), T["norm"]
    R.need("meta5.pmax", _same_f32(meta[:, 0], _fmax_tiles(T["pv"][:n], 32, nt * 2) if has_pop else np.zeros(nt * 2, F)))
    low = _tile_max64((pv64 * norm)[:n], 32, nt * 2)
    high = _tile_max64((pv64 * norm_upper(norm, d))[:n], 32, nt * 2) * 1.000002
    R.need("meta5.nmax.sound", meta[:, 1].astype(np.float64) >= low)
    R.need("meta5.nmax.tight", meta[:, 1].astype(np.float64) <= high)
    R.worst("nmax/exact", meta[:, 1], np.where(low > 1e-15, low, 0))
    R.need("meta5.rmax", _same_f32(meta[:, 2], _fmax_tiles(rv[:n], 32, nt * 2)))
    R.need("meta5.padding", meta[:, 3] == 0)
    empty = np.arange(nt * 2) * 32 >= n
    R.need("meta5.padding", meta[empty] == 0)
    # suffix maxima per 64-item tile
    live = real & ~np.isnan(T["popv"])
    pa = np.where(live, np.abs(T["popv"]), F(0)).astype(F) if has_pop else np.zeros(m, F)
    _check_suffix(R, f, pa, norm, 64, nt, d)
    R.need("sufR", _same_f32(f["sufR"], _suffix(_fmax_tiles(np.where(live, v, F(0)), 64, nt))))
    R.need("suf.monotone", np.diff(f["sufR"]) <= 0)
    return R


def _check_suffix(R, f, pa, norm, tile, nt, d):
    """sufA bit-equal, sufB between the float64 maximum and its cap, both non-increasing; pa: |pop| per position with 0 where nothing ranks"""
    R.need("sufA", _same_f32(f["sufA"], _suffix(_fmax_tiles(pa, tile, nt))))
    pa64 = pa.astype(np.float64)
    low = _suffix64(_tile_max64(pa64 * norm[: len(pa64)], tile, nt))
    high = _suffix64(_tile_max64(pa64 * norm_upper(norm[: len(pa64)], d), tile, nt)) * 1.000002
    b = f["sufB"].astype(np.float64)
    R.need("sufB.sound", b >= low)
    R.need("sufB.tight", b <= high)
    R.worst("sufB/exact", b, np.where(low > 1e-15, low, 0))
    R.need("suf.monotone", np.diff(f["sufA"]) <= 0)
    R.need("suf.monotone", np.diff(f["sufB"]) <= 0)


def check_prep3(f, I32, pop, order, d, bf16):
    """every condition on a decoded generation-3 prep (order None: pda_item_prep_*, which takes no popularity) -> Report"""
    R = Report()
    n = I32.shape[0]
    ordered, has_pop = order is not None, pop is not None
    src = np.arange(n, dtype=np.int32) if order is None else np.asarray(order, dtype=np.int32)
    T = _true_values(I32, pop, src, n, d, False)
    v = f["norm"]
    _check_norm(R, v, T["norm"], d, "norm")
    R.need("hdr", f["hdr"] == np.array([int(v.max().view(np.int32)), 0]), "max-norm bits, bad-order flag")
    _check_test_operands(R, f["bex"][:, :8], f["bex"][:, 8:], T["popv"], v, np.ones(n, bool), has_pop)
    if ordered:
        if has_pop:
            R.need("tail.pop", _same_f32(f["pop_p"], T["popv"]))
        R.need("tail.id", f["order"] == src)
        inv = np.zeros(n, np.int32)
        inv[src] = np.arange(n, dtype=np.int32)
        R.need("pos_of", f["pos_of"] == inv)
        nt = (n + 31) // 32
        if has_pop:
            pa = np.nan_to_num(np.abs(T["popv"]), nan=0.0).astype(F)
            _check_suffix(R, f, pa, T["norm"], 32, nt, d)
        else:                                                             # raw: sufA == 0, sufB the maximum of the stored norms
            R.need("sufA", f["sufA"] == 0)
            R.need("sufB.sound", _same_f32(f["sufB"], _suffix(_fmax_tiles(v, 32, nt))))
            R.need("suf.monotone", np.diff(f["sufB"]) <= 0)
    planes = gen3_planes(bf16, ordered)
    if planes > 0:
        R.need("rows.bits", f["hi_plane"] == bf16_rne(T["X"]))
    if planes > 1:
        R.need("rows.bits", f["lo_plane"] == bf16_rne((T["X"] - bf16_to_f32(bf16_rne(T["X"]))).astype(F)), "lo plane")
    return R


def check(c, f, inp, order):
    if c.kind in ("prep4", "prep7"):
        return check_prep4(f, inp["I32"], inp["pop"], order, c.d, f16img=c.kind == "prep7")
    return check_prep3(f, inp["I32"], inp["pop"], order, c.d, c.bf16)


def decode(c, blob, with_pop):
    if c.kind in ("prep4", "prep7"):
        return decode_prep4(blob, c.n, c.d)
    return decode_prep3(blob, c.n, c.d, c.bf16, c.kind == "gen3o", with_pop)


def named_bytes(f):
    """every byte the layout names, field by field (bit stability compares these, never the alignment gaps)"""
    return {k: np.ascontiguousarray(x).view(np.uint8).ravel() for k, x in f.items()}
