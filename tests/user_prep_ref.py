"""The user side of the pre-filter, restated: the per-block user image (uprep5_kernel, and warm4_kernel / warm_score + warm_select by contract), its
padded norms, the funnel's padded residual norms and the two Bloom filters of the train items (hist_bloom4_kernel, hist_bloom7_kernel).  Shared by
test_user_prep_host.py (CPU) and test_gpu_user_prep.py (GPU).  No tests in here.  The number formats, PAD, cap(d), quantum(d) and norm_upper are
prep_ref's.

Layout (the comment above uprep5_kernel, pda_amd/csrc/pda_v4_shared.h): the block is padded to n_pad = whole workgroups of 4 UPW rows (UPW = 256 at
d = 64 / 128, 128 at d = 256: 1 024 or 512 rows); a fragment is 64 lanes x 16 bytes = 16 users x 32 elements, fragment (wgw, u, k) starts at lane
index ((wgw NU + u) NK + k) 64 with NU = UPW / 16, NK = d / 32, wgw = row / UPW; lane l holds user 16 u + (l & 15), elements 32 k + 8 (l >> 4) .. + 7.
frag_index() is that sentence and nothing else; decode_image() gathers through it, encode_image() scatters through it.

Conditions, all computed from (U, users) alone -- check_user_image:
  image.bits      bf16 image of an fp32 table: the RNE rounding of the row, bit for bit; of a bf16 table: the table's bits; fp16 image: the RNE half of the
                  value clamped to +-65504 (a bf16 table widened first; below half's subnormal range: +-0)
  image.padding   rows n .. n_pad - 1: zero bytes
  unorm.sound     unorm^2 + quantum(d) >= ||u||^2 in float64
  unorm.tight     unorm <= norm_upper(||u||, d)
  unorm.pad       unorm >= floor(d) sqrt(||u||^2 - quantum(d)): the mirror of cap(d).  The pad is part of the contract, not only an allowance for this
                  kernel's own roundings: the sweeps multiply the stored norm on (pda_v7_funnel.h forms (uerr + unorm 2^-14) 1.001 from it) and count on
                  PAD to cover their arithmetic.  floor(d) = PAD sqrt(1 - gamma_d) (1 - u)^4 by the derivation of cap(d) with every rounding taken
                  downwards; a norm that lost one of PAD's two factors (1.0001 or 1.0009765625 left) lies below it, a correct fp32 norm cannot.
  unorm.zero      exactly 0 for a row of zeros (of either sign);  unorm.padding  exactly 0 behind the block
  uerr.*          the same five against the exact float64 norm of u - image(u), as prep_ref treats the residual norms of the item rows;
                  uerr.zero: exactly 0 where every element is representable
check_bloom:
  bloom.bits               the device words == the restated words, bit for bit (1 024 bits in 32 words per row; bits h1 = (x 0x9E3779B1) >> 22 and
                           h2 = (x 0x85EBCA6B + 0x27D4EB2F) >> 22 in uint32; generation 4: x = the item id as stored; the funnel: x =
                           pos_of[id - item_offset], ids outside [item_offset, item_offset + n_items_local) skipped)
  bloom.no_false_negative  for every train item of a row (the funnel: inside the shard) BOTH its bits are set: what the candidate stage relies on, stated
                           without the restated words

Out of scope: overflow or underflow of a row's SUM of squares in fp32 (include/pda_hip.h states the precondition, prep_ref repeats it).
"""
import collections
import functools
import zlib

import numpy as np

import prep_ref as pr

F = pr.F
DIMS = pr.DIMS
TABLE_ROWS = 2000
BLOCKS = {64: (1, 17, 255, 257, 1025), 128: (1, 17, 255, 257, 1025), 256: (1, 17, 127, 129, 513)}


def floor(d):
    """smallest stored norm / exact norm of a correct fp32 prep (module docstring: unorm.pad)"""
    g = d * pr.U24 / (1.0 - d * pr.U24)
    return pr.PAD * np.sqrt(1.0 - g) * (1.0 - pr.U24) ** 4


# ---- layout ----------------------------------------------------------------------------------------------------------------------------------------
def upw(d):
    return 128 if d == 256 else 256


def n_pad(n, d):
    ut = 4 * upw(d)
    return (n + ut - 1) // ut * ut


def image_bytes(n, d):
    return n_pad(n, d) * 2 * d


def frag_index(rb, c, d, defect=None):
    """16-byte fragment index of (block row rb, 8-element chunk c of the row)"""
    NK, NU = d // 32, upw(d) // 16
    wgw, u, j, k, g = rb // upw(d), (rb >> 4) & (NU - 1), rb & 15, c >> 2, c & 3
    if defect == "kstep_reversed":
        k = NK - 1 - k
    lane = g + 4 * j if defect == "lane_swapped" else j + 16 * g
    return ((wgw * NU + u) * NK + k) * 64 + lane


def _index_grid(npad, d, defect=None):
    return frag_index(np.arange(npad)[:, None], np.arange(d // 8)[None, :], d, defect)


def decode_image(raw, n, d):
    """image bytes (uint8 [n_pad 2 d]) -> uint16 [n_pad, d]: row rb, element e of the block"""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    npad = n_pad(n, d)
    assert raw.size == npad * 2 * d, (raw.size, npad, d)
    return raw.view(np.uint16).reshape(npad * d // 8, 8)[_index_grid(npad, d)].reshape(npad, d)


def encode_image(rows16, d, defect=None):
    """uint16 [n_pad, d] -> image bytes"""
    npad = rows16.shape[0]
    out = np.zeros((npad * d // 8, 8), np.uint16)
    out[_index_grid(npad, d, defect)] = rows16.reshape(npad, d // 8, 8)
    return out.view(np.uint8).ravel()


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "d bf16 f16 n")        # bf16: the table's type; f16: the funnel's image (with uerr)


def case_id(c):
    return "d%d-%s-%s-n%d" % (c.d, "bf16" if c.bf16 else "f32", "f16img" if c.f16 else "bf16img", c.n)


def gpu_cases():
    return [Case(d, bf, f16, n) for d in DIMS for bf in (False, True) for f16 in (False, True) for n in BLOCKS[d]]


# the special rows of every table (row id -> kind); everything else is N(0, 0.3)
SPECIAL = {5: "zero", 6: "signed_zero", 11: "tiny", 12: "large", 100: "clamp", 101: "exact", 102: "bf16_half", 103: "bf16_half_even", 104: "f16_half",
           105: "f16_small", TABLE_ROWS - 1: "minus_zero"}


@functools.lru_cache(maxsize=None)
def make_table(d, bf16):
    """-> (U32 float32 [2 000, d] the table's values, Ubits uint16 or None).  One table per (d, type), every row kind in it:
      zero / signed_zero   0.0 everywhere / +-0.0 alternating: the norm is exactly 0, the image keeps the signs
      tiny, large          N(0, 0.3) x 1e-18 (squares partly subnormal; every element flushes to 0 in fp16: the residual is the row) and x 1e4
      clamp                one entry of 7e4 among N(0, 0.3): the fp16 image holds 65504, that element's residual is 4 496
      exact                multiples of 1/8 up to 15/8: representable in bf16 and fp16, residual 0
      bf16_half            (1 + (2 j + 1) 2^-8) 2^e, j = 0, 1, 2, ..: exact half-way points between bf16 neighbours, the lower one's last bit even and odd
                           in turn -- RNE goes down, up, down, ..; truncation always down; half-up always up
      bf16_half_even       the same with even lower neighbours only: RNE rounds EVERY element down by 2^-8 relative, 3.6 x the pad -- where a norm
                           summed from the rounded row is too small
      f16_half             (1 + (2 j + 1) 2^-11) 2^e: the same for fp16 (e inside half's normal range)
      f16_small            +-1e-6 (half's subnormal range) and +-1e-9 (flushes to +-0: the whole value is the residual) in turn
      minus_zero           the LAST row: N(0, 0.3) with -0.0 at elements 0 and d - 1"""
    rng = np.random.default_rng(zlib.crc32(b"user table %d" % d))
    U = (rng.standard_normal((TABLE_ROWS, d)) * 0.3).astype(F)
    e = np.arange(d)
    sign = np.where(e % 3 == 0, -1.0, 1.0)
    scale = 2.0 ** ((e // 8) % 9 - 4)
    for r, kind in SPECIAL.items():
        if kind == "zero":
            U[r] = 0.0
        elif kind == "signed_zero":
            U[r] = np.where(e % 2 == 0, F(0.0), F(-0.0))
        elif kind == "tiny":
            U[r] *= F(1e-18)
        elif kind == "large":
            U[r] *= F(1e4)
        elif kind == "clamp":
            U[r, d // 2 + 3] = F(7e4)
        elif kind == "exact":
            U[r] = (sign * ((e % 15) + 1) / 8.0).astype(F)
        elif kind == "bf16_half":
            U[r] = (sign * (1.0 + (2 * (e % 64) + 1) * 2.0 ** -8) * scale).astype(F)
        elif kind == "bf16_half_even":
            U[r] = (sign * (1.0 + (4 * (e % 32) + 1) * 2.0 ** -8) * scale).astype(F)
        elif kind == "f16_half":
            U[r] = (sign * (1.0 + (2 * (e % 512) + 1) * 2.0 ** -11) * scale).astype(F)
        elif kind == "f16_small":
            U[r] = (sign * np.where(e % 2 == 0, 1e-6, 1e-9)).astype(F)
        elif kind == "minus_zero":
            U[r, 0] = U[r, d - 1] = F(-0.0)
    bits = None
    if bf16:
        bits = pr.bf16_rne(U)
        U = pr.bf16_to_f32(bits)
    U.setflags(write=False)
    return U, bits


def make_users(c):
    """block rows -> user ids: shuffled, with repeats, the last row of the table and (from 17 rows on) every special row among them"""
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
    if c.n == 1:
        return np.array([TABLE_ROWS - 1], np.int32)
    must = np.array(sorted(SPECIAL), np.int32)
    assert c.n > len(must) + 2
    fill = rng.integers(0, TABLE_ROWS, c.n - len(must)).astype(np.int32)
    fill[0], fill[1] = must[3], fill[-1]                          # a special row and an ordinary one twice
    return rng.permutation(np.concatenate([must, fill])).astype(np.int32)


# ---- fp32 emulation of uprep5_kernel ---------------------------------------------------------------------------------------------------------------
IMAGE_MUTANTS = {
    "image_rtz": "image.bits", "image_half_up": "image.bits", "fp16_clamp_omitted": "image.bits", "norm_from_rounded": "unorm.sound",
    "pad_1.0009765625_dropped": "unorm.pad", "pad_1.0001_dropped": "unorm.pad", "residual_of_neighbour": "uerr.tight", "lane_swapped": "image.bits",
    "kstep_reversed": "image.bits", "padding_norm_nonzero": "unorm.padding",
}
BLOOM_MUTANTS = {
    "one_hash": "bloom.no_false_negative", "tail_dropped": "bloom.no_false_negative", "block_row_for_user_id": "bloom.no_false_negative",
    "out_of_shard_hashed": "bloom.bits",
}
NORM_PAIRS = ((0, 4), (1, 5), (2, 6), (3, 7))       # ss += x[k] x[k] + y[k] y[k], x = elements 0 .. 3 and y = 4 .. 7 of the thread's eight
HALF_PAIRS = ((0, 1), (2, 3), (4, 5), (6, 7))       # pack_half8: rs += r0 r0 + r1 r1 over neighbouring elements


def sumsq32(X, d, pairs):
    """a row's fp32 sum of squares as uprep5_kernel forms it: eight squares per thread in its order, then the xor ladder over the row's d / 8 threads"""
    m, T = X.shape[0], d // 8
    Y = np.ascontiguousarray(X, dtype=F).reshape(m, T, 8)
    ss = np.zeros((m, T), F)
    with np.errstate(under="ignore"):
        for a, b in pairs:
            ss = ss + (Y[:, :, a] * Y[:, :, a] + Y[:, :, b] * Y[:, :, b])
        lanes, o = np.arange(T), T // 2
        while o > 0:
            ss = ss + ss[:, lanes ^ o]
            o //= 2
    return ss[:, 0]


def padded32(ss, defect=None):
    v = np.sqrt(ss.astype(F))
    if defect != "pad_1.0009765625_dropped":
        v = v * F(1.0009765625)
    if defect != "pad_1.0001_dropped":
        v = v * F(1.0001)
    return v.astype(F)


def bf16_half_up(x):
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32).astype(np.uint64)
    return ((u + 0x8000) >> 16).astype(np.uint16)


def emulate_user_image(U32, Ubits, users, d, f16, defect=None):
    """uprep5_kernel<d, bf16 table, .., F16 = f16> in numpy fp32 -> dict(raw: image bytes, unorm, uerr or None)"""
    n = len(users)
    npad = n_pad(n, d)
    X = np.zeros((npad, d), F)
    X[:n] = U32[users]
    if f16:
        img = pr.f16_rne_clamped(X, clamp=defect != "fp16_clamp_omitted")
        back = img.view(np.float16).astype(F)
    else:
        if Ubits is not None:
            img = np.zeros((npad, d), np.uint16)
            img[:n] = Ubits[users]
        else:
            img = {"image_rtz": pr.bf16_rtz, "image_half_up": bf16_half_up}.get(defect, pr.bf16_rne)(X)
        back = pr.bf16_to_f32(img)
    ss = sumsq32(back if defect == "norm_from_rounded" and np.isfinite(back).all() else X, d, NORM_PAIRS)
    unorm = padded32(ss, defect)
    if defect == "padding_norm_nonzero":
        unorm[n:] = F(1.0)
    f = {"raw": encode_image(img, d, defect), "unorm": unorm, "uerr": None}
    if f16:
        with np.errstate(invalid="ignore"):
            res = (X - (back.reshape(npad, d // 2, 2)[:, :, ::-1].reshape(npad, d) if defect == "residual_of_neighbour" else back)).astype(F)
        res = np.where(np.isfinite(res), res, F(0))
        f["uerr"] = padded32(sumsq32(res, d, HALF_PAIRS), defect)
    return f


# ---- conditions on the image and the norms ---------------------------------------------------------------------------------------------------------
def expected_image(U32, Ubits, users, d, f16):
    """the bits the image must hold in rows 0 .. n - 1, from the table alone"""
    X = U32[users]
    if f16:
        return pr.f16_rne_clamped(X)
    return Ubits[users] if Ubits is not None else pr.bf16_rne(X)


def _check_padded(R, what, v, true2, n, d):
    """v float32 [n_pad] stored, true2 float64 [n] exact squared norms"""
    v64 = v.astype(np.float64)
    true = np.sqrt(true2)
    R.need(what + ".sound", (v64[:n] >= 0) & (v64[:n] ** 2 + pr.quantum(d) >= true2))
    R.need(what + ".tight", v64[:n] <= pr.cap(d) * np.sqrt(true2 + pr.quantum(d)))
    R.need(what + ".pad", v64[:n] >= floor(d) * np.sqrt(np.maximum(true2 - pr.quantum(d), 0.0)))
    R.need(what + ".zero", (v[:n] == 0) | (true2 > 0))
    R.need(what + ".padding", v[n:] == 0)
    R.worst(what + "/exact", v64[:n], np.where(true > 1e-15, true, 0))          # (below: the quantum, not the pad, decides the ratio)


def check_user_image(raw, unorm, uerr, U32, Ubits, users, d, f16):
    """every condition on a block's image bytes, padded norms and (f16) padded residual norms -> prep_ref.Report"""
    R = pr.Report()
    n = len(users)
    npad = n_pad(n, d)
    img = decode_image(raw, n, d)
    want = expected_image(U32, Ubits, users, d, f16)
    R.need("image.bits", img[:n] == want)
    R.need("image.padding", img[n:] == 0)
    X64 = U32[users].astype(np.float64)
    unorm = np.ascontiguousarray(unorm, dtype=F)
    assert unorm.shape == (npad,), (unorm.shape, npad)
    assert pr.norm_upper(1.0, d) == pr.cap(d) * np.sqrt(1.0 + pr.quantum(d))            # (unorm.tight below is prep_ref.norm_upper, spelled out)
    _check_padded(R, "unorm", unorm, (X64 * X64).sum(1), n, d)
    assert (uerr is not None) == bool(f16)
    if f16:
        uerr = np.ascontiguousarray(uerr, dtype=F)
        assert uerr.shape == (npad,), (uerr.shape, npad)
        res = X64 - pr.f16_to_f64(want)
        _check_padded(R, "uerr", uerr, (res * res).sum(1), n, d)
    return R


# ---- the Bloom filters -----------------------------------------------------------------------------------------------------------------------------
M32 = np.uint64(0xFFFFFFFF)


def bloom_h1(x):
    return (((np.asarray(x).astype(np.int64).astype(np.uint64) & M32) * np.uint64(0x9E3779B1)) & M32) >> np.uint64(22)


def bloom_h2(x):
    return ((((np.asarray(x).astype(np.int64).astype(np.uint64) & M32) * np.uint64(0x85EBCA6B) + np.uint64(0x27D4EB2F)) & M32)) >> np.uint64(22)


def _set_bits(words, r, h):
    np.bitwise_or.at(words[r], (h >> np.uint64(5)).astype(np.intp), (np.uint64(1) << (h & np.uint64(31))).astype(np.uint32))


def bloom_keys(ids, shard=None, defect=None):
    """what a row's train-item ids are hashed as.  shard None: generation 4, the id as stored; shard (pos_of, item_offset): the funnel, the visiting
    position of the ids inside [item_offset, item_offset + len(pos_of))"""
    ids = np.asarray(ids, dtype=np.int64)
    if shard is None:
        return ids
    pos_of, off = shard
    loc = ids - off
    inside = (loc >= 0) & (loc < len(pos_of))
    if defect == "out_of_shard_hashed":
        return np.asarray(pos_of, dtype=np.int64)[np.clip(loc, 0, len(pos_of) - 1)]
    return np.asarray(pos_of, dtype=np.int64)[loc[inside]]


def _hist_row(users, r, by_user, defect=None):
    return int(users[r]) if by_user and defect != "block_row_for_user_id" else r


def bloom_words(users, indptr, indices, by_user, shard=None):
    """the restated filters: uint32 [len(users), 32]"""
    words = np.zeros((len(users), 32), np.uint32)
    for r in range(len(users)):
        hr = _hist_row(users, r, by_user)
        keys = bloom_keys(indices[indptr[hr]: indptr[hr + 1]], shard)
        _set_bits(words, r, bloom_h1(keys))
        _set_bits(words, r, bloom_h2(keys))
    return words


def emulate_bloom(users, indptr, indices, by_user, shard=None, defect=None):
    """hist_bloom4_kernel / hist_bloom7_kernel as they walk a row: eight lanes, lane `sub` takes entries b + sub + 32 t + 8 q, q = 0 .. 3 in flight,
    each guarded by the row's end"""
    words = np.zeros((len(users), 32), np.uint32)
    for r in range(len(users)):
        hr = _hist_row(users, r, by_user, defect)
        b, e = int(indptr[hr]), int(indptr[hr + 1])
        if defect == "tail_dropped":
            e = b + (e - b) // 32 * 32
        taken = [i0 + 8 * q for sub in range(8) for i0 in range(b + sub, e, 32) for q in range(4) if i0 + 8 * q < e]
        keys = bloom_keys(indices[np.array(taken, dtype=np.int64)], shard, defect)
        _set_bits(words, r, bloom_h1(keys))
        if defect != "one_hash":
            _set_bits(words, r, bloom_h2(keys))
    return words


def check_bloom(words, users, indptr, indices, by_user, shard=None):
    """-> prep_ref.Report on device (or emulated) words uint32 [len(users), 32]"""
    R = pr.Report()
    words = np.ascontiguousarray(words).view(np.uint32).reshape(len(users), 32)
    R.need("bloom.bits", words == bloom_words(users, indptr, indices, by_user, shard))
    ok = np.ones(len(users), bool)
    for r in range(len(users)):
        hr = int(users[r]) if by_user else r
        keys = bloom_keys(indices[indptr[hr]: indptr[hr + 1]], shard)
        for h in (bloom_h1(keys), bloom_h2(keys)):
            ok[r] &= bool(((words[r][(h >> np.uint64(5)).astype(np.intp)] >> (h & np.uint64(31)).astype(np.uint32)) & 1).all())
    R.need("bloom.no_false_negative", ok)
    return R


HIST_LENS = (150, 0, 1, 3, 4, 5, 8, 9, 31, 32, 33, 64, 1025, 40)       # the last: a row of repeated ids
HIST_ROWS = 80
BLOOM_BLOCKS = (1, 31, 32, 33, 70)
SHARD_ITEMS, SHARD_OFFSET = 300, 100
BloomCase = collections.namedtuple("BloomCase", "funnel by_user n")


def bloom_case_id(c):
    return "%s-%s-n%d" % ("funnel" if c.funnel else "gen4", "by_user" if c.by_user else "by_row", c.n)


def bloom_cases():
    return [BloomCase(fn, bu, n) for fn in (False, True) for bu in (True, False) for n in BLOOM_BLOCKS]


@functools.lru_cache(maxsize=None)
def make_history(funnel):
    """-> (indptr int64 [81], indices int32): one CSR of 80 rows, rows 0 .. 13 of HIST_LENS entries (every remainder of the 8-lanes x 4-loads loop:
    0, 1, 3, 4, 5, 8, 9, 31, 32, 33, 64, 150 = 4 x 32 + 22, 1 025 = 32 x 32 + 1), the same lengths shuffled over the rows behind, ids ascending inside
    a row.  Generation 4: ids from all of [0, 2^31), 2^31 - 1 and 0 among them.  The funnel: ids from [0, 600) around the shard [100, 400) -- train items
    on both sides of it, both of its edges -- and one id of 2^31 - 1."""
    rng = np.random.default_rng(20261 + int(funnel))
    lens = list(HIST_LENS) + [HIST_LENS[i] for i in rng.integers(0, len(HIST_LENS), HIST_ROWS - len(HIST_LENS))]
    rows = []
    for i, L in enumerate(lens):
        r = rng.integers(0, 600 if funnel else 2 ** 31, L).astype(np.int64)
        if L == 40:
            r[8:] = r[rng.integers(0, 8, 32)]                       # repeated ids
        if L >= 31:
            r[:6] = [0, SHARD_OFFSET - 1, SHARD_OFFSET, SHARD_OFFSET + SHARD_ITEMS - 1, SHARD_OFFSET + SHARD_ITEMS, 2 ** 31 - 1]
        rows.append(np.sort(r))
    indptr = np.zeros(HIST_ROWS + 1, np.int64)
    indptr[1:] = np.cumsum(lens)
    indices = np.concatenate(rows).astype(np.int32)
    indptr.setflags(write=False)
    indices.setflags(write=False)
    return indptr, indices


def make_bloom_users(c):
    """not arange: a shuffle of the history's rows with one repeat, rows 0 .. 13 (every length) among them from 31 rows on"""
    rng = np.random.default_rng(zlib.crc32(bloom_case_id(c).encode()))
    if c.n == 1:
        return np.array([12], np.int32)                             # (the 1 025-entry row by user id, the 150-entry row by block row)
    u = np.concatenate([np.arange(len(HIST_LENS)), len(HIST_LENS) + rng.permutation(HIST_ROWS - len(HIST_LENS))[: c.n - len(HIST_LENS) - 1]])
    u = rng.permutation(np.concatenate([u, u[-1:]])).astype(np.int32)
    if (u == np.arange(c.n)).all():
        u = u[::-1].copy()
    return u


def shard_order():
    """a fixed random visiting order of the funnel's 300-item shard -> (order int32, pos_of int32)"""
    order = np.random.default_rng(20263).permutation(SHARD_ITEMS).astype(np.int32)
    pos_of = np.zeros(SHARD_ITEMS, np.int32)
    pos_of[order] = np.arange(SHARD_ITEMS, dtype=np.int32)
    return order, pos_of
