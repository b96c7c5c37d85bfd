"""CPU: the user side's checker (tests/user_prep_ref.py) before it meets the device.

  layout          the restated n_pad and image bytes equal offs[3] of pda_score_topk4_phase_image_offsets (the library loads without a GPU; what
                  ops.huge_user_image / ops.funnel_user_image allocate is compared on the device, in test_gpu_user_prep.py: they need HBM tensors);
                  the restated fragment index is a permutation of the image's fragments, and the decoder inverts the encoder
  emulation       an fp32 emulation of uprep5_kernel and of the two Bloom kernels' walks satisfies every condition on every case test_gpu_user_prep.py
                  uses: the conditions are attainable by a correct fp32 kernel, and no case is left out or loosened for the reference's sake
  mutants         fourteen single-defect variants of the emulations each fail the condition they NAME on at least one case
  the table       holds every row kind it promises, and the kinds do what they are there for (the residual of the 7e4 entry is 4 496, ...)
"""
import ctypes as C

import numpy as np
import pytest

import prep_ref as pr
import user_prep_ref as ur

F = np.float32


def inputs(c):
    U32, Ubits = ur.make_table(c.d, c.bf16)
    return U32, Ubits, ur.make_users(c)


def bloom_inputs(c):
    indptr, indices = ur.make_history(c.funnel)
    shard = (ur.shard_order()[1], ur.SHARD_OFFSET) if c.funnel else None
    return ur.make_bloom_users(c), indptr, indices, shard


def test_n_pad_equals_the_library():
    from pda_amd import _lib
    lib = _lib.load()
    for d in ur.DIMS:
        for n in sorted(set(ur.BLOCKS[d]) | {2, 16, 511, 512, 1023, 1024, 2049, 17003, 262144}):
            offs = (C.c_size_t * 4)()
            assert lib.pda_score_topk4_phase_image_offsets(n, 20000, d, 1, C.cast(offs, C.c_void_p)) == 0
            assert int(offs[3]) == ur.n_pad(n, d), (n, d)
            assert ur.image_bytes(n, d) == int(offs[3]) * 2 * d


@pytest.mark.parametrize("d", ur.DIMS)
def test_the_fragment_index_is_a_permutation_and_the_decoder_inverts_the_encoder(d):
    for n in ur.BLOCKS[d]:
        npad = ur.n_pad(n, d)
        idx = ur.frag_index(np.arange(npad)[:, None], np.arange(d // 8)[None, :], d)
        assert np.array_equal(np.sort(idx.ravel()), np.arange(npad * d // 8))
        rows = np.random.default_rng(n).integers(0, 65536, (npad, d)).astype(np.uint16)
        assert np.array_equal(ur.decode_image(ur.encode_image(rows, d), n, d), rows)
    # the sentence of the layout, by hand: d = 256 (UPW 128, NU 8, NK 8), row 300 = wave 2, user block 2, user 12; chunk 13 = k-step 3, quarter 1
    if d == 256:
        assert ur.frag_index(300, 13, d) == ((2 * 8 + 2) * 8 + 3) * 64 + (12 + 16 * 1)
    else:       # UPW 256, NU 16: row 300 = wave 1, user block 2, user 12; chunk 6 = k-step 1, quarter 2
        assert ur.frag_index(300, 6, d) == ((1 * 16 + 2) * (d // 32) + 1) * 64 + (12 + 16 * 2)


def test_the_case_lists_cover_what_they_promise():
    cs = ur.gpu_cases()
    assert len(cs) == len(set(cs)) == 60
    for d in ur.DIMS:
        for bf in (False, True):
            for f16 in (False, True):
                assert {c.n for c in cs if (c.d, c.bf16, c.f16) == (d, bf, f16)} == set(ur.BLOCKS[d])
    for c in cs:
        users = ur.make_users(c)
        assert len(users) == c.n and (ur.TABLE_ROWS - 1) in users and users.max() < ur.TABLE_ROWS
        if c.n > 1:
            assert set(ur.SPECIAL) <= set(users.tolist()) and len(np.unique(users)) < c.n and not np.array_equal(users, np.sort(users))
    bs = ur.bloom_cases()
    assert {(c.funnel, c.by_user) for c in bs} == {(a, b) for a in (False, True) for b in (False, True)} and {c.n for c in bs} == set(ur.BLOOM_BLOCKS)
    for funnel in (False, True):
        indptr, indices = ur.make_history(funnel)
        lens = np.diff(indptr)
        assert {0, 1, 3, 4, 5, 8, 9, 31, 32, 33, 64, 150, 1025} <= set(lens[:14].tolist()) and len(lens) == ur.HIST_ROWS
        assert {int(x) % 32 for x in lens} >= {0, 1, 3, 4, 5, 8, 9, 31, 22} and all((np.diff(indices[b:e]) >= 0).all() for b, e in zip(indptr[:-1], indptr[1:]))
        rep = indices[indptr[13]: indptr[14]]
        assert len(rep) == 40 and len(np.unique(rep)) < 20
        assert indices.max() == 2 ** 31 - 1
        if funnel:
            inside = (indices >= ur.SHARD_OFFSET) & (indices < ur.SHARD_OFFSET + ur.SHARD_ITEMS)
            assert inside.any() and (indices < ur.SHARD_OFFSET).any() and (indices[~inside] > ur.SHARD_OFFSET).any()
        else:
            assert (indices > 2 ** 30).any()
    for c in bs:
        users = ur.make_bloom_users(c)
        assert len(users) == c.n and users.max() < ur.HIST_ROWS and not np.array_equal(users, np.arange(c.n))
        if c.n >= 31:
            assert set(range(14)) <= set(users.tolist()) and len(np.unique(users)) < c.n


@pytest.mark.parametrize("d", ur.DIMS)
def test_the_row_kinds_do_what_they_are_there_for(d):
    U, _ = ur.make_table(d, False)
    row = {kind: U[r] for r, kind in ur.SPECIAL.items()}
    assert not row["zero"].any() and not row["signed_zero"].any() and np.signbit(row["signed_zero"]).any() and not np.signbit(row["signed_zero"]).all()
    assert np.signbit(row["minus_zero"][[0, d - 1]]).all() and (row["minus_zero"][[0, d - 1]] == 0).all()
    sq = row["tiny"].astype(np.float64) ** 2
    assert (sq < 2.0 ** -126).any() and sq.sum() > 2.0 ** -120                              # subnormal squares, a normal sum
    assert np.abs(row["large"]).max() < 65504 and (row["large"].astype(np.float64) ** 2).sum() < 1e30
    clamp = row["clamp"].astype(np.float64) - pr.f16_to_f64(pr.f16_rne_clamped(row["clamp"]))
    assert np.abs(clamp).max() == 4496.0
    assert np.array_equal(pr.bf16_to_f32(pr.bf16_rne(row["exact"])), row["exact"]) and np.array_equal(pr.f16_to_f64(pr.f16_rne_clamped(row["exact"])), row["exact"])
    for kind in ("bf16_half", "bf16_half_even"):
        x = row[kind]
        lo, hi = pr.bf16_rtz(x), ur.bf16_half_up(x)
        assert (hi == lo + 1).all() and (x.view(np.uint32) & 0xFFFF == 0x8000).all()         # exact half-way points
        rne = pr.bf16_rne(x)
        assert ((rne & 1) == 0).all()
        if kind == "bf16_half":
            assert (rne == lo).any() and (rne == hi).any()                                    # even and odd lower neighbours
        else:
            assert (rne == lo).all()
    x = row["f16_half"].astype(np.float64)
    h = pr.f16_rne_clamped(row["f16_half"])
    res = x - pr.f16_to_f64(h)
    assert ((h & 1) == 0).all() and (res * x > 0).any() and (res * x < 0).any()              # ties to even, towards and away from zero
    assert np.array_equal(np.abs(res), 2.0 ** (np.floor(np.log2(np.abs(x))) - 11))           # exactly half a unit of the last place
    small = pr.f16_rne_clamped(row["f16_small"])
    assert set((small[0::2] & 0x7FFF).tolist()) == {17} and set((small[1::2] & 0x7FFF).tolist()) == {0}      # 1e-6 = 17 x 2^-24 rounded; 1e-9 -> +-0
    assert (small[1::2] == 0x8000).any() and (small[1::2] == 0).any()


@pytest.mark.parametrize("c", ur.gpu_cases(), ids=ur.case_id)
def test_the_emulation_meets_every_condition(c):
    U32, Ubits, users = inputs(c)
    f = ur.emulate_user_image(U32, Ubits, users, c.d, c.f16)
    assert f["raw"].size == ur.image_bytes(c.n, c.d)
    R = ur.check_user_image(f["raw"], f["unorm"], f["uerr"], U32, Ubits, users, c.d, c.f16)
    print("%s: %s" % (ur.case_id(c), R.line()))
    assert not R.failed, R.failed


@pytest.mark.parametrize("c", ur.bloom_cases(), ids=ur.bloom_case_id)
def test_the_bloom_emulation_meets_every_condition(c):
    users, indptr, indices, shard = bloom_inputs(c)
    R = ur.check_bloom(ur.emulate_bloom(users, indptr, indices, c.by_user, shard), users, indptr, indices, c.by_user, shard)
    assert not R.failed, R.failed


@pytest.mark.parametrize("mutant", sorted(ur.IMAGE_MUTANTS))
def test_every_image_mutant_fails_its_named_condition(mutant):
    hits = []
    for c in ur.gpu_cases():
        U32, Ubits, users = inputs(c)
        f = ur.emulate_user_image(U32, Ubits, users, c.d, c.f16, defect=mutant)
        R = ur.check_user_image(f["raw"], f["unorm"], f["uerr"], U32, Ubits, users, c.d, c.f16)
        if ur.IMAGE_MUTANTS[mutant] in R.failed:
            hits.append(ur.case_id(c))
    print("%s fails %s on %d cases" % (mutant, ur.IMAGE_MUTANTS[mutant], len(hits)))
    assert hits, "%s passed the condition it should trip" % mutant


@pytest.mark.parametrize("mutant", sorted(ur.BLOOM_MUTANTS))
def test_every_bloom_mutant_fails_its_named_condition(mutant):
    hits = []
    for c in ur.bloom_cases():
        users, indptr, indices, shard = bloom_inputs(c)
        R = ur.check_bloom(ur.emulate_bloom(users, indptr, indices, c.by_user, shard, defect=mutant), users, indptr, indices, c.by_user, shard)
        if ur.BLOOM_MUTANTS[mutant] in R.failed:
            hits.append(ur.bloom_case_id(c))
    print("%s fails %s on %d cases" % (mutant, ur.BLOOM_MUTANTS[mutant], len(hits)))
    assert hits, "%s passed the condition it should trip" % mutant


def test_the_mutants_the_issue_lists_are_all_there():
    assert len(ur.IMAGE_MUTANTS) == 10 and len(ur.BLOOM_MUTANTS) == 4
    assert set(ur.IMAGE_MUTANTS.values()) <= {"image.bits", "image.padding", "unorm.sound", "unorm.tight", "unorm.pad", "unorm.zero", "unorm.padding",
                                             "uerr.sound", "uerr.tight", "uerr.pad", "uerr.zero", "uerr.padding"}
    assert set(ur.BLOOM_MUTANTS.values()) <= {"bloom.bits", "bloom.no_false_negative"}


def test_the_hashes_are_uint32_arithmetic():
    """against Python integers: ids up to 2^31 - 1 wrap in 32 bits, not 64"""
    for x in (0, 1, 299, 65535, 2 ** 30 + 12345, 2 ** 31 - 1):
        assert int(ur.bloom_h1(np.array([x]))[0]) == ((x * 0x9E3779B1) & 0xFFFFFFFF) >> 22
        assert int(ur.bloom_h2(np.array([x]))[0]) == ((x * 0x85EBCA6B + 0x27D4EB2F) & 0xFFFFFFFF) >> 22
