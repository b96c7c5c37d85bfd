"""CPU: the item prep's checker (tests/prep_ref.py) before it meets the device.

  layout totals   the restated offset tables end where the library's *_bytes entry points say (the library loads without a GPU)
  emulation       an fp32 emulation of both preps satisfies every condition on every case test_gpu_item_prep.py uses: the conditions are attainable
                  by a correct fp32 prep, and no case is left out or loosened for the reference's sake
  mutants         sixteen single-defect variants of the emulation each fail a NAMED condition on at least one case
  host proof      decided_tail_cases.suffix_bounds -- the bounds test_decided_tail_criterion.py proves the criterion on -- is bit-equal to the
                  emulation on sufA and never above it on sufB: a larger bound decides later, never earlier, so the proof carries over
"""
import numpy as np
import pytest

import decided_tail_cases as dt
import prep_ref as pr

F = np.float32
ENTRIES = ("pda_item_prep4_bytes", "pda_item_prep_bytes", "pda_item_prep_ordered_bytes", "pda_item_prep_bf16_bytes", "pda_item_prep_ordered_bf16_bytes")
# the condition(s) a mutant has to trip, by name: anything else failing alone does not count
EXPECTED = {
    "pad_dropped": {"norm.sound"},
    "pad_twice": {"norm.tight"},
    "norm_half_row": {"norm.sound"},
    "suffix_exclusive": {"sufA", "sufB.sound", "sufR"},
    "tile_max_32_of_64": {"sufA", "sufB.sound", "sufR"},
    "ipop_nearest": {"ipop.le"},
    "ipop_uncapped": {"ipop.cap"},
    "image_rtz": {"image.bits"},
    "image_unscaled": {"image.bits"},
    "residual_unscaled": {"rnorm.sound", "rnorm.tight"},
    "padding_pop_zero": {"tail.padding"},
    "nan_ranked": {"sufA"},
    "pos_of_off_by_one": {"pos_of"},
    "swizzle_omitted": {"image.bits"},
    "fp16_clamp_omitted": {"image.bits"},
    "meta5_other_half": {"meta5.pmax", "meta5.nmax.sound", "meta5.rmax"},
}


def resolved_order(c, inp):
    return pr.host_visiting_order(inp["I32"], inp["pop"]) if isinstance(inp["order"], str) else inp["order"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_layout_totals_equal_the_library(entry):
    from pda_amd import _lib
    fn = getattr(_lib.load(), entry)
    for d in pr.DIMS:
        for n in pr.LAYOUT_N + (2, 31, 32, 33, 127, 128, 129, 1000, 1 << 20):
            assert fn(n, d) == pr.layout_total(entry, n, d), (entry, n, d)


def test_the_case_list_covers_what_it_promises():
    cs = pr.gpu_cases()
    assert 90 <= len(cs) <= 130
    for kind in ("prep4", "prep7", "gen3o"):
        for d in pr.DIMS:
            for bf in (False, True):
                for n in (65, 4097):
                    assert any(c.kind == kind and c.d == d and c.bf16 == bf and c.n == n and c.orderk == "random" for c in cs)
    for d in pr.DIMS:
        assert {1, 63, 64, 65, 4097} <= {c.n for c in cs if c.d == d}
    for d in (64, 256):
        assert set(pr.POPS) <= {c.popk for c in cs if c.d == d and c.kind == "prep4"}
        assert set(pr.ORDERS) <= {c.orderk for c in cs if c.d == d and c.kind == "prep4"}
    assert {c.plant for c in cs if c.n == 65600 and c.d == 64} == {"last", "t1024", "t1023"}
    assert all(c.d == 64 for c in cs if c.n == 65600)


@pytest.mark.parametrize("c", pr.gpu_cases(), ids=pr.case_id)
def test_the_emulation_meets_every_condition(c):
    inp = pr.make_inputs(c)
    order = resolved_order(c, inp)
    R = pr.check(c, pr.emulate(c, inp, order), inp, order)
    print("%s: %s" % (pr.case_id(c), R.line()))
    assert not R.failed, R.failed


def test_the_emulation_survives_its_own_decoder():
    """emulated fields -> bytes at the layout's offsets -> decode: the same fields (the decoders read where the layout says)"""
    c = pr.Case("prep4", 128, False, 65, "pow", "random", None)
    inp = pr.make_inputs(c)
    f = pr.emulate(c, inp, inp["order"])
    L = pr.prep4_layout(c.n, c.d)
    blob = np.zeros(L["total"], np.uint8)

    def put(off, x):
        b = np.ascontiguousarray(x).view(np.uint8).ravel()
        blob[off: off + b.size] = b
    for k in ("hdr", "pos_of", "sufA", "sufB", "sufR", "meta5", "pinfo"):
        put(L[k], f[k])
    put(L["rows5"], f["rows5_raw"])
    put(L["rows"], np.concatenate([f["row"].view(np.uint8), f["lo"].view(np.uint8), f["hi"].view(np.uint8), f["tail"].view(np.uint8)], 1))
    g = pr.decode_prep4(blob, c.n, c.d)
    assert sorted(g) == sorted(f)
    for k in f:
        assert np.array_equal(pr.named_bytes(f)[k], pr.named_bytes(g)[k]), k


@pytest.mark.parametrize("mutant", pr.MUTANTS)
def test_every_mutant_fails_a_named_condition(mutant):
    hits = {}
    for c in pr.mutant_cases():
        inp = pr.make_inputs(c)
        order = resolved_order(c, inp)
        R = pr.check(c, pr.emulate(c, inp, order, defect=mutant), inp, order)
        for name in set(R.failed) & EXPECTED[mutant]:
            hits.setdefault(name, []).append(pr.case_id(c))
    print("%s fails %s" % (mutant, {k: len(v) for k, v in hits.items()}))
    assert hits, "%s passed every condition it should trip" % mutant


def test_there_are_at_least_twelve_mutants():
    assert len(pr.MUTANTS) >= 12 and set(pr.MUTANTS) == set(EXPECTED)


@pytest.mark.parametrize("popk", ["pow", "zeros", "tiny", "nan", "ones"])
@pytest.mark.parametrize("n", [65, 4097])
def test_the_host_proof_bounds_are_below_the_kernels(n, popk):
    """suffix_bounds pads the norm by 1.0000005, the kernel by 1.0009765625 * 1.0001: the helper's sufB is the tighter one everywhere."""
    for d in pr.DIMS:
        inp = pr.make_inputs(pr.Case("prep4", d, False, n, popk, None, None))
        order, sufA, sufB = dt.suffix_bounds(inp["I32"], inp["pop"])
        f = pr.emulate_prep4(inp["I32"], inp["pop"], order.astype(np.int32), d)
        assert np.array_equal(sufA.view(np.uint32), f["sufA"].view(np.uint32))
        assert (sufB <= f["sufB"]).all()
        assert (sufB[f["sufB"] > 0] > 0).all()
        R = pr.check_prep4(f, inp["I32"], inp["pop"], order.astype(np.int32), d)
        assert not R.failed, R.failed
