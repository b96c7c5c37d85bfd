"""What the seven sampler entry points of the library refuse before they launch anything, without a GPU: the checks they share (pda_sample.h:
sample_call_ok) violated one at a time, and the limits that are each entry point's own.  Every call here carries a violation, so none reaches a
launch; that a batch above the SSM sampler's cap is FINE for the triplet sampler needs a launch: tests/test_gpu_sampler_parity.py."""
import ctypes as C

import pytest

ERR_ARG = -1
NULL = C.c_void_p(None)


@pytest.fixture(scope="module")
def lib():
    from pda_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def bufs():
    """Two distinct non-null addresses (never dereferenced)."""
    keep = C.create_string_buffer(4096)
    at = C.addressof(keep)
    yield C.c_void_p(at), C.c_void_p(at + 64)
    del keep


def entry_points(lib, b, c):
    """name -> (call, has a device counter); call(**what differs from a sound call).  out_a / out_b: pos and neg (negs for SSM)."""
    def triplets(users=b, indptr=b, indices=b, out_a=b, out_b=b, gen=1, n_pool=9, B=8, lo=0, hi=12, pop=NULL, pos_pop=NULL, n_slots=0):
        return lib.pda_sample_triplets(users, gen, NULL, n_pool, B, indptr, indices, NULL, lo, hi, pop, n_slots, 1, 1, out_a, out_b, pos_pop, NULL, NULL)

    def triplets_dev(users=b, indptr=b, indices=b, out_a=b, out_b=b, gen=1, n_pool=9, B=8, lo=0, hi=12, pop=NULL, pos_pop=NULL, n_slots=0, step_dev=b,
                     step_next=c):
        return lib.pda_sample_triplets_dev(users, gen, NULL, n_pool, B, indptr, indices, NULL, lo, hi, pop, n_slots, 1, step_dev, step_next, out_a, out_b,
                                           pos_pop, NULL, NULL)

    def batches_dev(users=b, indptr=b, indices=b, out_a=b, out_b=b, gen=1, n_pool=9, B=8, lo=0, hi=12, pop=NULL, pos_pop=NULL, n_slots=0, step_dev=b,
                    step_next=c, n=3):
        return lib.pda_sample_batches_dev(users, gen, NULL, n_pool, B, n, indptr, indices, NULL, lo, hi, pop, n_slots, 1, step_dev, step_next, out_a,
                                          out_b, pos_pop, NULL, 0, NULL)

    def dice(users=b, indptr=b, indices=b, out_a=b, out_b=b, gen=1, n_pool=9, B=8, n_items=12, order=b, mask=b, margin=3.0):
        return lib.pda_dice_sample(users, gen, NULL, n_pool, B, indptr, indices, n_items, order, b, b, margin, 1, 1, out_a, out_b, mask, NULL)

    def dice_dev(users=b, indptr=b, indices=b, out_a=b, out_b=b, gen=1, n_pool=9, B=8, n_items=12, order=b, mask=b, margin_dev=b, step_dev=b,
                 step_next=c):
        return lib.pda_dice_sample_dev(users, gen, NULL, n_pool, B, indptr, indices, n_items, order, b, b, margin_dev, 1, step_dev, step_next, out_a, out_b,
                                       mask, NULL)

    def ssm(users=b, indptr=b, indices=b, out_a=b, out_b=b, gen=1, n_pool=9, B=8, N=4, lo=0, hi=12):
        return lib.pda_ssm_sample(users, gen, NULL, n_pool, B, N, indptr, indices, lo, hi, 1, 1, out_a, out_b, NULL)

    def ssm_dev(users=b, indptr=b, indices=b, out_a=b, out_b=b, gen=1, n_pool=9, B=8, N=4, lo=0, hi=12, step_dev=b, step_next=c):
        return lib.pda_ssm_sample_dev(users, gen, NULL, n_pool, B, N, indptr, indices, lo, hi, 1, step_dev, step_next, out_a, out_b, NULL)

    return {"pda_sample_triplets": (triplets, False), "pda_sample_triplets_dev": (triplets_dev, True), "pda_sample_batches_dev": (batches_dev, True),
            "pda_dice_sample": (dice, False), "pda_dice_sample_dev": (dice_dev, True), "pda_ssm_sample": (ssm, False),
            "pda_ssm_sample_dev": (ssm_dev, True)}


NAMES = ["pda_sample_triplets", "pda_sample_triplets_dev", "pda_sample_batches_dev", "pda_dice_sample", "pda_dice_sample_dev", "pda_ssm_sample",
         "pda_ssm_sample_dev"]


@pytest.mark.parametrize("name", NAMES)
def test_every_entry_point_makes_the_shared_checks(lib, bufs, name):
    b, c = bufs
    call, counter = entry_points(lib, b, c)[name]
    for arg in ("users", "indptr", "indices", "out_a", "out_b"):
        assert call(**{arg: NULL}) == ERR_ARG, arg
    assert call(gen=1, n_pool=0) == ERR_ARG and call(gen=1, n_pool=-4) == ERR_ARG        # users to be drawn from an empty pool
    assert call(B=0) == ERR_ARG and call(B=-1) == ERR_ARG
    if counter:
        assert call(step_dev=NULL) == ERR_ARG                            # a missing counter
        assert call(step_dev=NULL, step_next=NULL) == ERR_ARG
        assert call(step_dev=b, step_next=b) == ERR_ARG                  # step + 1 stored where other workgroups still read the step


def test_the_limits_that_are_an_entry_point_s_own(lib, bufs):
    b, c = bufs
    ep = {k: v[0] for k, v in entry_points(lib, b, c).items()}
    # the triplet sampler: the range of negatives, the popularity outputs with a popularity matrix, the number of batches
    for name in ("pda_sample_triplets", "pda_sample_triplets_dev", "pda_sample_batches_dev"):
        assert ep[name](lo=5, hi=5) == ERR_ARG and ep[name](lo=6, hi=5) == ERR_ARG
        assert ep[name](pop=b, pos_pop=NULL, n_slots=3) == ERR_ARG and ep[name](pop=b, pos_pop=b, n_slots=3) == ERR_ARG       # (neg_pop is null)
        assert ep[name](pop=b, pos_pop=b, n_slots=0) == ERR_ARG
    assert ep["pda_sample_batches_dev"](n=0) == ERR_ARG and ep["pda_sample_batches_dev"](n=65536) == ERR_ARG
    # the SSM sampler: B <= 2^22 (the [B, N] block is indexed in 32 bits), 1 <= N <= 256, the range of negatives
    for name in ("pda_ssm_sample", "pda_ssm_sample_dev"):
        assert ep[name](B=(1 << 22) + 1) == ERR_ARG
        assert ep[name](N=0) == ERR_ARG and ep[name](N=257) == ERR_ARG and ep[name](lo=5, hi=5) == ERR_ARG
    # PNSM: the catalogue and its three arrays, the mask; the margin by value must be >= 0 (a NaN is not), the one in device memory must be there
    for name in ("pda_dice_sample", "pda_dice_sample_dev"):
        assert ep[name](n_items=0) == ERR_ARG and ep[name](order=NULL) == ERR_ARG and ep[name](mask=NULL) == ERR_ARG
    assert ep["pda_dice_sample"](margin=-1.0) == ERR_ARG and ep["pda_dice_sample"](margin=float("nan")) == ERR_ARG
    assert ep["pda_dice_sample_dev"](margin_dev=NULL) == ERR_ARG
