"""grlbwt_fm_match / grlbwt_fm_mems on the serial stand-in (CPU): the cases and checkers of tests/match_cases.py, each on a plain
context and on one with 64-bit positions.  (The stand-in runs the same functor as the HIP kernel, one cell after the other
through prim::for_each and without a top level.)"""
import numpy as np
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import match_cases as mc

FLAGS = (0, engine.FLAG_FORCE_IDX64)


@pytest.fixture(scope="module")
def sim():
    from tests import simlib
    return simlib.sim_library()


@pytest.fixture(scope="module")
def ctxs(sim):
    with engine.Context(0, FLAGS[0], sim) as a, engine.Context(0, FLAGS[1], sim) as b:
        yield (a, b), fc.Mem(False)


def test_binding_names_the_new_calls():
    assert {"grlbwt_fm_match", "grlbwt_fm_mems", "grlbwt_fm_match_info_get"} <= set(engine.ABI_SYMBOLS)
    assert all(hasattr(engine.FmIndex, n) for n in ("match", "mems", "match_info"))


def test_pattern_set_is_not_vacuous():
    """On the brute-force values alone, for the DNA collection: at least a third of the ends have a match of 8 cells, a fifth reach
    the cap of 16, 40 ends have none, there are 30 distinct lengths and 60 patterns with two or more MEMs of 8 cells.  (The seed
    of match_cases.collection_patterns gives 185 patterns and 5341 ends: 59 % with L >= 8, 31 % with L >= 16, 72 with L = 0,
    61 distinct lengths, 78 such patterns.)"""
    assert hasattr(engine.FmIndex, "match")
    ex = mc.expected("dna")
    mc.not_vacuous(ex)
    for name in fc.COLLECTIONS:
        flat = mc.expected(name).flat
        assert (flat == 0).any() and (flat > 1).any(), name


@pytest.mark.parametrize("name", fc.COLLECTIONS)
def test_match_and_mems_against_the_text(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_collection(ctx, flags, ctxs[1], sim, name)


@pytest.mark.parametrize("name", fc.FOREIGN)
def test_match_on_foreign_images(ctxs, name):
    for ctx in ctxs[0]:
        mc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])


def test_launch_shapes(sim, ctxs):
    def serial(n, n_patterns, info):
        assert (info["walk_lanes"], info["lane_refills"]) == (n, 0)

    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_shapes(ctx, flags, ctxs[1], sim, serial)


def test_refusals(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_refusals(ctx, flags, ctxs[1], sim)


def test_match_lengths_never_grow_by_more_than_one():
    """the fact the MEM rule rests on, on the brute-force values: L[e + 1] <= L[e] + 1 inside every pattern"""
    assert hasattr(engine.FmIndex, "mems")
    for name in fc.COLLECTIONS:
        for L in mc.expected(name).L:
            assert all(b <= a + 1 for a, b in zip(L, L[1:])), name
    assert np.array_equal(mc.expected("dna").capped(16), np.minimum(mc.expected("dna").flat, np.uint64(16)))
