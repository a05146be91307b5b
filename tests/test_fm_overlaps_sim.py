"""grlbwt_fm_overlaps / grlbwt_fm_overlaps_of / grlbwt_fm_overlap_targets on the serial stand-in (CPU): the cases and checkers of
tests/overlap_cases.py, each on a plain context and on one with 64-bit positions.  (The stand-in runs the same search functor as
the HIP kernels, one query after the other through prim::for_each and without a top level, and expands the ranges by a for_each
over the entries.)"""
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import overlap_cases as oc

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
    assert {"grlbwt_fm_overlaps", "grlbwt_fm_overlaps_of", "grlbwt_fm_overlap_targets", "grlbwt_fm_overlap_info_get"} <= set(engine.ABI_SYMBOLS)
    assert all(hasattr(engine.FmIndex, n) for n in ("overlaps", "overlaps_of", "overlap_targets", "overlap_info"))


def test_read_set_is_not_vacuous():
    """On the brute-force values alone, for the collection made for overlaps (67 strings, 114 queries): hits at every L from 2 to
    30; a range of three strings or more; a string that overlaps itself with a proper suffix (the periodic read); a query of 8
    cells or more without a hit at min_len 8.  Every collection has a query with a hit and one with none."""
    assert hasattr(engine.FmIndex, "overlaps")
    ex = oc.expected("reads")
    assert len(ex.strs) == oc.N_STRIDE + 14 == 67 and sum(1 for s in ex.strs if not s) == 2
    oc.not_vacuous(ex)
    for name in oc.NAMES:
        n = [len(hs) for hs in oc.expected(name).full]
        assert max(n) >= 1 and min(n) == 0, (name, n)


@pytest.mark.parametrize("name", oc.NAMES)
def test_overlaps_against_the_text(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        oc.run_collection(ctx, flags, ctxs[1], sim, name)


def test_targets_around_the_tile_boundaries(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        oc.run_tile_ranges(ctx, flags, ctxs[1], sim)


def test_launch_shapes(sim, ctxs):
    def serial(n, info):
        assert (info["walk_lanes"], info["lane_refills"]) == (n, 0)

    for ctx, flags in zip(ctxs[0], FLAGS):
        oc.run_shapes(ctx, flags, ctxs[1], sim, serial)


def test_refusals(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        oc.run_refusals(ctx, flags, ctxs[1], sim)


def test_overlaps_on_foreign_images(ctxs):
    hits = 0
    for name in fc.FOREIGN:
        for ctx in ctxs[0]:
            hits += oc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])
    assert hits >= 50
