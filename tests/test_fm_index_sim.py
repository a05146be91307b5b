"""grlbwt_fm_* on the serial stand-in (CPU): the cases and checkers of tests/fm_cases.py, each on a plain context and on one
with 64-bit positions.  (The stand-in calls the same step function as the HIP kernel, through prim::for_each and without
a top level.)"""
import numpy as np
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic

FLAGS = (0, engine.FLAG_FORCE_IDX64)


@pytest.fixture(scope="module")
def sim():
    from tests import simlib
    return simlib.sim_library()


@pytest.fixture(scope="module")
def ctxs(sim):
    with engine.Context(0, FLAGS[0], sim) as a, engine.Context(0, FLAGS[1], sim) as b:
        yield (a, b), fc.Mem(False)


def test_pattern_sets_are_not_vacuous():
    """On the brute-force results themselves: in every collection at least half of the patterns occur, one in ten does not."""
    for col in fc.COLS.values():
        fc.expected_counts(col, fc.collection_patterns(col))
    assert len(fc.FOREIGN) >= 40 and any(ic.BY_NAME[n].giant for n in fc.FOREIGN)


@pytest.mark.parametrize("name", fc.FOREIGN)
def test_count_on_foreign_images(ctxs, name):
    for ctx in ctxs[0]:
        fc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])


@pytest.mark.parametrize("name", fc.COLLECTIONS)
def test_count_and_locate_against_the_text(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        fc.run_collection(ctx, flags, ctxs[1], sim, name)


def test_launch_shapes(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        fc.run_shapes(ctx, flags, ctxs[1], sim)


def test_refusals(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        fc.run_refusals(ctx, flags, ctxs[1], sim)


def test_index_outlives_its_context_without_a_fault(sim):
    """grlbwt_ctx_destroy releases the indexes still alive; closing such an index afterwards touches nothing."""
    mem = fc.Mem(False)
    col = fc.COLS["identical"]
    blob = fc.image_of(sim, col, 0)
    keep, img = mem.put(blob)
    ctx = engine.Context(0, 0, sim)
    fm = engine.FmIndex(ctx, img, len(blob), locate=True)
    other = engine.FmIndex(ctx, img, len(blob))
    assert fc.count(fm, mem, [[]], 1) == [(0, col.n)]
    other.close()
    ctx.close()
    fm.close()
    fm.close()
    with engine.Context(0, 0, sim) as ctx2, engine.FmIndex(ctx2, img, len(blob)) as fm2:      # the library is as it was
        assert fc.count(fm2, mem, [[]], 1) == [(0, col.n)]
