"""grlbwt_fm_repeats on the serial stand-in (CPU): the cases and checkers of tests/repeat_cases.py, each on a plain context and on
one with 64-bit positions.  (The stand-in runs the generic form: searches in the tree in memory; it reports the device library's
tile.  The staircase that crosses a node of the second level above the tiles runs on the device only.)"""
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import repeat_cases as rc
from tests import walk_cases as wk

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
    assert {"grlbwt_fm_repeats", "grlbwt_fm_repeat_info_get"} <= set(engine.ABI_SYMBOLS)
    assert all(hasattr(engine.FmIndex, n) for n in ("repeats_raw", "repeats", "repeat_info")) and hasattr(engine, "RepeatInfo")


def test_sizes_follow_the_shape(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        rc.run_sizes_follow_the_shape(ctx, flags, ctxs[1], sim)


@pytest.mark.parametrize("name", rc.ROWS + rc.SMALL)
def test_collections(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        rc.run_collection(ctx, flags, ctxs[1], sim, name)


def test_staircases(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        rc.run_staircases(ctx, flags, ctxs[1], sim, False)


def test_filters(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        rc.run_filters(ctx, flags, ctxs[1], sim)


def test_row_windows(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        rc.run_windows(ctx, flags, ctxs[1], sim)


def test_each_output_alone_and_sizing(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        rc.run_outputs_and_sizing(ctx, flags, ctxs[1], sim)


def test_refusals(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        rc.run_refusals(ctx, flags, ctxs[1], sim)


def test_index_is_unchanged(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        rc.run_index_unchanged(ctx, flags, ctxs[1], sim)


def test_cross_check_with_locate_extract_count(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        rc.run_cross_check(ctx, flags, ctxs[1], sim)


def test_foreign_images(sim, ctxs):
    done = refused = 0
    for name in wk.FOREIGN:
        for ctx in ctxs[0]:
            d, r = rc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])
            done, refused = done + d, refused + r
    assert done >= 20            # (the others are refused: by grlbwt_fm_create, or by the passes as not the BWT of a collection)
