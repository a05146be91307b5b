"""grlbwt_fm_repeats on the HIP library: the cases and checkers of tests/repeat_cases.py, each on a plain context and on one with
64-bit positions: the minima kernel, the tile search and the emit over the selected rows."""
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import repeat_cases as rc
from tests import walk_cases as wk

pytestmark = pytest.mark.gpu
FLAGS = (0, engine.FLAG_FORCE_IDX64)


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as g
    return g.build_hip()


@pytest.fixture(scope="module")
def ctxs(hip):
    mem = fc.Mem(True)
    with engine.Context(0, FLAGS[0], hip) as a, engine.Context(0, FLAGS[1], hip) as b:
        yield (a, b), mem


def test_sizes_follow_the_shape_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        rc.run_sizes_follow_the_shape(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("name", rc.ROWS + rc.SMALL)
def test_collections_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        rc.run_collection(ctx, flags, ctxs[1], hip, name)


def test_staircases_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        rc.run_staircases(ctx, flags, ctxs[1], hip, True)


def test_filters_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        rc.run_filters(ctx, flags, ctxs[1], hip)


def test_row_windows_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        rc.run_windows(ctx, flags, ctxs[1], hip)


def test_each_output_alone_and_sizing_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        rc.run_outputs_and_sizing(ctx, flags, ctxs[1], hip)


def test_refusals_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        rc.run_refusals(ctx, flags, ctxs[1], hip)


def test_index_is_unchanged_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        rc.run_index_unchanged(ctx, flags, ctxs[1], hip)


def test_cross_check_with_locate_extract_count_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        rc.run_cross_check(ctx, flags, ctxs[1], hip)


def test_foreign_images_hip(hip, ctxs):
    done = refused = 0
    for name in wk.FOREIGN:
        for ctx in ctxs[0]:
            d, r = rc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])
            done, refused = done + d, refused + r
    assert done >= 20            # (the others are refused: by grlbwt_fm_create, or by the passes as not the BWT of a collection)
