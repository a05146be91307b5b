"""grlbwt_debruijn_* on the HIP library: the cases and checkers of tests/debruijn_cases.py, each on a plain context and on one with
64-bit positions: both passes of the edge search under the LDS top level and the tile kernel of the unitigs' first cells.  (The
generic form of the first cells is the stand-in's; the product library does not compile the development switch that selects it
on the device, so tools/gpu_fm_debruijn.py compares the two forms there, on a development library.)"""
import pytest

from grlbwt_amd import engine
from tests import debruijn_cases as dc
from tests import fm_cases as fc
from tests import image_cases as ic
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


@pytest.mark.parametrize("name", dc.NODE_TARGETS)
def test_nodes_around_the_edge_tile_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_nodes_around_the_edge_tile(ctx, flags, ctxs[1], hip, name)


@pytest.mark.parametrize("name", dc.CELL_TARGETS)
def test_cells_around_the_decode_tile_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_cells_around_the_decode_tile(ctx, flags, ctxs[1], hip, name)


def test_cycles_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_cycles(ctx, flags, ctxs[1], hip)


def test_branches_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_branches(ctx, flags, ctxs[1], hip)


def test_filters_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_filters(ctx, flags, ctxs[1], hip)


def test_values_of_k_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_values_of_k(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("name", dc.SMALL)
def test_smaller_collections_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_small(ctx, flags, ctxs[1], hip, name)


def test_each_output_alone_and_sizing_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_outputs_and_sizing(ctx, flags, ctxs[1], hip)


def test_refusals_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_refusals(ctx, flags, ctxs[1], hip)


def test_index_is_unchanged_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_index_unchanged(ctx, flags, ctxs[1], hip)


def test_foreign_images_hip(hip, ctxs):
    done = refused = 0
    for name in wk.FOREIGN:
        for ctx in ctxs[0]:
            d, r = dc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])
            done, refused = done + d, refused + r
    assert done >= 20            # (the others are refused: by grlbwt_fm_create, or by the passes as not the BWT of a collection)
