"""grlbwt_debruijn_* on the serial stand-in (CPU): the cases and checkers of tests/debruijn_cases.py, each on a plain context and on
one with 64-bit positions.  (The stand-in runs the generic forms; it reports the device library's tiles.)"""
import pytest

from grlbwt_amd import engine
from tests import debruijn_cases as dc
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import walk_cases as wk

FLAGS = (0, engine.FLAG_FORCE_IDX64)


@pytest.fixture(scope="module")
def sim():
    from tests import simlib
    return simlib.sim_library()


@pytest.fixture(scope="module")
def ctxs(sim):
    mem = fc.Mem(False)
    with engine.Context(0, FLAGS[0], sim) as a, engine.Context(0, FLAGS[1], sim) as b:
        yield (a, b), mem


def test_binding_names_the_new_calls():
    names = {"grlbwt_debruijn_create", "grlbwt_debruijn_destroy", "grlbwt_debruijn_info_get", "grlbwt_debruijn_nodes", "grlbwt_debruijn_edges",
             "grlbwt_debruijn_unitigs"}
    assert names <= set(engine.ABI_SYMBOLS)
    assert hasattr(engine.FmIndex, "de_bruijn") and hasattr(engine, "DeBruijnInfo")
    assert all(hasattr(engine.DeBruijn, n) for n in ("info", "nodes", "edges", "unitigs", "nodes_raw", "edges_raw", "unitigs_raw"))


@pytest.mark.parametrize("name", dc.NODE_TARGETS)
def test_nodes_around_the_edge_tile(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_nodes_around_the_edge_tile(ctx, flags, ctxs[1], sim, name)


@pytest.mark.parametrize("name", dc.CELL_TARGETS)
def test_cells_around_the_decode_tile(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_cells_around_the_decode_tile(ctx, flags, ctxs[1], sim, name)


def test_cycles(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_cycles(ctx, flags, ctxs[1], sim)


def test_branches(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_branches(ctx, flags, ctxs[1], sim)


def test_filters(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_filters(ctx, flags, ctxs[1], sim)


def test_values_of_k(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_values_of_k(ctx, flags, ctxs[1], sim)


@pytest.mark.parametrize("name", dc.SMALL)
def test_smaller_collections(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_small(ctx, flags, ctxs[1], sim, name)


def test_each_output_alone_and_sizing(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_outputs_and_sizing(ctx, flags, ctxs[1], sim)


def test_refusals(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_refusals(ctx, flags, ctxs[1], sim)


def test_index_is_unchanged(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_index_unchanged(ctx, flags, ctxs[1], sim)


def test_foreign_images(sim, ctxs):
    done = refused = 0
    for name in wk.FOREIGN:
        for ctx in ctxs[0]:
            d, r = dc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])
            done, refused = done + d, refused + r
    assert done >= 20            # (the others are refused: by grlbwt_fm_create, or by the passes as not the BWT of a collection)
