"""grlbwt_cdebruijn_* on the serial stand-in (CPU): the cases and checkers of tests/cdebruijn_cases.py, each on a plain context and
on one with 64-bit positions.  (The stand-in runs the generic forms; it reports the device library's tiles.)"""
import pytest

from grlbwt_amd import engine
from tests import cdebruijn_cases as cd
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
    names = {"grlbwt_cdebruijn_create", "grlbwt_cdebruijn_destroy", "grlbwt_cdebruijn_info_get", "grlbwt_cdebruijn_nodes", "grlbwt_cdebruijn_links",
             "grlbwt_cdebruijn_unitigs"}
    assert names <= set(engine.ABI_SYMBOLS)
    assert hasattr(engine.FmIndex, "de_bruijn_canonical") and hasattr(engine, "CDeBruijnInfo")
    assert all(hasattr(engine.CanonicalDeBruijn, n) for n in ("info", "nodes", "links", "unitigs", "nodes_raw", "links_raw", "unitigs_raw"))


@pytest.mark.parametrize("name", cd.TARGETS)
def test_nodes_around_the_tile(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_nodes_around_the_tile(ctx, flags, ctxs[1], sim, name)


@pytest.mark.parametrize("name", cd.TARGETS)
def test_cells_around_the_tile(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_cells_around_the_tile(ctx, flags, ctxs[1], sim, name)


def test_one_strand_and_both(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_strands(ctx, flags, ctxs[1], sim)


def test_all_nodes_rigid_is_the_plain_graph(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_all_rigid(ctx, flags, ctxs[1], sim)


def test_hairpins_palindromes_loops_cycles_branches_filters(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_shapes(ctx, flags, ctxs[1], sim)


def test_values_of_k(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_values_of_k(ctx, flags, ctxs[1], sim)


@pytest.mark.parametrize("name", ["two_bytes", "wide_u64"])
def test_pairs_over_other_alphabets(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_other_alphabets(ctx, flags, ctxs[1], sim, name)


def test_each_output_alone_and_sizing(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_outputs_and_sizing(ctx, flags, ctxs[1], sim)


def test_refusals(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_refusals(ctx, flags, ctxs[1], sim)


def test_index_is_unchanged(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_index_unchanged(ctx, flags, ctxs[1], sim)


def test_foreign_images(sim, ctxs):
    done = refused = 0
    for name in wk.FOREIGN:
        for ctx in ctxs[0]:
            d, r = cd.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])
            done, refused = done + d, refused + r
    assert done >= 20            # (the others are refused: by grlbwt_fm_create, by the passes or by the merge as not the BWT of a collection)
