"""grlbwt_cdebruijn_* on the HIP library: the cases and checkers of tests/cdebruijn_cases.py, each on a plain context and on one with
64-bit positions: the mate pass and both passes of the edge search under the LDS top level, the fused merge, the tile kernel of
the unitigs' first cells and the walks of the - nodes without a mate as tickets.  (The generic forms are the stand-in's; the
product library does not compile the development switch that selects them on the device, so tools/gpu_fm_cdebruijn.py compares
the two forms there, on a development library.)"""
import pytest

from grlbwt_amd import engine
from tests import cdebruijn_cases as cd
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


@pytest.mark.parametrize("name", cd.TARGETS)
def test_nodes_around_the_tile_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_nodes_around_the_tile(ctx, flags, ctxs[1], hip, name)


@pytest.mark.parametrize("name", cd.TARGETS)
def test_cells_around_the_tile_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_cells_around_the_tile(ctx, flags, ctxs[1], hip, name)


def test_one_strand_and_both_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_strands(ctx, flags, ctxs[1], hip)


def test_all_nodes_rigid_is_the_plain_graph_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_all_rigid(ctx, flags, ctxs[1], hip)


def test_hairpins_palindromes_loops_cycles_branches_filters_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_shapes(ctx, flags, ctxs[1], hip)


def test_values_of_k_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_values_of_k(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("name", ["two_bytes", "wide_u64"])
def test_pairs_over_other_alphabets_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_other_alphabets(ctx, flags, ctxs[1], hip, name)


def test_each_output_alone_and_sizing_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_outputs_and_sizing(ctx, flags, ctxs[1], hip)


def test_refusals_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_refusals(ctx, flags, ctxs[1], hip)


def test_index_is_unchanged_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_index_unchanged(ctx, flags, ctxs[1], hip)


def test_foreign_images_hip(hip, ctxs):
    done = refused = 0
    for name in wk.FOREIGN:
        for ctx in ctxs[0]:
            d, r = cd.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])
            done, refused = done + d, refused + r
    assert done >= 20            # (the others are refused: by grlbwt_fm_create, by the passes or by the merge as not the BWT of a collection)


@pytest.mark.parametrize("lanes", ["64", "320"])
def test_lanes_that_take_further_tickets_hip(hip, ctxs, monkeypatch, lanes):
    """GRLBWT_WALK_LANES = 64 (one wave) and 320 (five waves): so few lanes work through the heads of the mate pass and through the
    walks of the - nodes without a mate by taking further tickets"""
    monkeypatch.setenv("GRLBWT_QUIET_ENV", "1")
    monkeypatch.setenv("GRLBWT_WALK_LANES", lanes)
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_cells_around_the_tile(ctx, flags, ctxs[1], hip, "tile_plus_1")
        cd.run_shapes(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("top", ["0", "2"])
def test_small_and_no_top_level_hip(hip, ctxs, monkeypatch, top):
    """GRLBWT_FM_TOP_BITS = 0 (the searches read memory alone) and 2 (four keys in LDS)"""
    monkeypatch.setenv("GRLBWT_QUIET_ENV", "1")
    monkeypatch.setenv("GRLBWT_FM_TOP_BITS", top)
    for ctx, flags in zip(ctxs[0], FLAGS):
        cd.run_nodes_around_the_tile(ctx, flags, ctxs[1], hip, "tile_plus_1")
        cd.run_strands(ctx, flags, ctxs[1], hip)
