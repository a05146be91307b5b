"""grlbwt_fm_kmers_canonical on the HIP library: the cases and checkers of tests/ckmer_cases.py, each on a plain context and on one
with 64-bit positions: the ticket kernel of the mate pass under the LDS top level, the LDS spectrum over the representatives and
the tile decode."""
import pytest

from grlbwt_amd import engine
from tests import ckmer_cases as cc
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


def test_sizes_follow_the_tiles_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_sizes_follow_the_tiles(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("name", cc.ROWS)
def test_rows_around_the_tiles_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_rows(ctx, flags, ctxs[1], hip, name)


def test_both_strands_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_both_strands(ctx, flags, ctxs[1], hip)


def test_heads_around_the_mate_tile_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_heads_around_the_mate_tile(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("lanes", ["64", "320"])
def test_lanes_that_take_further_tickets_hip(hip, ctxs, monkeypatch, lanes):
    """GRLBWT_WALK_LANES = 64 (one wave) and 320 (five waves over one workgroup): unset, these inputs have fewer heads than the device
    has lanes and no lane takes a second ticket; so few lanes work through every head by refilling"""
    monkeypatch.setenv("GRLBWT_QUIET_ENV", "1")
    monkeypatch.setenv("GRLBWT_WALK_LANES", lanes)
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_rows(ctx, flags, ctxs[1], hip, "rows_tile_plus_1")
        cc.run_both_strands(ctx, flags, ctxs[1], hip)
        cc.run_heads_around_the_mate_tile(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("top", ["0", "2"])
def test_small_and_no_top_level_hip(hip, ctxs, monkeypatch, top):
    """GRLBWT_FM_TOP_BITS = 0 (the searches read memory alone) and 2 (four keys in LDS beside the complement table)"""
    monkeypatch.setenv("GRLBWT_QUIET_ENV", "1")
    monkeypatch.setenv("GRLBWT_FM_TOP_BITS", top)
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_rows(ctx, flags, ctxs[1], hip, "rows_tile")
        cc.run_no_complement(ctx, flags, ctxs[1], hip, "reads_with_n")


def test_entries_around_the_decode_tile_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_entries_around_the_decode_tile(ctx, flags, ctxs[1], hip)


def test_palindromes_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_palindromes(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("name", ["reads_with_n", "rare_symbol", "sigma_256"])
def test_symbols_without_complement_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_no_complement(ctx, flags, ctxs[1], hip, name)


@pytest.mark.parametrize("name", ["two_bytes", "wide_u64"])
def test_maps_over_other_alphabets_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_other_alphabets(ctx, flags, ctxs[1], hip, name)


def test_values_of_k_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_values_of_k(ctx, flags, ctxs[1], hip)


def test_one_symbol_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_one_symbol(ctx, flags, ctxs[1], hip)


def test_filters_windows_and_sizing_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_filters_windows_sizing(ctx, flags, ctxs[1], hip)


def test_spectrum_bins_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_spectrum_bins(ctx, flags, ctxs[1], hip)


def test_refusals_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_refusals(ctx, flags, ctxs[1], hip)


def test_index_is_unchanged_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_index_unchanged(ctx, flags, ctxs[1], hip)


def test_foreign_images_hip(hip, ctxs):
    done = refused = 0
    for name in wk.FOREIGN:
        for ctx in ctxs[0]:
            d, r = cc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])
            done, refused = done + d, refused + r
    print("foreign images: %d answered, %d refused" % (done, refused))
    assert done >= cc.FOREIGN_FLOOR      # (the others are refused: by grlbwt_fm_create, by the passes as not the BWT of a collection, or for the separator in a pair)
