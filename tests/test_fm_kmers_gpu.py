"""grlbwt_fm_kmers on the HIP library: the cases and checkers of tests/kmer_cases.py, each on a plain context and on one with 64-bit
positions: the LDS spectrum and the tile decode."""
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import kmer_cases as kc
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
        kc.run_sizes_follow_the_tiles(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("name", kc.ROWS)
def test_rows_around_the_tiles_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_rows(ctx, flags, ctxs[1], hip, name)


def test_entries_around_the_decode_tile_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_entries_around_the_decode_tile(ctx, flags, ctxs[1], hip)


def test_values_of_k_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_values_of_k(ctx, flags, ctxs[1], hip)


def test_early_distinct_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_early_distinct(ctx, flags, ctxs[1], hip)


def test_one_symbol_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_one_symbol(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("name", kc.SMALL)
def test_smaller_collections_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_small(ctx, flags, ctxs[1], hip, name)


def test_each_output_alone_and_sizing_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_outputs_and_sizing(ctx, flags, ctxs[1], hip)


def test_spectrum_bins_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_spectrum_bins(ctx, flags, ctxs[1], hip)


def test_row_windows_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_row_windows(ctx, flags, ctxs[1], hip)


def test_refusals_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_refusals(ctx, flags, ctxs[1], hip)


def test_index_is_unchanged_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_index_unchanged(ctx, flags, ctxs[1], hip)


def test_foreign_images_hip(hip, ctxs):
    done = refused = 0
    for name in wk.FOREIGN:
        for ctx in ctxs[0]:
            d, r = kc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])
            done, refused = done + d, refused + r
    assert done >= 20            # (the others are refused: by grlbwt_fm_create, or by the passes as not the BWT of a collection)
