"""grlbwt_fm_kmers on the serial stand-in (CPU): the cases and checkers of tests/kmer_cases.py, each on a plain context and on one
with 64-bit positions.  (The stand-in runs the generic decode and a serial spectrum; it reports the device library's tiles.)"""
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import kmer_cases as kc
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
    assert {"grlbwt_fm_kmers", "grlbwt_fm_kmer_info_get"} <= set(engine.ABI_SYMBOLS)
    assert all(hasattr(engine.FmIndex, n) for n in ("kmers", "kmer_spectrum", "kmer_info")) and hasattr(engine, "KmerInfo")


def test_sizes_follow_the_tiles(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_sizes_follow_the_tiles(ctx, flags, ctxs[1], sim)


@pytest.mark.parametrize("name", kc.ROWS)
def test_rows_around_the_tiles(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_rows(ctx, flags, ctxs[1], sim, name)


def test_entries_around_the_decode_tile(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_entries_around_the_decode_tile(ctx, flags, ctxs[1], sim)


def test_values_of_k(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_values_of_k(ctx, flags, ctxs[1], sim)


def test_early_distinct(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_early_distinct(ctx, flags, ctxs[1], sim)


def test_one_symbol(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_one_symbol(ctx, flags, ctxs[1], sim)


@pytest.mark.parametrize("name", kc.SMALL)
def test_smaller_collections(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_small(ctx, flags, ctxs[1], sim, name)


def test_each_output_alone_and_sizing(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_outputs_and_sizing(ctx, flags, ctxs[1], sim)


def test_spectrum_bins(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_spectrum_bins(ctx, flags, ctxs[1], sim)


def test_row_windows(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_row_windows(ctx, flags, ctxs[1], sim)


def test_refusals(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_refusals(ctx, flags, ctxs[1], sim)


def test_index_is_unchanged(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        kc.run_index_unchanged(ctx, flags, ctxs[1], sim)


def test_foreign_images(sim, ctxs):
    done = refused = 0
    for name in wk.FOREIGN:
        for ctx in ctxs[0]:
            d, r = kc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])
            done, refused = done + d, refused + r
    assert done >= 20            # (the others are refused: by grlbwt_fm_create, or by the passes as not the BWT of a collection)
