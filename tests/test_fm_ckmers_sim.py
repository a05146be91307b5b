"""grlbwt_fm_kmers_canonical on the serial stand-in (CPU): the cases and checkers of tests/ckmer_cases.py, each on a plain context
and on one with 64-bit positions.  (The stand-in runs the generic mate pass, the generic decode and a serial spectrum; it reports
the device library's tiles.)"""
import pytest

from grlbwt_amd import engine
from tests import ckmer_cases as cc
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
    with engine.Context(0, FLAGS[0], sim) as a, engine.Context(0, FLAGS[1], sim) as b:
        yield (a, b), fc.Mem(False)


def test_binding_names_the_new_calls():
    assert {"grlbwt_fm_kmers_canonical", "grlbwt_fm_kmers_canonical_info_get"} <= set(engine.ABI_SYMBOLS)
    assert all(hasattr(engine.FmIndex, n) for n in ("canonical_kmers_raw", "canonical_kmers", "canonical_kmer_spectrum", "canonical_kmer_info"))
    assert hasattr(engine, "CkmerInfo")


def test_sizes_follow_the_tiles(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_sizes_follow_the_tiles(ctx, flags, ctxs[1], sim)


@pytest.mark.parametrize("name", cc.ROWS)
def test_rows_around_the_tiles(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_rows(ctx, flags, ctxs[1], sim, name)


def test_both_strands(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_both_strands(ctx, flags, ctxs[1], sim)


def test_heads_around_the_mate_tile(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_heads_around_the_mate_tile(ctx, flags, ctxs[1], sim)


def test_entries_around_the_decode_tile(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_entries_around_the_decode_tile(ctx, flags, ctxs[1], sim)


def test_palindromes(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_palindromes(ctx, flags, ctxs[1], sim)


@pytest.mark.parametrize("name", ["reads_with_n", "rare_symbol", "sigma_256"])
def test_symbols_without_complement(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_no_complement(ctx, flags, ctxs[1], sim, name)


@pytest.mark.parametrize("name", ["two_bytes", "wide_u64"])
def test_maps_over_other_alphabets(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_other_alphabets(ctx, flags, ctxs[1], sim, name)


def test_values_of_k(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_values_of_k(ctx, flags, ctxs[1], sim)


def test_one_symbol(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_one_symbol(ctx, flags, ctxs[1], sim)


def test_filters_windows_and_sizing(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_filters_windows_sizing(ctx, flags, ctxs[1], sim)


def test_spectrum_bins(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_spectrum_bins(ctx, flags, ctxs[1], sim)


def test_refusals(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_refusals(ctx, flags, ctxs[1], sim)


def test_index_is_unchanged(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        cc.run_index_unchanged(ctx, flags, ctxs[1], sim)


def test_foreign_images(sim, ctxs):
    done = refused = 0
    for name in wk.FOREIGN:
        for ctx in ctxs[0]:
            d, r = cc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])
            done, refused = done + d, refused + r
    print("foreign images: %d answered, %d refused" % (done, refused))
    assert done >= cc.FOREIGN_FLOOR      # (the others are refused: by grlbwt_fm_create, by the passes as not the BWT of a collection, or for the separator in a pair)
