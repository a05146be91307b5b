"""grlbwt_merge_* on the serial stand-in (CPU): the cases and checkers of tests/merge_cases.py, each on a plain context and on
one with 64-bit positions.  (The stand-in runs a round through the generic primitives -- gathered keys and a stable sort --
and everything around the round as the HIP library does.)"""
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import merge_cases as mc

FLAGS = (0, engine.FLAG_FORCE_IDX64)


@pytest.fixture(scope="module")
def sim():
    from tests import simlib
    return simlib.sim_library()


@pytest.fixture(scope="module")
def ctxs(sim):
    with engine.Context(0, FLAGS[0], sim) as a, engine.Context(0, FLAGS[1], sim) as b:
        yield (a, b), fc.Mem(False)


def test_inputs_are_sized_by_the_tile(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_sizes_follow_the_tile(ctx, flags, ctxs[1], sim)


@pytest.mark.parametrize("name", mc.PAIR_NAMES)
def test_merge_equals_the_build_of_the_concatenation(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_pair(ctx, flags, ctxs[1], sim, name)


def test_foreign_encodings_merge_to_the_same_bytes(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_foreign(ctx, flags, ctxs[1], sim)


def test_merging_is_associative(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_associativity(ctx, flags, ctxs[1], sim)


@pytest.mark.parametrize("name", ["rows_tile_plus_1", "wide_u64", "two_bytes"])
def test_merged_image_inverts_to_the_concatenated_text(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_round_trip(ctx, flags, ctxs[1], sim, name)


def test_max_rounds(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_max_rounds(ctx, flags, ctxs[1], sim)


def test_refusals(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_refusals(ctx, flags, ctxs[1], sim)


def test_merges_outlive_their_context_without_a_fault(sim):
    mc.run_handles_outlive_the_context(fc.Mem(False), sim)


def test_merge_files(sim, ctxs, tmp_path):
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_files(ctx, flags, ctxs[1], sim, tmp_path)


def test_selftest_covers_the_round(sim, ctxs):
    """the round primitive's check inside grlbwt_selftest, at a size of a few tiles"""
    assert ctxs[0][0].selftest(20000, 11) == 0
