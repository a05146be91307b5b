"""grlbwt_merge_* on the HIP library: the cases and checkers of tests/merge_cases.py, each on a plain context and on one with
64-bit positions.  The rounds are the three kernels of prim::MgRound; the inputs are sized from the tile they report."""
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import merge_cases as mc

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


def test_inputs_are_sized_by_the_tile_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_sizes_follow_the_tile(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("name", mc.PAIR_NAMES)
def test_merge_equals_the_build_of_the_concatenation_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_pair(ctx, flags, ctxs[1], hip, name)


def test_foreign_encodings_merge_to_the_same_bytes_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_foreign(ctx, flags, ctxs[1], hip)


def test_merging_is_associative_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_associativity(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("name", ["rows_tile_plus_1", "wide_u64", "two_bytes"])
def test_merged_image_inverts_to_the_concatenated_text_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_round_trip(ctx, flags, ctxs[1], hip, name)


def test_max_rounds_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_max_rounds(ctx, flags, ctxs[1], hip)


def test_refusals_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_refusals(ctx, flags, ctxs[1], hip)


def test_merges_outlive_their_context_without_a_fault_hip(hip, ctxs):
    mc.run_handles_outlive_the_context(ctxs[1], hip)


def test_merge_files_hip(hip, ctxs, tmp_path):
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_files(ctx, flags, ctxs[1], hip, tmp_path)


@pytest.mark.parametrize("name", ["rows_three_tiles_17", "disjoint_alphabets", "sigma_256"])
def test_sort_form_of_the_round_gives_the_same_merge_hip(hip, ctxs, monkeypatch, name):
    """GRLBWT_MERGE_ROUND=sort: a round as gathered keys and the radix sort's pass -- the form the fused kernels are measured
    against (tools/gpu_image_merge.py) has to be a merge too"""
    monkeypatch.setenv("GRLBWT_QUIET_ENV", "1")
    monkeypatch.setenv("GRLBWT_MERGE_ROUND", "sort")
    for ctx, flags in zip(ctxs[0], FLAGS):
        mc.run_pair(ctx, flags, ctxs[1], hip, name)
