"""grlbwt_select_* on the serial stand-in (CPU): the cases and checkers of tests/select_cases.py, each on a plain context and on
one with 64-bit positions.  (The stand-in reaches the marking functors through WalkSerialFn, one ticket after the other, and runs
everything around the walks as the HIP library does.)"""
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import select_cases as sc

FLAGS = (0, engine.FLAG_FORCE_IDX64)


@pytest.fixture(scope="module")
def sim():
    from tests import simlib
    return simlib.sim_library()


@pytest.fixture(scope="module")
def ctxs(sim):
    with engine.Context(0, FLAGS[0], sim) as a, engine.Context(0, FLAGS[1], sim) as b:
        yield (a, b), fc.Mem(False)


@pytest.mark.parametrize("name", list(sc.DNA_LISTS))
def test_drop_and_keep_equal_the_build_of_the_remaining_text(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_dna_list(ctx, flags, ctxs[1], sim, name)


@pytest.mark.parametrize("name", sc.EDGE_NAMES)
def test_word_edges_of_the_two_bit_vectors(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_edge(ctx, flags, ctxs[1], sim, name)


@pytest.mark.parametrize("name", list(sc.HEADERS))
def test_header_widths_follow_the_remaining_strings(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_header(ctx, flags, ctxs[1], sim, name)


def test_runs_that_become_neighbours_are_joined(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_runs_join(ctx, flags, ctxs[1], sim)


@pytest.mark.parametrize("name", ["two_bytes", "wide_u64"])
def test_wide_symbols_and_the_output_inverts(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_wide(ctx, flags, ctxs[1], sim, name)


@pytest.mark.parametrize("bits", sc.CP_BITS)
@pytest.mark.parametrize("name", ["mixed", "repeats"])
def test_checkpointed_form_equals_the_per_string_form(sim, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_checkpointed(ctx, flags, ctxs[1], sim, name, bits)


def test_checkpointed_form_on_the_dna_collection(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_checkpointed_dna(ctx, flags, ctxs[1], sim)


def test_select_undoes_the_merge_and_the_merge_undoes_select(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_merge_algebra(ctx, flags, ctxs[1], sim)


def test_foreign_encodings_select_to_the_same_bytes(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_foreign(ctx, flags, ctxs[1], sim)


@pytest.mark.parametrize("name", sc.FOREIGN)
def test_images_of_no_collection_give_a_refusal_or_a_result(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_not_a_collection(ctx, flags, ctxs[1], ic.BY_NAME[name])


def test_refusals(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_refusals(ctx, flags, ctxs[1], sim)


def test_selections_outlive_their_context_without_a_fault(sim):
    sc.run_handles_outlive_the_context(fc.Mem(False), sim)


def test_select_files(sim, ctxs, tmp_path):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_files(ctx, flags, ctxs[1], sim, tmp_path)
