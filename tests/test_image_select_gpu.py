"""grlbwt_select_* on the HIP library: the cases and checkers of tests/select_cases.py, each on a plain context and on one with
64-bit positions.  The marking walks are prim::walk_tickets over the listed strings or over the checkpoints."""
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import select_cases as sc

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


@pytest.mark.parametrize("name", list(sc.DNA_LISTS))
def test_drop_and_keep_equal_the_build_of_the_remaining_text_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_dna_list(ctx, flags, ctxs[1], hip, name)


@pytest.mark.parametrize("name", sc.EDGE_NAMES)
def test_word_edges_of_the_two_bit_vectors_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_edge(ctx, flags, ctxs[1], hip, name)


def test_lanes_take_the_listed_strings_as_tickets_hip(hip, ctxs, monkeypatch):
    """130 listed strings on 64 lanes: the other 66 are drawn from the ticket word"""
    monkeypatch.setenv("GRLBWT_QUIET_ENV", "1")
    monkeypatch.setenv("GRLBWT_WALK_LANES", "64")
    for ctx, flags in zip(ctxs[0], FLAGS):
        info = sc.run_lanes(ctx, flags, ctxs[1], hip)
        assert info["lane_refills"] == 66


@pytest.mark.parametrize("name", list(sc.HEADERS))
def test_header_widths_follow_the_remaining_strings_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_header(ctx, flags, ctxs[1], hip, name)


def test_runs_that_become_neighbours_are_joined_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_runs_join(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("name", ["two_bytes", "wide_u64"])
def test_wide_symbols_and_the_output_inverts_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_wide(ctx, flags, ctxs[1], hip, name)


@pytest.mark.parametrize("bits", sc.CP_BITS)
@pytest.mark.parametrize("name", ["mixed", "repeats"])
def test_checkpointed_form_equals_the_per_string_form_hip(hip, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_checkpointed(ctx, flags, ctxs[1], hip, name, bits)


def test_checkpointed_form_on_the_dna_collection_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_checkpointed_dna(ctx, flags, ctxs[1], hip)


def test_select_undoes_the_merge_and_the_merge_undoes_select_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_merge_algebra(ctx, flags, ctxs[1], hip)


def test_foreign_encodings_select_to_the_same_bytes_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_foreign(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("name", sc.FOREIGN)
def test_images_of_no_collection_give_a_refusal_or_a_result_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_not_a_collection(ctx, flags, ctxs[1], ic.BY_NAME[name])


def test_refusals_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_refusals(ctx, flags, ctxs[1], hip)


def test_selections_outlive_their_context_without_a_fault_hip(hip, ctxs):
    sc.run_handles_outlive_the_context(ctxs[1], hip)


def test_select_files_hip(hip, ctxs, tmp_path):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_files(ctx, flags, ctxs[1], hip, tmp_path)
