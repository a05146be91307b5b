"""grlbwt_fm_sa on the serial stand-in (CPU): the cases and checkers of tests/sa_cases.py, each on a plain context and on one with
64-bit positions.  (The stand-in walks one ticket after the other: walk_lanes is the number of tickets, and no lane refills.)
Locating every row of the collections of long strings is what the call replaces and what the stand-in cannot afford (header of
tests/walk_cases.py): "equal to locate" runs on the small collections here, on all of them in the GPU file."""
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import sa_cases as sc
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
    assert {"grlbwt_fm_sa", "grlbwt_fm_sa_info_get"} <= set(engine.ABI_SYMBOLS)
    assert all(hasattr(engine.FmIndex, n) for n in ("suffix_array", "sa_info")) and hasattr(engine, "SaInfo")


@pytest.mark.parametrize("name", sc.SMALL)
def test_prefix_doubling_is_pinned_to_the_python_sort(name):
    sc.run_sort_is_pinned(name)


@pytest.mark.parametrize("bits", sc.FORMS, ids=sc.FORM_IDS)
@pytest.mark.parametrize("name", wk.NAMES)
def test_whole_array_against_the_text(sim, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_whole(ctx, flags, ctxs[1], sim, name, bits)


@pytest.mark.parametrize("bits", sc.FORMS, ids=sc.FORM_IDS)
@pytest.mark.parametrize("name", [n for n in wk.NAMES if n not in wk.LARGE])
def test_equal_to_locate(sim, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_equals_locate(ctx, flags, ctxs[1], sim, name, bits)


@pytest.mark.parametrize("name,bits", sc.WINDOW_CASES, ids=sc.WINDOW_IDS)
def test_windows(sim, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_windows(ctx, flags, ctxs[1], sim, name, bits)


@pytest.mark.parametrize("bits", (None, 6), ids=["strings", "segments_b6"])
@pytest.mark.parametrize("name", ("dna", "mixed", "wide_u64"))
def test_one_output_at_a_time(sim, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_one_output(ctx, flags, ctxs[1], sim, name, bits)


@pytest.mark.parametrize("bits", (None, 6), ids=["strings", "segments_b6"])
def test_width_refusals(sim, ctxs, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_width_refusals(ctx, flags, ctxs[1], sim, bits)


@pytest.mark.parametrize("bits", (None, 6), ids=["strings", "segments_b6"])
def test_other_refusals(sim, ctxs, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_refusals(ctx, flags, ctxs[1], sim, bits)


def test_index_is_unchanged(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_index_unchanged(ctx, flags, ctxs[1], sim)


def test_foreign_images(sim, ctxs):
    done = lost = 0
    for name in wk.FOREIGN:
        for ctx in ctxs[0]:
            d, l = sc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])
            done, lost = done + d, lost + l
    assert done >= 20 and lost >= 100            # (some of these images hold rows on no string's chain: the "none" entries)
