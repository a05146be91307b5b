"""grlbwt_docs_* on the serial stand-in (CPU): the cases and checkers of tests/docs_cases.py, each on a plain context and on one
with 64-bit positions.  The stand-in runs the generic form of the queries -- a search per range row and per entry -- which is
also the form the device's tile kernels are measured against."""
import pytest

from grlbwt_amd import engine
from tests import docs_cases as dc
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
        yield (a, b), dc.fc.Mem(False)


def test_binding_names_the_new_calls():
    assert {"grlbwt_docs_create", "grlbwt_docs_destroy", "grlbwt_docs_info_get", "grlbwt_docs_count", "grlbwt_docs_list"} <= set(engine.ABI_SYMBOLS)
    assert hasattr(engine.FmIndex, "documents") and hasattr(engine, "DocsInfo") and engine.DOCS_OCCURRENCES == 1
    assert all(hasattr(engine.FmDocs, n) for n in ("count", "list", "info", "__enter__", "__exit__"))


@pytest.mark.parametrize("bits", dc.FORMS, ids=dc.FORM_IDS)
@pytest.mark.parametrize("name", dc.NAMES)
def test_ranges_of_counted_patterns(sim, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_counted(ctx, flags, ctxs[1], sim, name, bits)


@pytest.mark.parametrize("bits", (None, 6), ids=["strings", "segments_b6"])
@pytest.mark.parametrize("name", ("reads3000", "mixed"))
def test_shapes_that_can_break_a_tile_kernel(sim, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_shapes(ctx, flags, ctxs[1], sim, name, bits)


@pytest.mark.parametrize("bits", (None, 6), ids=["strings", "segments_b6"])
@pytest.mark.parametrize("name", ("dna", "reads3000", "wide_u64"))
def test_one_output_at_a_time(sim, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_one_output(ctx, flags, ctxs[1], sim, name, bits)


@pytest.mark.parametrize("bits", (None, 6), ids=["strings", "segments_b6"])
@pytest.mark.parametrize("name", ("repeats", "reads3000"))
def test_occurrences(sim, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_occurrences(ctx, flags, ctxs[1], sim, name, bits)


@pytest.mark.parametrize("bits", (None, 6), ids=["strings", "segments_b6"])
def test_refusals(sim, ctxs, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_refusals(ctx, flags, ctxs[1], sim, bits)


def test_index_is_unchanged_and_the_handle_outlives_it(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_index_unchanged(ctx, flags, ctxs[1], sim)


def test_foreign_images(sim, ctxs):
    made = refused = 0
    for name in wk.FOREIGN:
        for ctx in ctxs[0]:
            m, r = dc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])
            made, refused = made + m, refused + r
    assert made >= 1 and refused >= 1            # both outcomes occur: BWTs of collections, and images with rows on no string's chain


def test_handles_alive_are_released_with_the_context(sim):
    col = dc.COLS["dna"]
    mem = dc.fc.Mem(False)
    with engine.Context(0, 0, sim) as ctx:
        fm = dc.sc.index(ctx, 0, mem, sim, col, None)
        docs = fm.documents(occurrences=True)
        dc.check(col, docs, mem, [(0, col.n)])
    docs.close()                                 # (a closed context has released its handles: nothing left to do)
    fm.close()
