"""grlbwt_docs_* on the HIP library: the cases and checkers of tests/docs_cases.py, each on a plain context and on one with 64-bit
positions.  Here the queries run the two tile kernels (prim::docs_flags, and prim::docs_emit where no occurrences are asked for:
cases 3 and 4 list without them too): the shapes of case 2 put more than 256 range starts into one tile, a range over four tiles
and more than 180 tiles into one launch."""
import pytest

from grlbwt_amd import engine
from tests import docs_cases as dc
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
    mem = dc.fc.Mem(True)
    with engine.Context(0, FLAGS[0], hip) as a, engine.Context(0, FLAGS[1], hip) as b:
        yield (a, b), mem


@pytest.mark.parametrize("bits", dc.FORMS, ids=dc.FORM_IDS)
@pytest.mark.parametrize("name", dc.NAMES)
def test_ranges_of_counted_patterns_hip(hip, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_counted(ctx, flags, ctxs[1], hip, name, bits)


@pytest.mark.parametrize("bits", (None, 6), ids=["strings", "segments_b6"])
@pytest.mark.parametrize("name", ("reads3000", "mixed"))
def test_shapes_that_can_break_a_tile_kernel_hip(hip, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_shapes(ctx, flags, ctxs[1], hip, name, bits)


@pytest.mark.parametrize("bits", (None, 6), ids=["strings", "segments_b6"])
@pytest.mark.parametrize("name", ("dna", "reads3000", "wide_u64"))
def test_one_output_at_a_time_hip(hip, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_one_output(ctx, flags, ctxs[1], hip, name, bits)


@pytest.mark.parametrize("bits", (None, 6), ids=["strings", "segments_b6"])
@pytest.mark.parametrize("name", ("repeats", "reads3000"))
def test_occurrences_hip(hip, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_occurrences(ctx, flags, ctxs[1], hip, name, bits)


@pytest.mark.parametrize("bits", (None, 6), ids=["strings", "segments_b6"])
def test_refusals_hip(hip, ctxs, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_refusals(ctx, flags, ctxs[1], hip, bits)


def test_index_is_unchanged_and_the_handle_outlives_it_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        dc.run_index_unchanged(ctx, flags, ctxs[1], hip)


def test_foreign_images_hip(ctxs):
    made = refused = 0
    for name in wk.FOREIGN:
        for ctx in ctxs[0]:
            m, r = dc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])
            made, refused = made + m, refused + r
    assert made >= 1 and refused >= 1            # both outcomes occur: BWTs of collections, and images with rows on no string's chain
