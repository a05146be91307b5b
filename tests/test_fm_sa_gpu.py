"""grlbwt_fm_sa on the HIP library: the cases and checkers of tests/sa_cases.py, each on a plain context and on one with 64-bit
positions.  Here "equal to locate" runs on every collection, the long strings included, and the lanes case runs the storing walk
under GRLBWT_WALK_LANES of 64 (one wave takes every ticket), 320 and unset."""
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import sa_cases as sc
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


@pytest.mark.parametrize("bits", sc.FORMS, ids=sc.FORM_IDS)
@pytest.mark.parametrize("name", wk.NAMES)
def test_whole_array_against_the_text_hip(hip, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_whole(ctx, flags, ctxs[1], hip, name, bits)


@pytest.mark.parametrize("bits", sc.FORMS, ids=sc.FORM_IDS)
@pytest.mark.parametrize("name", wk.NAMES)
def test_equal_to_locate_hip(hip, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_equals_locate(ctx, flags, ctxs[1], hip, name, bits)


@pytest.mark.parametrize("name,bits", sc.WINDOW_CASES, ids=sc.WINDOW_IDS)
def test_windows_hip(hip, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_windows(ctx, flags, ctxs[1], hip, name, bits)


@pytest.mark.parametrize("bits", (None, 6), ids=["strings", "segments_b6"])
@pytest.mark.parametrize("name", ("dna", "mixed", "wide_u64"))
def test_one_output_at_a_time_hip(hip, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_one_output(ctx, flags, ctxs[1], hip, name, bits)


@pytest.mark.parametrize("bits", (None, 6), ids=["strings", "segments_b6"])
def test_width_refusals_hip(hip, ctxs, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_width_refusals(ctx, flags, ctxs[1], hip, bits)


@pytest.mark.parametrize("bits", (None, 6), ids=["strings", "segments_b6"])
def test_other_refusals_hip(hip, ctxs, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_refusals(ctx, flags, ctxs[1], hip, bits)


def test_index_is_unchanged_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_index_unchanged(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("lanes", wk.LANES, ids=["lanes%s" % (v or "_unset") for v in wk.LANES])
@pytest.mark.parametrize("bits", (None, 2, 6), ids=["strings", "segments_b2", "segments_b6"])
@pytest.mark.parametrize("name", wk.REFILL)
def test_lanes_hip(hip, ctxs, monkeypatch, name, bits, lanes):
    """the same outputs whatever the number of lanes; lane_refills = the tickets past the first one of every lane"""
    monkeypatch.setenv("GRLBWT_QUIET_ENV", "1")
    if lanes is None:
        monkeypatch.delenv("GRLBWT_WALK_LANES", raising=False)
    else:
        monkeypatch.setenv("GRLBWT_WALK_LANES", lanes)
    for ctx, flags in zip(ctxs[0], FLAGS):
        sc.run_whole(ctx, flags, ctxs[1], hip, name, bits, lanes)


def test_foreign_images_hip(ctxs):
    done = lost = 0
    for name in wk.FOREIGN:
        for ctx in ctxs[0]:
            d, l = sc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])
            done, lost = done + d, lost + l
    assert done >= 20 and lost >= 100            # (some of these images hold rows on no string's chain: the "none" entries)
