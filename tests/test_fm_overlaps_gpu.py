"""grlbwt_fm_overlaps / grlbwt_fm_overlaps_of / grlbwt_fm_overlap_targets on the HIP library: the cases and checkers of
tests/overlap_cases.py, each on a plain context and on one with 64-bit positions.  The collections, the launch shapes and the
refusals run under GRLBWT_FM_TOP_BITS = 0 (every level of a search from HBM), 2 (a top level of four keys) and the default (these
small indexes sit in LDS whole), each as lanes that take tickets (prim::top_tickets, the default) and as one lane per query
(GRLBWT_FM_MATCH=l, prim::top_search); the foreign images under the default and under four keys with one lane per query.  Every
setting is held to the same expected values, so all give equal outputs."""
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import overlap_cases as oc

pytestmark = pytest.mark.gpu
FLAGS = (0, engine.FLAG_FORCE_IDX64)
SETTINGS = [(top, form) for top in ("0", "2", None) for form in (None, "l")]
IDS = ["top%s-%s" % (top or "default", "lanes" if form else "tickets") for top, form in SETTINGS]


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as g
    return g.build_hip()


@pytest.fixture(scope="module")
def ctxs(hip):
    mem = fc.Mem(True)
    with engine.Context(0, FLAGS[0], hip) as a, engine.Context(0, FLAGS[1], hip) as b:
        yield (a, b), mem


def set_env(monkeypatch, top, form, lanes=None):
    monkeypatch.setenv("GRLBWT_QUIET_ENV", "1")
    for name, value in (("GRLBWT_FM_TOP_BITS", top), ("GRLBWT_FM_MATCH", form), ("GRLBWT_WALK_LANES", lanes)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


@pytest.fixture(params=SETTINGS, ids=IDS)
def setting(request, monkeypatch):
    set_env(monkeypatch, *request.param)
    return request.param


@pytest.mark.parametrize("name", oc.NAMES)
def test_overlaps_against_the_text_hip(hip, ctxs, setting, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        oc.run_collection(ctx, flags, ctxs[1], hip, name)


def test_targets_around_the_tile_boundaries_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        oc.run_tile_ranges(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("top,form", [(None, None), ("2", "l")], ids=["default-tickets", "top2-lanes"])
def test_overlaps_on_foreign_images_hip(ctxs, monkeypatch, top, form):
    set_env(monkeypatch, top, form)
    hits = 0
    for name in fc.FOREIGN:
        for ctx in ctxs[0]:
            hits += oc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])
    assert hits >= 50


def test_launch_shapes_hip(hip, ctxs, setting):
    """unset, no lane takes a second ticket: there are never fewer lanes than queries rounded up to a wave"""
    top, form = setting

    def launch(n, info):
        assert info["lane_refills"] == 0
        assert info["walk_lanes"] == (n if form else (n + 63) // 64 * 64)

    for ctx, flags in zip(ctxs[0], FLAGS):
        oc.run_shapes(ctx, flags, ctxs[1], hip, launch)


@pytest.mark.parametrize("top", ["0", None], ids=["top0", "default"])
def test_one_wave_takes_every_ticket_hip(hip, ctxs, monkeypatch, top):
    """GRLBWT_WALK_LANES=64: one wave works through every batch, 5000 queries included, by refilling its lanes"""
    set_env(monkeypatch, top, None, "64")
    seen = {}

    def launch(n, info):
        assert info["walk_lanes"] == (64 if n else 0)
        assert info["lane_refills"] == max(n - 64, 0), (n, info)
        seen[n] = info["lane_refills"]

    for ctx, flags in zip(ctxs[0], FLAGS):
        oc.run_shapes(ctx, flags, ctxs[1], hip, launch)
    assert seen[5000] == 5000 - 64


def test_refusals_hip(hip, ctxs, setting):
    for ctx, flags in zip(ctxs[0], FLAGS):
        oc.run_refusals(ctx, flags, ctxs[1], hip)
