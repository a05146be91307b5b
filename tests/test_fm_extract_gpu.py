"""grlbwt_fm_extract on the HIP library: the cases and checkers of tests/extract_cases.py, each on a plain context and on one with
64-bit positions; the launch shapes also under GRLBWT_WALK_LANES = 64 (one wave), 320 (five waves over two workgroups) and unset,
where lanes that finish a piece take the next ticket."""
import pytest

from grlbwt_amd import engine
from tests import extract_cases as xc
from tests import fm_cases as fc
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
    mem = fc.Mem(True)
    with engine.Context(0, FLAGS[0], hip) as a, engine.Context(0, FLAGS[1], hip) as b:
        yield (a, b), mem


@pytest.fixture(autouse=True)
def quiet(monkeypatch):
    monkeypatch.setenv("GRLBWT_QUIET_ENV", "1")
    monkeypatch.delenv("GRLBWT_WALK_LANES", raising=False)


@pytest.mark.parametrize("form", xc.FORMS, ids=xc.form_id)
def test_every_string_whole_hip(hip, ctxs, form):
    for ctx, flags in zip(ctxs[0], FLAGS):
        xc.run_whole(ctx, flags, ctxs[1], hip, *form)


@pytest.mark.parametrize("form", xc.FORMS, ids=xc.form_id)
def test_edges_around_every_sample_hip(hip, ctxs, form):
    for ctx, flags in zip(ctxs[0], FLAGS):
        xc.run_edges(ctx, flags, ctxs[1], hip, *form)


def test_mixed_without_checkpoints_hip(hip, ctxs):
    """the cost model of an index without checkpoints: a range walks from its string's END, here up to 300 000 dependent steps"""
    col = wk.COLS["mixed"]
    for ctx, flags in zip(ctxs[0], FLAGS):
        with xc.make_index(ctx, flags, ctxs[1], hip, col, None) as fm:
            Q = xc.sample_positions(fm, ctxs[1], col, None)
            xi, (pieces, skip) = xc.check(fm, ctxs[1], col, Q, xc.MIXED_HEADS, on_gpu=True)
            assert xi["n_samples"] == 5 and int(pieces.max()) == 1 and int(skip.max()) == 299999


def test_piece_accounting_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        xc.run_accounting(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("lanes", wk.LANES, ids=["lanes64", "lanes320", "default"])
@pytest.mark.parametrize("form", [("mixed", 2), ("mixed", 6), ("dna", 0), ("dna", None), ("edge_m65", 2)], ids=xc.form_id)
def test_launch_shapes_hip(hip, ctxs, monkeypatch, form, lanes):
    if lanes:
        monkeypatch.setenv("GRLBWT_WALK_LANES", lanes)
    for ctx, flags in zip(ctxs[0], FLAGS):
        infos = xc.run_shapes(ctx, flags, ctxs[1], hip, *form, lanes=lanes)
        if lanes == "64" and form[0] == "mixed":
            assert infos[-1]["lane_refills"] > 0 and infos[-2]["lane_refills"] > 0, infos[-2:]


@pytest.mark.parametrize("form", [("dna", 2), ("dna", None), ("mixed", 6)], ids=xc.form_id)
def test_round_trip_with_locate_hip(hip, ctxs, form):
    for ctx, flags in zip(ctxs[0], FLAGS):
        xc.run_round_trip(ctx, flags, ctxs[1], hip, *form)


def test_cell_widths_and_alignment_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        xc.run_widths(ctx, flags, ctxs[1], hip)


def test_refusals_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        xc.run_refusals(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("name", xc.FOREIGN)
def test_foreign_images_hip(ctxs, name):
    for ctx in ctxs[0]:
        xc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])
