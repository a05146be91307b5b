"""grlbwt_fm_extract on the serial stand-in (CPU): the cases and checkers of tests/extract_cases.py, each on a plain context and on
one with 64-bit positions.  (The stand-in runs the same begin / step / end functor as the HIP kernel, one piece after the other.)"""
import numpy as np
import pytest

from grlbwt_amd import engine
from tests import extract_cases as xc
from tests import fm_cases as fc
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
        yield (a, b), fc.Mem(False)


def test_the_cases_reach_what_they_are_for():
    """On the recipe itself: empty strings, a string of one cell, the large collections only with checkpoints (but `mixed`, with
    at most 16 ranges), launch shapes with empty, short and long ranges and ranges that start behind their string."""
    assert [len(s) for s in wk.COLS["mixed"].strings] == [300000, 0, 70000, 1, 63]
    assert any(len(s) == 0 for s in wk.COLS["dna"].strings)
    assert set(xc.SMALL) == set(wk.NAMES) - {"one_long", "mixed", "repeats"} and all(wk.COLS[n].n < 5000 for n in xc.SMALL if n != "dna")
    assert len(xc.MIXED_HEADS) <= 16 and len(xc.FOREIGN) >= 40
    r = xc.shape_ranges(wk.COLS["mixed"], 5000, 6000).astype(np.int64)
    ln = xc.slens(wk.COLS["mixed"])[r[:, 0]]
    size = r[:, 2] - r[:, 1]
    assert (size == 0).any() and (size > 400).any() and (r[:, 1] >= ln).any() and (r[:, 2] > ln).any() and len(set(r[:, 0].tolist())) == 5


@pytest.mark.parametrize("form", xc.FORMS, ids=xc.form_id)
def test_every_string_whole(sim, ctxs, form):
    for ctx, flags in zip(ctxs[0], FLAGS):
        xc.run_whole(ctx, flags, ctxs[1], sim, *form)


@pytest.mark.parametrize("form", xc.FORMS, ids=xc.form_id)
def test_edges_around_every_sample(sim, ctxs, form):
    for ctx, flags in zip(ctxs[0], FLAGS):
        xc.run_edges(ctx, flags, ctxs[1], sim, *form)


def test_mixed_without_checkpoints(sim, ctxs):
    """the cost model of an index without checkpoints: a range walks from its string's END, here up to 300 000 dependent steps"""
    col = wk.COLS["mixed"]
    for ctx, flags in zip(ctxs[0], FLAGS):
        with xc.make_index(ctx, flags, ctxs[1], sim, col, None) as fm:
            Q = xc.sample_positions(fm, ctxs[1], col, None)
            xi, (pieces, skip) = xc.check(fm, ctxs[1], col, Q, xc.MIXED_HEADS)
            assert xi["n_samples"] == 5 and int(pieces.max()) == 1 and int(skip.max()) == 299999


def test_piece_accounting(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        xc.run_accounting(ctx, flags, ctxs[1], sim)


@pytest.mark.parametrize("form", [("mixed", 2), ("mixed", 6), ("dna", 0), ("dna", None), ("edge_m65", 2)], ids=xc.form_id)
def test_launch_shapes(sim, ctxs, form):
    for ctx, flags in zip(ctxs[0], FLAGS):
        xc.run_shapes(ctx, flags, ctxs[1], sim, *form)


@pytest.mark.parametrize("form", [("dna", 2), ("dna", None), ("mixed", 6)], ids=xc.form_id)
def test_round_trip_with_locate(sim, ctxs, form):
    for ctx, flags in zip(ctxs[0], FLAGS):
        xc.run_round_trip(ctx, flags, ctxs[1], sim, *form, cap=1024)


def test_cell_widths_and_alignment(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        xc.run_widths(ctx, flags, ctxs[1], sim)


def test_refusals(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        xc.run_refusals(ctx, flags, ctxs[1], sim)


@pytest.mark.parametrize("name", xc.FOREIGN)
def test_foreign_images(ctxs, name):
    for ctx in ctxs[0]:
        xc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])
