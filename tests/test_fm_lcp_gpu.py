"""grlbwt_fm_lcp on the HIP library: the cases and checkers of tests/lcp_cases.py, each on a plain context and on one with 64-bit
positions, with the fused pass kernel (prim::LcpRound, the default); and the two forms of a pass -- the fused kernel and, with
GRLBWT_LCP_ROUND=plain, the generic primitives -- held to byte-identical outputs."""
import numpy as np
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import lcp_cases as lc

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
def fused(monkeypatch):
    monkeypatch.setenv("GRLBWT_QUIET_ENV", "1")
    monkeypatch.delenv("GRLBWT_LCP_ROUND", raising=False)


def test_sizes_follow_the_tile_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        lc.run_sizes_follow_the_tile(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("name", lc.NAMES)
def test_lcp_of_collections_hip(hip, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        lc.run_case(ctx, flags, ctxs[1], hip, name)


def test_foreign_encodings_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        lc.run_foreign(ctx, flags, ctxs[1], hip)


def test_caps_and_widths_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        lc.run_caps(ctx, flags, ctxs[1], hip)


def test_outputs_are_independent_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        lc.run_outputs_are_independent(ctx, flags, ctxs[1], hip)


def test_histograms_are_sized_by_the_refusal_hip(hip, ctxs, monkeypatch):
    for ctx, flags in zip(ctxs[0], FLAGS):
        lc.run_sizing_idiom(ctx, flags, ctxs[1], hip, monkeypatch)


def test_index_is_unchanged_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        lc.run_index_unchanged(ctx, flags, ctxs[1], hip)


def test_refusals_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        lc.run_refusals(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("name", lc.PLAIN_NAMES)
def test_plain_form_gives_the_same_bytes_hip(hip, ctxs, monkeypatch, name):
    """GRLBWT_LCP_ROUND=plain: the values, both histograms and the counters of the fused form, uncapped and capped; and the
    expected values themselves"""
    mem = ctxs[1]
    for ctx, flags in zip(ctxs[0], FLAGS):
        c = lc.cases(lc.tile_rows(ctx, mem, hip, flags))[name]
        blob = lc.image(hip, flags, c)
        keep, img = mem.put(blob)
        with engine.FmIndex(ctx, img, len(blob)) as fm:
            for cap, w in ((0, 4), (7, 1), (0, 8)):
                monkeypatch.delenv("GRLBWT_LCP_ROUND", raising=False)
                a = lc.lcp(fm, mem, c.n, cap, w)
                monkeypatch.setenv("GRLBWT_LCP_ROUND", "plain")
                b = lc.lcp(fm, mem, c.n, cap, w)
                lc.check(c.exp, *b, cap, w)
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
                assert a[3] == b[3], (a[3], b[3])
