"""grlbwt_fm_* on the HIP library: the cases and checkers of tests/fm_cases.py, each on a plain context and on one with
64-bit positions, and each under GRLBWT_FM_TOP_BITS = 0 (every level of a search from HBM), 2 (a top level of four keys:
the indexes of a hundred runs and more have many keys per stride) and the default (these small indexes sit in LDS whole)."""
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic

pytestmark = pytest.mark.gpu
FLAGS = (0, engine.FLAG_FORCE_IDX64)
TOP_BITS = ["0", "2", None]
TOP_IDS = ["top0", "top2", "default"]


@pytest.fixture(scope="module")
def hip():
    import __graft_entry__ as g
    return g.build_hip()


@pytest.fixture(scope="module")
def ctxs(hip):
    mem = fc.Mem(True)
    with engine.Context(0, FLAGS[0], hip) as a, engine.Context(0, FLAGS[1], hip) as b:
        yield (a, b), mem


@pytest.fixture(params=TOP_BITS, ids=TOP_IDS)
def top_bits(request, monkeypatch):
    monkeypatch.setenv("GRLBWT_QUIET_ENV", "1")
    if request.param is None:
        monkeypatch.delenv("GRLBWT_FM_TOP_BITS", raising=False)
    else:
        monkeypatch.setenv("GRLBWT_FM_TOP_BITS", request.param)
    return request.param


@pytest.mark.parametrize("name", fc.FOREIGN)
def test_count_on_foreign_images_hip(ctxs, top_bits, name):
    for ctx in ctxs[0]:
        fc.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])


@pytest.mark.parametrize("name", fc.COLLECTIONS)
def test_count_and_locate_against_the_text_hip(hip, ctxs, top_bits, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        fc.run_collection(ctx, flags, ctxs[1], hip, name)


def test_top_level_follows_the_switch(hip, ctxs, top_bits):
    """the three settings are three shapes of the search: none, four keys over many, the whole array"""
    col = fc.COLS["dna"]
    blob = fc.image_of(hip, col, 0)
    keep, img = ctxs[1].put(blob)
    for ctx in ctxs[0]:
        with engine.FmIndex(ctx, img, len(blob)) as fm:
            info = fm.info()
            assert info["n_runs"] > 100
            if top_bits == "0":
                assert info["top_entries"] == 0
            elif top_bits == "2":
                assert info["top_entries"] == 4
            else:
                assert info["top_entries"] >= 256


def test_launch_shapes_hip(hip, ctxs, top_bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        fc.run_shapes(ctx, flags, ctxs[1], hip)


def test_refusals_hip(hip, ctxs, top_bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        fc.run_refusals(ctx, flags, ctxs[1], hip)
