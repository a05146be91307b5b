"""The checkpointed LF walks on the HIP library: the cases and checkers of tests/walk_cases.py, each on a plain context and on
one with 64-bit positions; the inversion also under GRLBWT_WALK_LANES = 64 (one wave), 320 (five waves over two workgroups, the
second partly filled) and unset, where lanes that finish a segment take the next ticket."""
import pytest

from grlbwt_amd import engine
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


@pytest.mark.parametrize("bits", wk.INVERT_BITS)
@pytest.mark.parametrize("name", wk.NAMES)
def test_inversion_equals_the_text_hip(hip, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        wk.run_invert(ctx, flags, ctxs[1], hip, name, bits)


def test_one_block_heads_only_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        info = wk.run_invert(ctx, flags, ctxs[1], hip, "dna", 20)
        assert info["n_checkpoints"] == info["n_strings"] + 1


@pytest.mark.parametrize("lanes", wk.LANES, ids=["lanes64", "lanes320", "default"])
@pytest.mark.parametrize("name", wk.REFILL)
def test_lane_refill_hip(hip, ctxs, monkeypatch, name, lanes):
    if lanes:
        monkeypatch.setenv("GRLBWT_WALK_LANES", lanes)
    for ctx, flags in zip(ctxs[0], FLAGS):
        for bits in wk.INVERT_BITS:
            info = wk.run_invert(ctx, flags, ctxs[1], hip, name, bits, lanes)
            if lanes and name == "mixed":
                assert info["lane_refills"] > 0, (bits, info)


@pytest.mark.parametrize("bits", wk.INDEX_BITS)
@pytest.mark.parametrize("name", wk.NAMES)
def test_index_with_checkpoints_hip(hip, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        wk.run_index(ctx, flags, ctxs[1], hip, name, bits)


@pytest.mark.parametrize("name", wk.FOREIGN)
def test_foreign_images_same_outcome_hip(ctxs, name):
    for ctx in ctxs[0]:
        wk.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])


def test_refusals_hip(hip, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        wk.run_refusals(ctx, flags, ctxs[1], hip)


@pytest.mark.parametrize("name", ["dna", "two_bytes", "repeats"])
def test_output_at_any_alignment_hip(hip, ctxs, name):
    """u8 / u16 cells go out as aligned 8-byte words where the text is 8-byte aligned, cell by cell elsewhere: every offset of the
    output inside a word gives the text, and nothing in front of it or behind it is written"""
    col = wk.COLS[name]
    blob = fc.image_of(hip, col, 0)
    mem = ctxs[1]
    keep, img = mem.put(blob)
    for shift in (0, 1, 2, 3, 4, 7):
        at = shift * col.w
        out, pout = mem.out(at + col.n * col.w)
        n, info = ctxs[0][0].invert_image_checkpointed(img, len(blob), col.w, pout + at, col.n, sample_bits=3)
        got = mem.body(out, at + col.n * col.w)
        assert n == col.n and got[at:].tobytes() == col.data.tobytes(), (name, shift)
        assert bool((got[:at] == fc.FILL).all()), (name, shift)
