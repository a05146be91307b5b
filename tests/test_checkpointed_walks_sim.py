"""The checkpointed LF walks on the serial stand-in (CPU): the cases and checkers of tests/walk_cases.py, each on a plain context
and on one with 64-bit positions.  (The stand-in runs the same begin / step / end functors as the HIP kernel, one segment after
the other through prim::for_each.)"""
import pytest

from grlbwt_amd import engine
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
    """On the recipe itself: the checkpoint counts of the edge collections, strings shorter than a block and empty ones, void picks
    (a block's pick below the number of strings) in `mixed` and `dna` at small blocks and none in the one-string collections,
    whose chain length check_info therefore pins at every checkpoint."""
    for m in wk.EDGE_M:
        col = wk.COLS["edge_m%d" % m]
        assert len(col.strings) == 1 and 1 + -(-col.n // 16) == m and col.n % 16
    assert any(len(s) == 0 for s in wk.COLS["mixed"].strings) and any(len(s) == 0 for s in wk.COLS["dna"].strings)
    assert [len(s) for s in wk.COLS["mixed"].strings] == [300000, 0, 70000, 1, 63]
    assert len(wk.FOREIGN) >= 40
    for name, bits in (("mixed", 1), ("mixed", 2), ("dna", 4), ("dna", 6)):
        col = wk.COLS[name]
        assert any(wk.pick(j, col.n, bits) < len(col.strings) for j in range(-(-col.n // (1 << bits)))), (name, bits)
    for name in ["one_long"] + ["edge_m%d" % m for m in wk.EDGE_M]:
        col = wk.COLS[name]
        for bits in (1, 2, 4, 6, 8, 10):
            assert wk.pick(0, col.n, bits) != 0, (name, bits)
    # the rule: one pick per block, inside the block, and below n
    for n, b in ((9, 4), (1000, 4), (200001, 10), (5, 20)):
        for j in range(-(-n // (1 << b))):
            assert j << b <= wk.pick(j, n, b) < min(n, (j + 1) << b)


@pytest.mark.parametrize("bits", wk.INVERT_BITS)
@pytest.mark.parametrize("name", wk.NAMES)
def test_inversion_equals_the_text(sim, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        wk.run_invert(ctx, flags, ctxs[1], sim, name, bits)


def test_one_block_heads_only(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        info = wk.run_invert(ctx, flags, ctxs[1], sim, "dna", 20)
        assert info["n_checkpoints"] == info["n_strings"] + 1


@pytest.mark.parametrize("bits", wk.INDEX_BITS)
@pytest.mark.parametrize("name", wk.NAMES)
def test_index_with_checkpoints(sim, ctxs, name, bits):
    for ctx, flags in zip(ctxs[0], FLAGS):
        wk.run_index(ctx, flags, ctxs[1], sim, name, bits)


@pytest.mark.parametrize("name", wk.FOREIGN)
def test_foreign_images_same_outcome(ctxs, name):
    for ctx in ctxs[0]:
        wk.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])


def test_refusals(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        wk.run_refusals(ctx, flags, ctxs[1], sim)


@pytest.mark.parametrize("name", ["dna", "two_bytes", "repeats"])
def test_output_at_any_alignment(sim, ctxs, name):
    """u8 / u16 cells go out as aligned 8-byte words where the text is 8-byte aligned, cell by cell elsewhere: every offset of the
    output inside a word gives the text, and nothing in front of it or behind it is written"""
    col = wk.COLS[name]
    blob = fc.image_of(sim, col, 0)
    mem = ctxs[1]
    keep, img = mem.put(blob)
    for shift in (0, 1, 2, 3, 4, 7):
        at = shift * col.w
        out, pout = mem.out(at + col.n * col.w)
        n, info = ctxs[0][0].invert_image_checkpointed(img, len(blob), col.w, pout + at, col.n, sample_bits=3)
        got = mem.body(out, at + col.n * col.w)
        assert n == col.n and got[at:].tobytes() == col.data.tobytes(), (name, shift)
        assert bool((got[:at] == fc.FILL).all()), (name, shift)
