"""grlbwt_fm_lcp on the serial stand-in (CPU): the cases and checkers of tests/lcp_cases.py, each on a plain context and on one
with 64-bit positions.  (The stand-in runs a pass in its generic form: the primitives alone, one row after the other.)"""
import numpy as np
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import lcp_cases as lc

FLAGS = (0, engine.FLAG_FORCE_IDX64)


@pytest.fixture(scope="module")
def sim():
    from tests import simlib
    return simlib.sim_library()


@pytest.fixture(scope="module")
def ctxs(sim):
    with engine.Context(0, FLAGS[0], sim) as a, engine.Context(0, FLAGS[1], sim) as b:
        yield (a, b), fc.Mem(False)


def test_binding_names_the_new_calls():
    assert {"grlbwt_fm_lcp", "grlbwt_fm_lcp_info_get"} <= set(engine.ABI_SYMBOLS)
    assert all(hasattr(engine.FmIndex, n) for n in ("lcp", "lcp_info", "distinct_kmers"))


def test_naive_forms_agree_on_random_collections():
    """the matrix form against the tuple sort (Expected asserts it), and the k-mer formula on the definition alone: the rows
    with an LCP below k less the suffixes of fewer than k cells are the distinct windows"""
    assert hasattr(engine.FmIndex, "lcp")
    rng = np.random.default_rng(5)
    for trial in range(40):
        strs = [rng.integers(66, 66 + int(rng.integers(1, 4)), size=int(rng.integers(0, 12))) for _ in range(int(rng.integers(1, 8)))]
        cells = lc.mc.text(strs, 10, 1)
        if trial % 3 == 0:
            cells = np.concatenate([cells, cells])
        e = lc.Expected(cells)
        for k in range(1, 8):
            assert int((e.lcp < k).sum()) - int((e.slen < k).sum()) == e.kmers(k), (trial, k)


def test_sizes_follow_the_tile(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        lc.run_sizes_follow_the_tile(ctx, flags, ctxs[1], sim)


@pytest.mark.parametrize("name", lc.NAMES)
def test_lcp_of_collections(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        info = lc.run_case(ctx, flags, ctxs[1], sim, name)
        assert info["tile_rows"] == 4096


def test_foreign_encodings(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        lc.run_foreign(ctx, flags, ctxs[1], sim)


def test_caps_and_widths(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        lc.run_caps(ctx, flags, ctxs[1], sim)


def test_outputs_are_independent(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        lc.run_outputs_are_independent(ctx, flags, ctxs[1], sim)


def test_histograms_are_sized_by_the_refusal(sim, ctxs, monkeypatch):
    for ctx, flags in zip(ctxs[0], FLAGS):
        lc.run_sizing_idiom(ctx, flags, ctxs[1], sim, monkeypatch)


def test_index_is_unchanged(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        lc.run_index_unchanged(ctx, flags, ctxs[1], sim)


def test_refusals(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        lc.run_refusals(ctx, flags, ctxs[1], sim)
