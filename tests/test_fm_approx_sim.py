"""grlbwt_fm_approx on the serial stand-in (CPU): the cases and checkers of tests/approx_cases.py, each on a plain context and on
one with 64-bit positions.  (The stand-in runs the same functor as the HIP kernel, one pattern after the other through
prim::for_each and without a top level.)"""
import pytest

from grlbwt_amd import engine
from tests import approx_cases as ac
from tests import fm_cases as fc
from tests import image_cases as ic

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
    assert {"grlbwt_fm_approx", "grlbwt_fm_approx_info_get"} <= set(engine.ABI_SYMBOLS)
    assert all(hasattr(engine.FmIndex, n) for n in ("approx", "approx_info"))


def test_pattern_set_is_not_vacuous():
    """On the brute-force values alone, for the DNA collection (144 patterns): at k = 1 at least 12 patterns with two or more hits;
    at k = 2 at least 500 hits and 6 patterns without any; at k = 3 one list of 64 or more.  Every collection has, at its largest
    k, a pattern with several hits and one with none."""
    assert hasattr(engine.FmIndex, "approx")
    ex = ac.expected("dna")
    assert len(ex.pats) == 144
    ac.not_vacuous(ex)
    for name in fc.COLLECTIONS:
        ex = ac.expected(name)
        n = [len(l) for l in ex.lists(ex.kmax, range(len(ex.pats)))]
        assert max(n) >= 3 and min(n) == 0, (name, n)


def test_order_rule_is_a_total_order_on_the_lists():
    """the sort key of the rule never ties inside a list: two distinct variants differ at some offset"""
    assert hasattr(engine.FmIndex, "approx")
    ex = ac.expected("dna")
    for q, lst in zip(ex.pats, ex.var):
        keys = [ac.order_key(q, v) for _, v in lst]
        assert len(set(keys)) == len(keys) and keys == sorted(keys)


@pytest.mark.parametrize("name", fc.COLLECTIONS)
def test_approx_against_the_text(sim, ctxs, name):
    for ctx, flags in zip(ctxs[0], FLAGS):
        ac.run_collection(ctx, flags, ctxs[1], sim, name)


@pytest.mark.parametrize("name", fc.FOREIGN)
def test_approx_on_foreign_images(ctxs, name):
    for ctx in ctxs[0]:
        ac.run_foreign(ctx, ctxs[1], ic.BY_NAME[name])


def test_launch_shapes(sim, ctxs):
    def serial(n, info):
        assert (info["walk_lanes"], info["lane_refills"]) == (n, 0)

    for ctx, flags in zip(ctxs[0], FLAGS):
        ac.run_shapes(ctx, flags, ctxs[1], sim, serial)


def test_max_hits(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        ac.run_max_hits(ctx, flags, ctxs[1], sim)


def test_refusals(sim, ctxs):
    for ctx, flags in zip(ctxs[0], FLAGS):
        ac.run_refusals(ctx, flags, ctxs[1], sim)
