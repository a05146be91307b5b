"""CPU: the refinement rounds of the dictionary's suffix sort over the serial stand-in of the device primitives, against the
oracle.  The scans of a round hand their prefixes to the consumers (the unresolved slots compacted, the group heads of the
round, the closing of the groups) in two phases, total first; the stand-in runs the same consumers serially."""
import pytest

from grlbwt_amd import engine
from tests import parity
from tests import suffix_rounds_cases as cases


@pytest.fixture(scope="module")
def sim():
    from tests import simlib
    return simlib.sim_library()


@pytest.fixture(scope="module")
def inputs():
    return cases.small_inputs()


@pytest.mark.parametrize("which", cases.INPUTS)
@pytest.mark.parametrize("config", sorted(cases.CONFIGS))
def test_small_inputs(sim, oracle_mod, monkeypatch, inputs, config, which):
    for k, v in cases.CONFIGS[config].items():
        monkeypatch.setenv(k, v)
    cases.check_small(sim, inputs, which)


def test_first_sort_resolves_everything(sim, oracle_mod):
    """no unresolved slot after the first sort: the total of the first round's scan is zero, nothing is emitted"""
    data = cases.resolved_at_once()
    assert set(cases.sort_iters(sim, data)) == {1}
    parity.check_stagewise(sim, data, 1)


def test_one_string_of_one_symbol(sim, oracle_mod):
    parity.check_stagewise(sim, b"A\n", 1)


def test_identical_strings_refine_to_the_end(sim, oracle_mod, monkeypatch, capfd):
    """One group of 392 suffixes, 9 fewer per round.  Default limits: the 37 rounds with more than 64 items run the tiers behind
    the counting tier (they launch suffix_sort.big_scan), the last 7 (59 items down to 5) do not."""
    monkeypatch.setenv("GRLBWT_TABLE_TRACE", "1")
    rounds = cases.traced_rounds(sim, cases.identical_strings(), capfd)
    assert [r[1] for r in rounds] == list(range(392, 0, -9)) and all(r[2] == 1 for r in rounds)
    assert [r[3] for r in rounds] == [True] * 37 + [False] * 7


def test_rounds_with_and_without_a_group_above_the_cap(sim, oracle_mod, monkeypatch, capfd):
    """GRLBWT_SEG_CAP=4 on 2000 sampled reads, four refinement rounds in one build: the round of level 0 and the second round
    of level 2 have no group of more than 4 suffixes and end behind the counting tier; the round of level 1 and the first round
    of level 2 launch suffix_sort.big_scan and the LDS tier."""
    monkeypatch.setenv("GRLBWT_SEG_CAP", "4")
    monkeypatch.setenv("GRLBWT_TABLE_TRACE", "1")
    rounds = cases.traced_rounds(sim, cases.mixed_rounds(), capfd)
    assert [(r[0], r[3]) for r in rounds] == [(0, False), (1, True), (2, True), (2, False)], rounds


def test_selftest_split_scan_boundaries(sim):
    """grlbwt_selftest at a small n: its split-scan check runs at the edges of a scan tile and of the second level of tile sums
    whatever n is"""
    with engine.Context(0, 0, sim) as ctx:
        assert ctx.selftest(3000, 7) == 0
