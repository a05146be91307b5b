"""GPU (-m gpu): the refinement rounds of the dictionary's suffix sort on the device, against the oracle.  The scans of a round
hand their prefixes to the consumers in two phases (total first, then the per-tile scan with the consumer): no prefix array of
the unresolved slots, of a round's group heads or of the final groups is stored, and the passes that read them are gone."""
import os

import pytest

from grlbwt_amd import engine
from tests import parity
from tests import suffix_rounds_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__ as g
    lib = g.build_hip()
    assert os.path.exists(lib)
    return lib


@pytest.fixture(scope="module")
def inputs():
    return cases.small_inputs()


@pytest.mark.parametrize("which", cases.INPUTS)
@pytest.mark.parametrize("config", sorted(cases.CONFIGS))
def test_small_inputs(hip, oracle_mod, monkeypatch, inputs, config, which):
    for k, v in cases.CONFIGS[config].items():
        monkeypatch.setenv(k, v)
    cases.check_small(hip, inputs, which)


def test_first_sort_resolves_everything(hip, oracle_mod):
    """no unresolved slot after the first sort: the total of the first round's scan is zero, nothing is emitted"""
    data = cases.resolved_at_once()
    assert set(cases.sort_iters(hip, data)) == {1}
    parity.check_stagewise(hip, data, 1)


def test_one_string_of_one_symbol(hip, oracle_mod):
    parity.check_stagewise(hip, b"A\n", 1)


def test_identical_strings_refine_to_the_end(hip, oracle_mod, monkeypatch, capfd):
    """One group of 392 suffixes, 9 fewer per round.  Default limits: the 37 rounds with more than 64 items run the tiers behind
    the counting tier (they launch suffix_sort.big_scan), the last 7 (59 items down to 5) do not."""
    monkeypatch.setenv("GRLBWT_TABLE_TRACE", "1")
    rounds = cases.traced_rounds(hip, cases.identical_strings(), capfd)
    assert [r[1] for r in rounds] == list(range(392, 0, -9)) and all(r[2] == 1 for r in rounds)
    assert [r[3] for r in rounds] == [True] * 37 + [False] * 7


def _sites(lib, data, w=1):
    """launches per launch site and level of one profiled build"""
    with engine.Context(0, 0, lib) as ctx:
        ctx.profile_enable(True)
        ctx.upload(data, w)
        ctx.build()
        prof = ctx.profile()
    return {name: int(rec[0]) for name, rec in prof.items()}


def test_rounds_with_and_without_a_group_above_the_cap(hip, oracle_mod, monkeypatch, capfd):
    """GRLBWT_SEG_CAP=4 on 2000 sampled reads, four refinement rounds in one build: the round of level 0 and the second round
    of level 2 have no group of more than 4 suffixes and end behind the counting tier; the round of level 1 and the first round
    of level 2 launch suffix_sort.big_scan (one tile each: one launch) and the LDS tier."""
    monkeypatch.setenv("GRLBWT_SEG_CAP", "4")
    data = cases.mixed_rounds()
    sites = _sites(hip, data)
    monkeypatch.setenv("GRLBWT_TABLE_TRACE", "1")
    rounds = cases.traced_rounds(hip, data, capfd)
    assert [(r[0], r[3]) for r in rounds] == [(0, False), (1, True), (2, True), (2, False)], rounds
    assert all(r[1] <= 2048 for r in rounds)
    got = {lvl: (sites.get("suffix_sort.small#p%d" % lvl, 0), sites.get("suffix_sort.big_scan#p%d" % lvl, 0)) for lvl in range(3)}
    assert got == {0: (1, 0), 1: (1, 1), 2: (2, 1)}, sorted(k for k in sites if k.startswith("suffix_"))


def test_old_passes_are_not_launched(hip, inputs):
    """A profiled build of the reads: the passes that read the stored prefix arrays back (suffix_gstart, suffix_gid) are gone,
    and the sites that took their work over are there."""
    sites = {}
    for name, n in _sites(hip, inputs["reads"]).items():
        sites[name.split("#")[0]] = sites.get(name.split("#")[0], 0) + n
    assert sites.get("suffix_gstart", 0) == 0 and sites.get("suffix_gid", 0) == 0, sorted(k for k in sites if k.startswith("suffix_"))
    for s in ("suffix_unresolved_scan", "suffix_heads", "suffix_keys", "suffix_sort.small"):
        assert sites.get(s, 0) >= 1, (s, sorted(k for k in sites if k.startswith("suffix_")))


def test_selftest_split_scan_boundaries(hip):
    """grlbwt_selftest at a small n: its split-scan check runs at the edges of a scan tile and of the second level of tile sums
    whatever n is"""
    with engine.Context(0, 0, hip) as ctx:
        assert ctx.selftest(3000, 7) == 0
