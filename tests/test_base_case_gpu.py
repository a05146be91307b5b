"""GPU (-m gpu): the base case of a whole build on the device (a level of short strings is not parsed again: its BWT comes from
sorting its suffixes with the dictionary stage's sort, every string a phrase), against the oracle.  The cases are those of
tests/test_base_case_sim.py."""
import os

import pytest

from grlbwt_amd import engine
from tests import base_case_cases as cases
from tests import suffix_rounds_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__ as g
    lib = g.build_hip()
    assert os.path.exists(lib)
    return lib


@pytest.mark.parametrize("flags", [0, engine.FLAG_FORCE_IDX64], ids=["idx32", "idx64"])
@pytest.mark.parametrize("config", cases.TIER_CONFIGS)
def test_forced_on_reads_through_every_tier(hip, oracle_mod, monkeypatch, capfd, config, flags):
    """(a)"""
    cases.check_tiers(hip, config, flags, monkeypatch, capfd)


@pytest.mark.parametrize("flags", [0, engine.FLAG_FORCE_IDX64], ids=["idx32", "idx64"])
def test_forced_on_duplicates_empty_and_one_cell_strings(hip, oracle_mod, monkeypatch, flags):
    """(b)"""
    monkeypatch.setenv(cases.RATIO, cases.FORCED)
    cases.check_forced(hip, cases.dups_and_short(), 1, flags)


@pytest.mark.parametrize("n", [2047, 2048, 2049])
def test_forced_at_the_scan_tile_edge(hip, oracle_mod, monkeypatch, n):
    """(c)"""
    monkeypatch.setenv(cases.RATIO, cases.FORCED)
    cases.check_forced(hip, cases.n_reads(n))


def test_forced_on_u16_tokens(hip, oracle_mod, monkeypatch):
    """(d)"""
    monkeypatch.setenv(cases.RATIO, cases.FORCED)
    cases.check_forced(hip, cases.tokens(), 2)


@pytest.mark.parametrize("w", [4, 8])
def test_forced_on_a_wide_alphabet(hip, oracle_mod, monkeypatch, w):
    """(d)"""
    monkeypatch.setenv(cases.RATIO, cases.FORCED)
    cases.check_forced_wide(hip, w)


def test_default_ratio_fires_at_its_natural_level(hip, oracle_mod, monkeypatch):
    """(e): nothing forced; the deepest level of the build is the base level and holds that level's cells"""
    monkeypatch.delenv(cases.RATIO, raising=False)
    rounds, deepest = cases.check_forced(hip, cases.reads())
    assert rounds >= 2 and deepest["n"] == cases.level_cells(cases.reads(), rounds)


def test_ratio_zero_runs_the_oracles_rounds(hip, oracle_mod, monkeypatch):
    """(f)"""
    monkeypatch.setenv(cases.RATIO, "0")
    assert cases.check_same_rounds(hip, cases.reads()) >= 3


@pytest.mark.parametrize("ratio", [None, "0", cases.FORCED])
def test_builds_of_fewer_than_three_rounds_are_unaffected(hip, oracle_mod, monkeypatch, ratio):
    """(g)"""
    if ratio is None:
        monkeypatch.delenv(cases.RATIO, raising=False)
    else:
        monkeypatch.setenv(cases.RATIO, ratio)
    assert cases.check_same_rounds(hip, suffix_rounds_cases.identical_strings()) < 3
