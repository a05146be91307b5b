"""GPU (-m gpu): the three tiers of a refinement round -- counting up to GRLBWT_SEG_CAP, the LDS sort of one group per
workgroup up to GRLBWT_SEG_LDS_CAP, two radix sorts above -- against the oracle, with the limits lowered so that small inputs
enter every tier."""
import os

import pytest

from grlbwt_amd import engine, workloads
from tests import parity
from tests.test_engine_logic_sim import _long_run_collection

pytestmark = pytest.mark.gpu

# (GRLBWT_SEG_CAP, GRLBWT_SEG_LDS_CAP): all three tiers on small inputs; a middle tier of one size; everything but the giants
# in the middle tier (sizes that are no powers of two, both workgroup shapes); the middle tier off (the radix branch takes every
# group above the cap)
TIERS = [("1", "3"), ("4", "16"), ("4", "5"), ("1", "4096"), ("4", "0")]
TIER_SITES = ("suffix_sort.small", "suffix_sort.lds", "suffix_sort.big_groups")


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
    return (workloads.sampled_reads(20000, 100, 100000, seed=11).tobytes(),
            workloads.zipf_tokens(200000, doc_len=500, vocab=20000).tobytes(),
            _long_run_collection(2000, 4, 5))


def _site_launches(lib, data, w):
    """launches per launch site (the level tags folded) of one profiled build"""
    with engine.Context(0, 0, lib) as ctx:
        ctx.profile_enable(True)
        ctx.upload(data, w)
        ctx.build()
        prof = ctx.profile()
    sites = {}
    for name, rec in prof.items():
        site = name.split("#")[0]
        sites[site] = sites.get(site, 0) + int(rec[0])
    return sites


def _check(lib, inputs):
    reads, tokens, long_runs = inputs
    parity.check_stagewise(lib, reads, 1)
    parity.check_stagewise(lib, tokens, 2, engine.FLAG_FORCE_IDX64)
    parity.check_final(lib, long_runs, 1)           # run-aware keys


@pytest.mark.parametrize("cap,lds_cap", TIERS)
def test_segment_tiers(hip, oracle_mod, monkeypatch, inputs, cap, lds_cap):
    monkeypatch.setenv("GRLBWT_SEG_CAP", cap)
    monkeypatch.setenv("GRLBWT_SEG_LDS_CAP", lds_cap)
    _check(hip, inputs)
    if (cap, lds_cap) in (("1", "3"), ("4", "16")):
        sites = _site_launches(hip, inputs[0], 1)
        for s in TIER_SITES:                        # a tier that was never entered must not pass silently
            assert sites.get(s, 0) >= 1, (s, sorted(k for k in sites if k.startswith("suffix_sort")))


def test_segment_tiers_group_number_keys(hip, oracle_mod, monkeypatch, inputs):
    """Doubling rounds from the first round on, no run-aware keys: the LDS sort meets group-number keys (sentinel mask 1)."""
    monkeypatch.setenv("GRLBWT_SEG_CAP", "1")
    monkeypatch.setenv("GRLBWT_SEG_LDS_CAP", "3")
    monkeypatch.setenv("GRLBWT_DOUBLING_AFTER", "0")
    monkeypatch.setenv("GRLBWT_RUN_KEYS_MIN", "0")
    _check(hip, inputs)
