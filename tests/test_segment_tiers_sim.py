"""CPU: the three tiers of a refinement round (counting up to GRLBWT_SEG_CAP, one stable sort per group up to
GRLBWT_SEG_LDS_CAP, two radix sorts above) over the serial stand-in of the device primitives, against the oracle.  The
stand-in runs the same classification scan and the same write-out as the device library; only the per-group sort is serial."""
import pytest

from grlbwt_amd import engine, workloads
from tests import parity
from tests.test_engine_logic_sim import _long_run_collection

# (GRLBWT_SEG_CAP, GRLBWT_SEG_LDS_CAP): all three tiers on small inputs; a middle tier of one size; everything but the giants
# in the middle tier (sizes that are no powers of two); the middle tier off (the radix branch takes every group above the cap)
TIERS = [("1", "3"), ("4", "16"), ("4", "5"), ("1", "4096"), ("4", "0")]


@pytest.fixture(scope="module")
def sim():
    from tests import simlib
    return simlib.sim_library()


@pytest.fixture(scope="module")
def inputs():
    return (workloads.sampled_reads(20000, 100, 100000, seed=11).tobytes(),
            workloads.zipf_tokens(200000, doc_len=500, vocab=20000).tobytes(),
            _long_run_collection(2000, 4, 5))


def _check(lib, inputs):
    reads, tokens, long_runs = inputs
    parity.check_stagewise(lib, reads, 1)
    parity.check_stagewise(lib, tokens, 2, engine.FLAG_FORCE_IDX64)
    parity.check_final(lib, long_runs, 1)           # run-aware keys


@pytest.mark.parametrize("cap,lds_cap", TIERS)
def test_segment_tiers(sim, oracle_mod, monkeypatch, inputs, cap, lds_cap):
    monkeypatch.setenv("GRLBWT_SEG_CAP", cap)
    monkeypatch.setenv("GRLBWT_SEG_LDS_CAP", lds_cap)
    _check(sim, inputs)


def test_segment_tiers_group_number_keys(sim, oracle_mod, monkeypatch, inputs):
    """Doubling rounds from the first round on, no run-aware keys: the tiers order group-number keys (sentinel mask 1)."""
    monkeypatch.setenv("GRLBWT_SEG_CAP", "1")
    monkeypatch.setenv("GRLBWT_SEG_LDS_CAP", "3")
    monkeypatch.setenv("GRLBWT_DOUBLING_AFTER", "0")
    monkeypatch.setenv("GRLBWT_RUN_KEYS_MIN", "0")
    _check(sim, inputs)
