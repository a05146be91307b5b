"""CPU: the rows of the base case in their one-gather form and the run merge of unit rows, over the serial stand-in of the device
primitives, against the oracle (tests/base_rows_cases.py).  tests/test_base_rows_gpu.py runs the same cases on the device."""
import pytest

from grlbwt_amd import engine
from tests import base_rows_cases as rows

FLAGS = pytest.mark.parametrize("flags", [0, engine.FLAG_FORCE_IDX64], ids=["idx32", "idx64"])


@pytest.fixture(scope="module")
def sim():
    from tests import simlib
    return simlib.sim_library()


@FLAGS
@pytest.mark.parametrize("name", sorted(rows.INPUTS))
def test_forced_rows(sim, oracle_mod, monkeypatch, name, flags):
    rows.check_forced(sim, name, flags, monkeypatch)


@FLAGS
def test_first_bwt_without_lengths(sim, oracle_mod, monkeypatch, flags):
    rows.check_first_bwt(sim, flags, monkeypatch)
