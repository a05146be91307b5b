"""GPU (-m gpu): the rows of the base case in their one-gather form and the run merge of unit rows on the device, against the oracle.
The cases are those of tests/test_base_rows_sim.py (tests/base_rows_cases.py)."""
import os

import pytest

from grlbwt_amd import engine
from tests import base_rows_cases as rows

pytestmark = pytest.mark.gpu

FLAGS = pytest.mark.parametrize("flags", [0, engine.FLAG_FORCE_IDX64], ids=["idx32", "idx64"])


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__ as g
    lib = g.build_hip()
    assert os.path.exists(lib)
    return lib


@FLAGS
@pytest.mark.parametrize("name", sorted(rows.INPUTS))
def test_forced_rows(hip, oracle_mod, monkeypatch, name, flags):
    rows.check_forced(hip, name, flags, monkeypatch)


@FLAGS
def test_first_bwt_without_lengths(hip, oracle_mod, monkeypatch, flags):
    rows.check_first_bwt(hip, flags, monkeypatch)
