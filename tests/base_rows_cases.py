"""What tests/test_base_rows_sim.py and tests/test_base_rows_gpu.py share: the rows of the base case (Engine::base_bwt) in their
one-gather form -- front[t] = the cell in front of the suffix in slot t, whose bit 0 says "the suffix is a whole string" and whose
upper bits are the row's symbol -- and the run merge without a length array (merge_unit_runs), which Engine::first_bwt takes too.

Every forced case sets GRLBWT_BASE_CASE_RATIO to base_case_cases.FORCED and goes through base_case_cases.check_forced: the image
is the oracle's and the base case fired (at level 2 for each of these inputs).

* one string and two strings: the slot whose position is 0 has no cell in front of it; it is the first, the last and (one string)
  the only whole-string row;
* 20 distinct reads x 4000 copies (8,080,000 bytes; 788,000 rows merging into 80,164 runs) and 300 x 300 (9,090,000 bytes;
  873,600 rows, 94,855 runs): equal whole strings in their thousands, so the m-th whole-string row in sorted order takes the last
  cell of string m in text order under ties that only the text position breaks, and runs of equal rows longer than the
  2048-element scan tile, so the merge of unit rows carries a run across tile edges."""
import functools

import numpy as np

from grlbwt_amd import workloads
from tests import base_case_cases as cases


@functools.lru_cache(maxsize=None)
def few_strings(n):
    """n = 1 (seed 5: 101 bytes, 2 rows at the base level) or 2 (seed 6: 3 rows)"""
    return workloads.sampled_reads(n, 100, 5000, seed=4 + n).tobytes()


@functools.lru_cache(maxsize=None)
def copies(distinct, times, seed):
    """`distinct` reads of 100 cells, the block of them `times` times over"""
    block = workloads.sampled_reads(distinct, 100, 3000, seed=seed).reshape(distinct, 101)
    return np.tile(block, (times, 1)).tobytes()


# name -> the collection's bytes
INPUTS = {
    "one_string": lambda: few_strings(1),
    "two_strings": lambda: few_strings(2),
    "20x4000": lambda: copies(20, 4000, 22),
    "300x300": lambda: copies(300, 300, 21),
}


def check_forced(lib, name, flags, monkeypatch):
    monkeypatch.setenv(cases.RATIO, cases.FORCED)
    rounds, deepest = cases.check_forced(lib, INPUTS[name](), 1, flags)
    assert rounds == 2, rounds
    return deepest


def check_first_bwt(lib, flags, monkeypatch):
    """no base case: Engine::first_bwt makes the deepest level's runs (one cell per string) through the same merge of unit rows"""
    monkeypatch.setenv(cases.RATIO, "0")
    assert cases.check_same_rounds(lib, cases.reads(), 1, flags) >= 3
