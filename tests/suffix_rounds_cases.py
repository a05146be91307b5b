"""What tests/test_suffix_rounds_sim.py and tests/test_suffix_rounds_gpu.py share: the refinement rounds of the dictionary's
suffix sort, whose scans hand their prefixes straight to the consumers (unresolved slots, group heads of a round, the closing
of the groups), against the oracle.  The same cases run over the serial stand-in and over the device library."""
import re

import numpy as np

from grlbwt_amd import engine, workloads
from tests import parity
from tests.test_engine_logic_sim import _long_run_collection

# environment of a case: the default limits; every tier on small inputs; no LDS tier; doubling rounds with group-number keys
CONFIGS = {
    "default": {},
    "cap1_lds3": {"GRLBWT_SEG_CAP": "1", "GRLBWT_SEG_LDS_CAP": "3"},
    "cap4_lds0": {"GRLBWT_SEG_CAP": "4", "GRLBWT_SEG_LDS_CAP": "0"},
    "doubling": {"GRLBWT_DOUBLING_AFTER": "0", "GRLBWT_RUN_KEYS_MIN": "0"},
}
INPUTS = ("reads", "tokens", "long_runs")


def small_inputs():
    """the small inputs of tests/test_gpu_segment_tiers.py"""
    return {"reads": workloads.sampled_reads(20000, 100, 100000, seed=11).tobytes(),
            "tokens": workloads.zipf_tokens(200000, doc_len=500, vocab=20000).tobytes(),
            "long_runs": _long_run_collection(2000, 4, 5)}


def check_small(lib, inputs, which):
    if which == "reads":
        parity.check_stagewise(lib, inputs["reads"], 1)
    elif which == "tokens":
        parity.check_stagewise(lib, inputs["tokens"], 2, engine.FLAG_FORCE_IDX64)
    else:
        parity.check_final(lib, inputs["long_runs"], 1)          # run-aware keys


def _dna(rng, n):
    return bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))


def resolved_at_once():
    """strings shorter than a first-pass key (16 symbols of DNA): the first sort leaves no unresolved suffix"""
    rng = np.random.default_rng(5)
    return b"".join(_dna(rng, int(rng.integers(1, 12))) + b"\n" for _ in range(300))


def identical_strings():
    """twenty times the same run of one symbol, shorter than the run-aware keys' threshold: after the first sort one group holds
    every suffix longer than a key, and every round takes one key's worth of symbols off it, to the end of the phrase"""
    return (b"A" * 400 + b"\n") * 20


def mixed_rounds():
    """sampled reads: with GRLBWT_SEG_CAP=4 the early rounds of a level hold groups above the cap, the late ones do not"""
    return workloads.sampled_reads(2000, 100, 20000, seed=7).tobytes()


def sort_iters(lib, data, cell_bytes=1):
    """refinement rounds (+1) of every level of one build"""
    out = []
    with engine.Context(0, 0, lib) as ctx:
        ctx.upload(data, cell_bytes)
        while True:
            info, done = ctx.parse_round()
            out.append(int(info["sort_iters"]))
            if done:
                break
    return out


_ROUND = re.compile(r"\[grlbwt\] level (-?\d+) refinement round: (\d+) items in (\d+) groups; (.*)")


def traced_rounds(lib, data, capfd, cell_bytes=1):
    """(level, items, groups, the tiers behind the counting tier ran) of every refinement round of one build, in order, from
    the library's trace (GRLBWT_TABLE_TRACE must be set by the caller); the image is checked against the oracle"""
    capfd.readouterr()
    parity.check_final(lib, data, cell_bytes)
    err = capfd.readouterr().err
    return [(int(m.group(1)), int(m.group(2)), int(m.group(3)), not m.group(4).startswith("counting all"))
            for m in map(_ROUND.match, err.splitlines()) if m]
