"""What tests/test_base_case_sim.py and tests/test_base_case_gpu.py share: a whole build (grlbwt_build) that stops parsing at a
level of short strings and writes that level's BWT down by sorting its suffixes (Engine::base_bwt, GRLBWT_BASE_CASE_RATIO),
against the oracle.  The same cases run over the serial stand-in and over the device library.

Every case compares the final image with the oracle's, as parity.check_final does (for symbols of 2^30 and more: the oracle on the
rank text, tests/wide_check.py).  A case that forces the base case also asserts that it fired: the oracle needs at least three
rounds and the engine, after build(), answers fewer round_info indices than that."""
import functools
import re

import numpy as np

from grlbwt_amd import engine, workloads
from oracle import oracle
from tests import parity
from tests import suffix_rounds_cases
from tests import wide_check as wc

RATIO = "GRLBWT_BASE_CASE_RATIO"
FORCED = str(1 << 40)          # any level from the second on is a base case (its longest string permitting)
# the limits of the refinement's tiers, as tests/suffix_rounds_cases.py sets them: counting; LDS and radix; counting and radix
TIER_CONFIGS = ("default", "cap1_lds3", "cap4_lds0")


@functools.lru_cache(maxsize=None)
def reads():
    """the reads of tests/suffix_rounds_cases.py: 20x coverage, so suffixes tie down to the string ends"""
    return workloads.sampled_reads(20000, 100, 100000, seed=11).tobytes()


@functools.lru_cache(maxsize=None)
def dups_and_short():
    """whole strings many times over, empty strings, one-cell strings (the `dups` pool of tests/parity.py) and short random DNA:
    the whole-string rows and the ties that only the text position breaks"""
    rng = np.random.default_rng(20260011)
    pool = [b"ACGT\n", b"A\n", b"\n", b"ACGTACGT\n", b"TTTT\n", b"GATTACA\n"]
    parts = []
    for _ in range(4000):
        if rng.random() < 0.6:
            parts.append(pool[int(rng.integers(0, len(pool)))])
        else:
            parts.append(bytes(rng.choice(list(b"ACGT"), size=int(rng.integers(0, 60))).astype(np.uint8)) + b"\n")
    return b"".join(parts)


@functools.lru_cache(maxsize=None)
def n_reads(n):
    """n strings: 2047, 2048 and 2049 lie around the edge of a scan tile (the scan over the slots that hold a string start)"""
    return workloads.sampled_reads(n, 100, 5000, seed=13).tobytes()


@functools.lru_cache(maxsize=None)
def tokens():
    return workloads.zipf_tokens(200000, doc_len=500, vocab=20000).tobytes()


@functools.lru_cache(maxsize=None)
def wide(w):
    """strings over few values of 2^30 and more (the build runs on their ranks), repeated and empty ones among them"""
    lo, hi = (2 ** 31, 2 ** 32 - 1) if w == 4 else (2 ** 40, 2 ** 64 - 5)
    return wc.collection(np.random.default_rng([20260012, w]), w, 600, 80, 9, lo, hi)


@functools.lru_cache(maxsize=None)
def expected(data, cell_bytes=1):
    """(image, rounds) of the oracle, computed once per input"""
    o = oracle.OracleResult(data, cell_bytes)
    out = (o.rl_bwt, int(o.n_rounds))
    o.close()
    return out


def build(lib, data, cell_bytes=1, flags=0):
    """(image, valid round_info indices, level_info of the deepest level) of one grlbwt_build"""
    with engine.Context(0, flags, lib) as ctx:
        ctx.upload(data, cell_bytes)
        ctx.build()
        blob = ctx.result_bytes()
        rounds = 0
        while True:
            try:
                ctx.round_info(rounds)
            except engine.GrlbwtError:
                break
            rounds += 1
        return blob, rounds, ctx.level_info(rounds)


def check_forced(lib, data, cell_bytes=1, flags=0):
    """the image is the oracle's, and the base case fired: fewer rounds than the oracle's three or more"""
    exp, o_rounds = expected(data, cell_bytes)
    got, rounds, deepest = build(lib, data, cell_bytes, flags)
    assert got == exp, "rl_bwt differs (%d vs %d bytes)" % (len(got), len(exp))
    assert o_rounds >= 3 and rounds < o_rounds, (rounds, o_rounds)
    return rounds, deepest


def check_same_rounds(lib, data, cell_bytes=1, flags=0):
    """the image is the oracle's and the build ran the oracle's rounds"""
    exp, o_rounds = expected(data, cell_bytes)
    got, rounds, _ = build(lib, data, cell_bytes, flags)
    assert got == exp, "rl_bwt differs (%d vs %d bytes)" % (len(got), len(exp))
    assert rounds == o_rounds, (rounds, o_rounds)
    return rounds


def check_forced_wide(lib, w, flags=0):
    cells = wide(w)
    _, inv = wc.ranks_of(cells)
    o_rounds = expected(inv.tobytes(), 8)[1]
    exp = wc.oracle_on_ranks(cells, w)
    got, rounds, _ = build(lib, cells.tobytes(), w, flags)
    assert got == exp, "rl_bwt differs from the oracle on ranks (%d vs %d bytes)" % (len(got), len(exp))
    assert o_rounds >= 3 and rounds < o_rounds, (rounds, o_rounds)


def level_cells(data, level, cell_bytes=1):
    """cells of the text of `level` in the oracle's trace"""
    o = oracle.OracleResult(data, cell_bytes, trace=True)
    n = len(o.level_text(level)[0])
    o.close()
    return n


_BASE_ROUND = re.compile(r"\[grlbwt\] level (-?\d+) base case sort round: (\d+) items in (\d+) groups; (.*)")
_TIERS = re.compile(r"counting (\d+), LDS (\d+) \(.*\), radix (\d+)")


def base_rounds(err):
    """(level, items, counting, LDS, radix) of every sort round of the base case in the library's trace (GRLBWT_TABLE_TRACE)"""
    out = []
    for m in map(_BASE_ROUND.match, err.splitlines()):
        if not m:
            continue
        t = _TIERS.match(m.group(4))
        items = int(m.group(2))
        out.append((int(m.group(1)), items) + (tuple(int(t.group(i)) for i in (1, 2, 3)) if t else (items, 0, 0)))
    return out


def check_tiers(lib, config, flags, monkeypatch, capfd):
    """Case (a): the reads with the base case at level 2, under the tier limits of `config`.  The trace must show that the tiers
    the limits leave open ordered groups of the base case -- so the image, which depends on equal suffixes staying in position
    order, was made through each of them -- and that the dictionary stage's own trace line did not count these rounds."""
    for k, v in suffix_rounds_cases.CONFIGS[config].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv(RATIO, FORCED)
    monkeypatch.setenv("GRLBWT_TABLE_TRACE", "1")
    capfd.readouterr()
    rounds, _ = check_forced(lib, reads(), 1, flags)
    err = capfd.readouterr().err
    assert rounds == 2
    base = base_rounds(err)
    assert base and all(r[0] == 2 for r in base), base
    counting, lds, radix = (sum(r[i] for r in base) for i in (2, 3, 4))
    if config == "default":
        assert counting > 0
    elif config == "cap1_lds3":
        assert lds > 0 and radix > 0, base
    else:
        assert counting > 0 and lds == 0 and radix > 0, base
    dict_levels = {int(m.group(1)) for m in map(suffix_rounds_cases._ROUND.match, err.splitlines()) if m}
    assert dict_levels <= {0, 1}, dict_levels
