"""Shared by tests/test_fm_ckmers_sim.py (serial stand-in) and tests/test_fm_ckmers_gpu.py (HIP library): the strand-merged
(canonical) k-mers of a collection with their mates, totals and spectrum, from its FM index (grlbwt_fm_kmers_canonical).

Expected values share no code with the engine: the k-mers, their counts and their rows lo come from tests/kmer_cases.Expected (a
Python Counter of the windows, lo by the naive LCP); the reverse complement is taken through a dict built from the pairs; the
classes are found by a walk over the table with a set of the rows already placed.  The step counters of the mate pass are
modelled from the definition with sets of the collection's substrings.  Cross-checks against the index: FmIndex.count of the
reverse complement of the emitted cells is (mate_lo, mate_lo + total - count), and the rows lo and mate_lo together are the lo
column of FmIndex.kmers.

The inputs are sized from the tiles the library reports (canonical_kmer_info() of a first tiny call), never from constants.  Every
output buffer has guard bytes right behind the entries the call may write."""
import ctypes as C

import numpy as np

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import kmer_cases as kc
from tests import merge_cases as mc

EINVAL = kc.EINVAL
DT = fc.DT
FILL = fc.FILL
NONE = fc.NONE
MAX_BINS = kc.MAX_BINS
DNA = ((65, 84), (67, 71))                  # (A,T), (C,G): what a call without pairs means
OUTS = ("cells", "lo", "count", "mate_lo", "total")
ROWS = kc.ROWS
MATE_NAMES = ["mates_tile_minus_1", "mates_tile", "mates_tile_plus_1"]
FOREIGN_FLOOR = 300                         # answered calls over tests/walk_cases.FOREIGN on both contexts (the stand-in answers 312)
STEP_MODEL_MAX_K = 16                       # the exact model of the mate pass's steps keeps every substring of up to k cells


# ------------------------------------------------------------------ expected values
class Expected:
    """the classes of every k under one complement map, from kmer_cases.Expected"""

    def __init__(self, e, pairs=None):
        self.e = e
        self.pairs = DNA if pairs is None else tuple((int(a), int(b)) for a, b in pairs)
        self.comp = {}
        for a, b in self.pairs:
            assert a not in self.comp and (b not in self.comp or a == b)
            self.comp[a], self.comp[b] = b, a
        self.present = set(int(v) for v in e.vals[1:])              # the symbols' values, the separator's aside
        self.rest = any(v not in self.comp for v in self.present)   # a symbol without a pair: the walks run to cell k - 1
        self._tab = {}
        self._sub = {}

    def rc(self, x):
        if any(v not in self.comp for v in x):
            return None
        return tuple(self.comp[v] for v in reversed(x))

    def table(self, k):
        if k in self._tab:
            return self._tab[k]
        lo, count, cells = self.e.table(k)
        keys = [tuple(int(v) for v in row) for row in cells] if len(lo) else []
        row_of = {x: i for i, x in enumerate(keys)}
        mate = []
        for x in keys:
            r = self.rc(x)
            mate.append(-2 if r is None else row_of.get(r, -1))     # -2: no reverse complement; -1: it does not occur
        placed, reps = set(), []
        for i in range(len(keys)):                                   # ascending lo: the first member met is the representative
            if i in placed:
                continue
            members = {i} | ({mate[i]} if mate[i] >= 0 else set())
            assert not (members & placed)
            placed |= members
            reps.append(i)
        reps = np.array(reps, dtype=np.int64)
        m = np.array(mate, dtype=np.int64)[reps] if len(reps) else np.zeros(0, dtype=np.int64)
        t = dict(lo=lo[reps], count=count[reps], cells=cells[reps] if len(reps) else np.zeros((0, k if k < 64 else 1), dtype=np.uint64))
        t["mate_lo"] = np.array([int(lo[j]) if j >= 0 else NONE for j in m], dtype=np.uint64)
        t["total"] = np.array([int(count[i]) + (int(count[j]) if j >= 0 and j != i else 0) for i, j in zip(reps, m)], dtype=np.uint64)
        t["n_distinct"] = len(keys)
        t["n_classes"] = len(reps)
        t["n_paired"] = int(np.count_nonzero((m >= 0) & (m != reps)))
        t["n_palindromes"] = int(np.count_nonzero(m == reps))
        t["n_single"] = int(np.count_nonzero(m < 0))
        t["n_no_complement"] = int(np.count_nonzero(m == -2))
        t["all_lo"] = lo
        t["keys"] = keys
        assert t["n_distinct"] == 2 * t["n_paired"] + t["n_palindromes"] + t["n_single"]
        assert int(t["total"].sum()) == self.e.windows(k)
        self._tab[k] = t
        return t

    def substrings(self, j):
        if j not in self._sub:
            self._sub[j] = set(s[i:i + j] for s in self.e.strings for i in range(len(s) - j + 1))
        return self._sub[j]

    def steps(self, k):
        """(mate_walks, backward_steps, forward_steps of the mate pass) by the definition of the walk: cell t is read (a forward
        step); without a pair the walk ends; while the range lives, a complement the image holds costs a backward step, and the
        range dies when comp(x_t) .. comp(x_0) is no substring; a dead range ends the walk unless a symbol has no pair"""
        walks = bwd = fwd = 0
        for x in self.table(k)["keys"]:
            dead, b, pat = False, 0, ()
            for t in range(k):
                fwd += 1
                if x[t] not in self.comp:
                    break
                if not dead:
                    c = self.comp[x[t]]
                    if c not in self.present:
                        dead = True
                    else:
                        b += 1
                        pat = (c,) + pat
                        dead = tuple(self._code_of[v] for v in pat) not in self.substrings(len(pat))
                if dead and not self.rest:
                    break
            bwd += b
            walks += 1 if b else 0
        return walks, bwd, fwd

    @property
    def _code_of(self):
        if not hasattr(self, "_co"):
            self._co = {int(v): i for i, v in enumerate(self.e.vals)}
        return self._co


_exp = {}


def expected(c, pairs=None):
    key = (id(c), None if pairs is None else tuple(tuple(p) for p in pairs))
    if key not in _exp:
        _exp[key] = (c, Expected(c.exp, pairs))
    return _exp[key][1]


# ------------------------------------------------------------------ the collections
def revcomp(s):
    return np.array([{65: 84, 84: 65, 67: 71, 71: 67}[int(v)] for v in s[::-1]], dtype=np.uint8)


def make_cases(T, MT):
    P = dict(kc.cases(T))
    rng = np.random.default_rng(20261022)
    # both strands, what -R writes: the strings, then their reverse complements; 3 T + 17 rows (one empty string makes the sum odd)
    half = (3 * T + 17 - 1) // 2
    fwd = mc.strings_to(rng, half, mc.ACGT, 1)
    P["both_strands"] = kc.Case("both_strands", mc.text(fwd + [revcomp(s) for s in fwd] + [mc.ACGT[:0]], 10, 1), 1)
    # exactly MT - 1, MT, MT + 1 distinct 6-mers: one string per k-mer
    for name, m in zip(MATE_NAMES, (MT - 1, MT, MT + 1)):
        assert m <= 4 ** 6
        ids = np.sort(rng.choice(4 ** 6, size=m, replace=False))
        strs = [mc.ACGT[[(int(i) >> (2 * j)) & 3 for j in range(6)]] for i in ids]
        P[name] = kc.Case(name, mc.text(strs, 10, 1), 1)
    # palindromes: seeded with ACGT, AATT and GAATTC; ANT for the map with (N,N)
    seeds = [np.frombuffer(s, dtype=np.uint8) for s in (b"ACGT", b"AATT", b"GAATTC", b"CANTG", b"TTANTAA", b"ACGTACGT")]
    P["palindromes"] = kc.Case("palindromes", mc.text(seeds + mc.strings_to(rng, 400, mc.ACGT, 1), 10, 1), 1)
    # reads with N
    reads = mc.strings_to(rng, 700, np.frombuffer(b"ACGTACGTACGTACGTN", dtype=np.uint8), 1)
    P["reads_with_n"] = kc.Case("reads_with_n", mc.text(reads, 10, 1), 1)
    return P


_cases = {}


def cases(T, MT):
    if (T, MT) not in _cases:
        _cases[(T, MT)] = make_cases(T, MT)
    return _cases[(T, MT)]


def tiles(ctx, mem, lib, flags):
    """(tile_rows, tile_kmers, mate_tile, stage_bytes) from a first tiny call"""
    blob = mc.build(lib, flags, np.frombuffer(b"AC\nA\n", dtype=np.uint8), 1)
    keep, p = mem.put(blob)
    with engine.FmIndex(ctx, p, len(blob)) as fm:
        assert fm.canonical_kmers_raw(1) == 2
        i = fm.canonical_kmer_info()
    assert i["tile_rows"] >= 64 and i["tile_rows"] % 64 == 0 and i["tile_kmers"] >= 64 and i["stage_bytes"] >= 8 * i["tile_kmers"], i
    assert i["mate_tile"] >= 64 and i["mate_tile"] % 64 == 0, i
    assert (i["n_distinct"], i["n_classes"], i["n_single"], i["n_no_complement"]) == (2, 2, 2, 0), i      # neither T nor G occurs
    return i["tile_rows"], i["tile_kmers"], i["mate_tile"], i["stage_bytes"]


def open_case(ctx, flags, mem, lib, name, **kw):
    T = tiles(ctx, mem, lib, flags)
    c = cases(T[0], T[2])[name]
    blob = kc.image(lib, flags, c)
    keep, img = mem.put(blob)
    return c, engine.FmIndex(ctx, img, len(blob), **kw), T


# ------------------------------------------------------------------ one call, guarded outputs, everything checked
def select(x, k, min_count=1, max_count=0, rb=0, re=None):
    t = x.table(k)
    re = x.e.n if re is None else min(re, x.e.n)
    m = (t["lo"] >= rb) & (t["lo"] < re) & (t["total"] >= max(min_count, 1))
    if max_count:
        m &= t["total"] <= max_count
    return {name: t[name][m] for name in OUTS}


def spectrum(x, k, bins):
    return np.bincount(np.minimum(x.table(k)["total"], bins - 1).astype(np.int64), minlength=bins).astype(np.uint64)


def call(fm, mem, x, k, w, min_count=1, max_count=0, rb=0, re=None, outs=OUTS, bins=None, check_count=True):
    """grlbwt_fm_kmers_canonical with buffers of exactly the expected size, guards right behind; everything it wrote against `x`"""
    e = x.e
    want = select(x, k, min_count, max_count, rb, re)
    m = len(want["lo"])
    size = {name: 8 * m for name in OUTS}
    size["cells"] = m * k * w
    bufs = {name: mem.out(size[name]) for name in OUTS}
    spec = None if bins is None else np.full(bins + 2, 7, dtype=np.uint64)
    ptr = {name: bufs[name][1] if name in outs else None for name in OUTS}
    got = fm.canonical_kmers_raw(k, min_count, max_count, rb, re, None if x.pairs is DNA else x.pairs, w, ptr["cells"], ptr["lo"], ptr["count"],
                                 ptr["mate_lo"], ptr["total"], m, None if bins is None else spec[:bins])
    assert got == m, (got, m)
    info = fm.canonical_kmer_info()
    t = x.table(k)
    assert (info["k"], info["n_rows"], info["n_strings"]) == (k, e.n, e.n_strings), info
    for name in ("n_distinct", "n_classes", "n_paired", "n_palindromes", "n_single", "n_no_complement"):
        assert info[name] == t[name], (name, info, t[name])
    assert info["n_selected"] == m and info["n_windows"] == e.windows(k), info
    assert info["largest_total"] == (int(t["total"].max()) if t["n_classes"] else 0), info
    assert info["passes"] <= max(k - 1, 0) and info["passes"] + info["length_passes"] <= min(k - 1, e.longest + 1), info
    assert info["scratch_bytes"] >= e.n // 2 + t["n_distinct"] * 4, info
    decode = m * k if "cells" in outs else 0
    if k <= STEP_MODEL_MAX_K:
        walks, bwd, fwd = x.steps(k)
        assert (info["mate_walks"], info["backward_steps"], info["forward_steps"]) == (walks, bwd, fwd + decode), (info, walks, bwd, fwd, decode)
    assert info["mate_walks"] <= t["n_distinct"] and info["backward_steps"] <= info["forward_steps"] - decode <= t["n_distinct"] * k, info
    assert info["backward_steps"] >= k * (2 * t["n_paired"] + t["n_palindromes"]), info        # a search that finds its mate takes k steps
    for name in OUTS:
        if name in outs:
            dt = DT[w] if name == "cells" else np.uint64
            have = mem.body(bufs[name][0], size[name]).view(dt)
            ref = want[name].astype(dt).reshape(-1)
            assert np.array_equal(have, ref), (name, k, np.flatnonzero(have != ref)[:5])
        else:
            assert bool(np.all(mem.get(bufs[name][0]) == FILL)), name
    if bins is not None:
        assert np.array_equal(spec[:bins], spectrum(x, k, bins)) and bool(np.all(spec[bins:] == 7)), (k, bins)
        assert int(spec[:bins].sum()) == t["n_classes"]
    if check_count and m and "cells" in outs:       # what grlbwt_fm_count answers for the reverse complement of the emitted cells
        have = mem.body(bufs["cells"][0], size["cells"]).view(DT[w]).reshape(m, k)
        rcs = [x.rc(tuple(int(v) for v in row)) for row in have]
        idx = [i for i, r in enumerate(rcs) if r is not None and all(fc.fits([v], w) for v in r)]
        ranges = fc.count(fm, mem, [list(rcs[i]) for i in idx], w)
        for i, (a, b) in zip(idx, ranges):
            ml, tot, cnt, lo = (int(want[name][i]) for name in ("mate_lo", "total", "count", "lo"))
            if ml == NONE:
                assert a == b, (i, a, b)
            elif ml == lo:
                assert (a, b) == (lo, lo + cnt) and tot == cnt, (i, a, b)
            else:
                assert (a, b) == (ml, ml + tot - cnt), (i, a, b, ml, tot, cnt)
        assert all(int(want["mate_lo"][i]) == NONE for i, r in enumerate(rcs) if r is None)
    return info


# ------------------------------------------------------------------ the cases
def run_rows(ctx, flags, mem, lib, name):
    """rows around the tiles: the whole table at k = 1, 2, 5, 7 and 12 with a spectrum; walks that run all k steps beside walks that
    empty early"""
    c, fm, _ = open_case(ctx, flags, mem, lib, name)
    x = expected(c)
    for k in (1, 2):
        assert x.table(k)["n_single"] == 0 and x.table(k)["n_classes"] > 0
    t = x.table(12)
    assert t["n_single"] > 4 * (t["n_paired"] + t["n_palindromes"])
    assert any(0 < x.table(k)["n_single"] and 0 < x.table(k)["n_paired"] for k in (5, 7, 12))      # both kinds of walk side by side
    with fm:
        for k in (1, 2, 5, 7, 12):
            info = call(fm, mem, x, k, c.w, bins=64)
            t = x.table(k)
            paired = t["mate_lo"][(t["mate_lo"] != NONE) & (t["mate_lo"] != t["lo"])]
            lo, _, _ = fm.kmers(k, cells=False)
            assert np.array_equal(np.sort(np.concatenate([t["lo"], paired])), lo) and len(lo) == info["n_distinct"]


def run_sizes_follow_the_tiles(ctx, flags, mem, lib):
    T, TK, MT, _ = tiles(ctx, mem, lib, flags)
    P = cases(T, MT)
    assert P["both_strands"].n == 3 * T + 17
    for name, m in zip(MATE_NAMES, (MT - 1, MT, MT + 1)):
        assert len(P[name].exp.table(6)[0]) == m, name
    assert expected(P["rows_three_tiles_17"]).table(5)["n_classes"] > TK + 1


def run_both_strands(ctx, flags, mem, lib):
    c, fm, _ = open_case(ctx, flags, mem, lib, "both_strands")
    x = expected(c)
    with fm:
        for k in (4, 7, 16):
            info = call(fm, mem, x, k, 1, bins=32)
            t = x.table(k)
            assert info["n_single"] == 0 and info["n_classes"] * 2 == info["n_distinct"] + info["n_palindromes"], info
            pair = t["mate_lo"] != t["lo"]
            assert bool(np.all(t["total"][pair] % 2 == 0)) and bool(np.all(t["total"][pair] == 2 * t["count"][pair]))
            assert info["backward_steps"] == info["n_distinct"] * k                 # every search runs all k steps
        assert x.table(4)["n_palindromes"] > 0 and x.table(7)["n_palindromes"] == 0


def run_heads_around_the_mate_tile(ctx, flags, mem, lib):
    """mate_tile - 1, mate_tile, mate_tile + 1 heads: the last workgroup of the mate kernel is full, one short, one over"""
    for name in MATE_NAMES:
        c, fm, (T, TK, MT, _) = open_case(ctx, flags, mem, lib, name)
        with fm:
            info = call(fm, mem, expected(c), 6, 1, bins=8)
            assert info["n_distinct"] - MT == MATE_NAMES.index(name) - 1
            call(fm, mem, expected(c), 3, 1)


def run_entries_around_the_decode_tile(ctx, flags, mem, lib):
    """tile_kmers - 1, tile_kmers, tile_kmers + 1 selected classes, through the row window and through min_count"""
    c, fm, (T, TK, _, _) = open_case(ctx, flags, mem, lib, "rows_three_tiles_17")
    x = expected(c)
    with fm:
        t = x.table(5)
        assert t["n_classes"] > TK + 8
        for m in (TK - 1, TK, TK + 1):
            assert call(fm, mem, x, 5, 1, rb=0, re=int(t["lo"][m]))["n_selected"] == m
            assert call(fm, mem, x, 5, 1, rb=int(t["lo"][7]), re=int(t["lo"][7 + m]))["n_selected"] == m
        t = x.table(6)
        rep = t["lo"][t["total"] >= 3]
        assert len(rep) > TK + 1, len(rep)
        for m in (TK - 1, TK, TK + 1):
            assert call(fm, mem, x, 6, 1, min_count=3, re=int(rep[m]))["n_selected"] == m


def run_palindromes(ctx, flags, mem, lib):
    c, fm, _ = open_case(ctx, flags, mem, lib, "palindromes")
    x = expected(c)
    xn = expected(c, DNA + ((78, 78),))
    with fm:
        for k in (2, 4, 6, 8):
            info = call(fm, mem, x, k, 1, bins=8)
            assert info["n_palindromes"] > 0, k
        for k in (1, 3, 5, 7):
            assert call(fm, mem, x, k, 1)["n_palindromes"] == 0
        t = x.table(4)
        for word in (b"ACGT", b"AATT"):
            i = t["keys"].index(tuple(word))
            j = int(np.flatnonzero(t["lo"] == t["all_lo"][i])[0])
            assert t["mate_lo"][j] == t["lo"][j] and t["total"][j] == t["count"][j]
        assert tuple(b"GAATTC") in [tuple(int(v) for v in r) for r in x.table(6)["cells"][x.table(6)["mate_lo"] == x.table(6)["lo"]]]
        # (N,N): ANT is its own reverse complement
        info = call(fm, mem, xn, 3, 1, bins=8)
        t = xn.table(3)
        ant = [j for j, r in enumerate(t["cells"]) if tuple(int(v) for v in r) == tuple(b"ANT")]
        assert len(ant) == 1 and t["mate_lo"][ant[0]] == t["lo"][ant[0]] and info["n_palindromes"] >= 1 and info["n_no_complement"] == 0
        assert x.table(3)["n_no_complement"] > 0 and x.table(3)["n_palindromes"] == 0
        call(fm, mem, xn, 5, 1)
        call(fm, mem, xn, 7, 1)


def run_no_complement(ctx, flags, mem, lib, name):
    """symbols the map does not name: N in reads, Z, a whole alphabet"""
    c, fm, _ = open_case(ctx, flags, mem, lib, name)
    x = expected(c)
    with fm:
        for k in (1, 2, 3, 6):
            info = call(fm, mem, x, k, 8, bins=16)
            t = x.table(k)
            nc = [not all(int(v) in x.comp for v in r) for r in t["cells"]]
            assert info["n_no_complement"] == sum(nc)
            assert all(t["mate_lo"][i] == NONE and t["total"][i] == t["count"][i] for i, f in enumerate(nc) if f)
        if name == "reads_with_n":
            assert 0 < x.table(6)["n_no_complement"] < x.table(6)["n_single"] and x.table(6)["n_paired"] > 0
        if name == "sigma_256":
            assert x.table(2)["n_no_complement"] == x.table(2)["n_distinct"] and fm.canonical_kmer_info()["mate_walks"] == 0


def run_other_alphabets(ctx, flags, mem, lib, name):
    """custom pairs over the values of a two-byte and of a compacted 64-bit alphabet"""
    c, fm, _ = open_case(ctx, flags, mem, lib, name)
    e = c.exp
    v = [int(a) for a in e.vals[1:]]
    assert len(v) >= 6
    absent = max(v) + 5
    assert absent not in v and absent != int(e.vals[0])
    f = [int(a) for a in e.table(1)[2].reshape(-1)[np.argsort(-e.table(1)[1].astype(np.int64), kind="stable")] if int(a) != max(v)]
    maps = [
        ((f[0], f[1]), (f[2], f[2]), (max(v), f[3])),                  # the most frequent symbols paired, one with itself, the largest value
        tuple((a, b) for a, b in zip(v[0::2], v[1::2]))[:127] + ((absent, absent + 1),),      # everything that fits, and a pair of values not held
        ((v[0], absent),),                                             # a complement the image does not hold
        ((absent, absent + 1), (absent + 2, absent + 2)),              # nothing present is paired
    ]
    with fm:
        for pairs in maps:
            x = expected(c, pairs)
            for k in (1, 2, 3):
                info = call(fm, mem, x, k, 8, bins=8)
        x = expected(c, maps[3])
        for k in (1, 2, 4):
            t = x.table(k)
            lo, count, cells = e.table(k)
            assert np.array_equal(t["lo"], lo) and np.array_equal(t["total"], count) and bool(np.all(t["mate_lo"] == NONE))
            assert call(fm, mem, x, k, 8)["n_no_complement"] == len(lo)
        assert expected(c, maps[0]).table(1)["n_paired"] == 2 and expected(c, maps[0]).table(1)["n_palindromes"] == 1
        assert expected(c, maps[2]).table(1)["n_no_complement"] == len(v) - 1 and expected(c, maps[2]).table(1)["n_single"] == len(v)
        if name == "wide_u64":
            assert max(v) == 2 ** 63 + 11
            m = expected(c, maps[0]).table(2)["n_classes"]
            buf, p = mem.out(m * 2 * 4)
            msg = fc.einval(lambda: fm.canonical_kmers_raw(2, pairs=maps[0], cell_bytes=4, cells_ptr=p, capacity=m))
            assert "does not fit" in msg and bool(np.all(mem.get(buf) == FILL))


def run_values_of_k(ctx, flags, mem, lib):
    c, fm, (T, TK, MT, stage) = open_case(ctx, flags, mem, lib, "rows_tile_plus_1")
    x = expected(c)
    e = c.exp
    with fm:
        call(fm, mem, x, 1, 1, bins=8)
        big = stage // (8 * TK) + 3                                     # chunked staging: k * 8 * tile_kmers is above the LDS
        assert big * 8 * TK > stage and big <= e.longest and x.table(big)["n_classes"] > TK
        call(fm, mem, x, big, 8)
        info = call(fm, mem, x, e.longest, 1, bins=4)                   # k = the longest string
        assert info["n_distinct"] >= 1
        for k in (e.longest + 1, 2 ** 63):                              # longer than every string: no k-mer
            info = call(fm, mem, x, k, 1, bins=4)
            assert all(info[f] == 0 for f in ("n_distinct", "n_windows", "n_selected", "n_classes", "n_paired", "n_palindromes", "n_single",
                                              "n_no_complement", "largest_total", "mate_walks", "backward_steps", "forward_steps")), info


def run_one_symbol(ctx, flags, mem, lib):
    c, fm, (T, _, _, _) = open_case(ctx, flags, mem, lib, "one_symbol")
    x, xa = expected(c), expected(c, ((65, 65),))
    with fm:
        for k in (1, 7, 70):
            info = call(fm, mem, x, k, 1, bins=MAX_BINS)                # T does not occur: one class, single
            assert (info["n_classes"], info["n_single"], info["n_no_complement"], info["largest_total"]) == (1, 1, 0, 3 * T - k + 1), info
            assert (info["mate_walks"], info["backward_steps"], info["forward_steps"]) == (0, 0, 1 + k), info
            info = call(fm, mem, xa, k, 1, bins=2)                      # (A,A): a palindrome
            assert (info["n_classes"], info["n_palindromes"], info["n_single"], info["backward_steps"]) == (1, 1, 0, k), info
            call(fm, mem, xa, k, 1, rb=k + 1)                           # the head lies in front of the window: an empty table


def run_filters_windows_sizing(ctx, flags, mem, lib):
    c, fm, (T, TK, _, _) = open_case(ctx, flags, mem, lib, "rows_three_tiles_17")
    x = expected(c)
    e = c.exp
    L = ctx.L
    with fm:
        t = x.table(6)
        by_mate = (t["count"] < 2) & (t["total"] >= 2)
        assert int(np.count_nonzero(by_mate)) > 0                       # a class that passes min_count = 2 only because of its mate
        info = call(fm, mem, x, 6, 1, min_count=2)
        assert info["n_selected"] == int(np.count_nonzero(t["total"] >= 2)) > int(np.count_nonzero(t["count"] >= 2))
        top = int(t["total"].max())
        assert 0 < call(fm, mem, x, 6, 1, min_count=2, max_count=top - 1)["n_selected"] < info["n_selected"]
        assert call(fm, mem, x, 6, 1, max_count=1)["n_selected"] == int(np.count_nonzero(t["total"] == 1))
        cuts = [0, 1, e.n_strings, T - 1, T - 1, T + 64, 2 * T + 5, e.n]      # (an empty window among them)
        total = 0
        for a, b in zip(cuts, cuts[1:]):
            total += call(fm, mem, x, 6, 1, rb=a, re=b, check_count=False)["n_selected"]
        assert total == t["n_classes"]
        call(fm, mem, x, 6, 1, rb=e.n, re=engine.UINT64_MAX, check_count=False)      # clamped to [n, n): empty
        for outs in tuple((name,) for name in OUTS) + ((),):
            call(fm, mem, x, 4, 1, outs=outs, bins=16 if not outs else None)
            call(fm, mem, x, 4, 1, outs=outs, bins=16)
        m = x.table(4)["n_classes"]
        assert fm.canonical_kmers_raw(4) == m                           # n_classes_out alone, capacity 0
        bufs = [mem.out(m * 4)] + [mem.out(8 * m) for _ in range(4)]
        spec = np.full(16, 7, dtype=np.uint64)
        for which in ((0, 1, 2, 3, 4), (0,), (1,), (2,), (3,), (4,)):
            p = [C.c_void_p(bufs[i][1]) if i in which else None for i in range(5)]
            got = C.c_uint64(0)
            rc = L.grlbwt_fm_kmers_canonical(ctx._h, fm._h, 4, 1, 0, 0, engine.UINT64_MAX, None, 0, 1, p[0], p[1], p[2], p[3], p[4], m - 1,
                                             C.byref(got), spec.ctypes.data_as(C.c_void_p), 16)
            assert rc == EINVAL and got.value == m and "GRLBWT" not in L.grlbwt_last_error(ctx._h).decode()
            assert all(bool(np.all(mem.get(b) == FILL)) for b, _ in bufs) and bool(np.all(spec == 7))
            assert fm.canonical_kmer_info()["n_selected"] == m          # the call got as far as counting
        lo, count, mate_lo, tot, cells = fm.canonical_kmers(4)          # the binding sizes by the idiom
        want = x.table(4)
        assert all(np.array_equal(a, want[name]) for a, name in ((lo, "lo"), (count, "count"), (mate_lo, "mate_lo"), (tot, "total")))
        assert cells.dtype == np.uint8 and cells.shape == (m, 4) and np.array_equal(cells.astype(np.uint64), want["cells"])
        got = fm.canonical_kmers(4, min_count=3, rows=(int(want["lo"][3]), int(want["lo"][-2])), cells=False, pairs=b"ATCG")
        sel = select(x, 4, 3, 0, int(want["lo"][3]), int(want["lo"][-2]))
        assert got[4] is None and all(np.array_equal(a, sel[name]) for a, name in zip(got, ("lo", "count", "mate_lo", "total")))
        assert np.array_equal(fm.canonical_kmer_spectrum(4, 9), spectrum(x, 4, 9))
        assert np.array_equal(fm.canonical_kmer_spectrum(4, 9, pairs=[(65, 84), (67, 71)]), spectrum(x, 4, 9))


def run_spectrum_bins(ctx, flags, mem, lib):
    c, fm, _ = open_case(ctx, flags, mem, lib, "rows_tile_minus_1")
    x = expected(c)
    with fm:
        k = 3
        top = int(x.table(k)["total"].max())
        assert top > 3
        info = call(fm, mem, x, k, 1, outs=(), bins=1)                  # one bin: the last one, bin 0 = n_classes
        assert int(spectrum(x, k, 1)[0]) == info["n_classes"]
        for bins in (2, top + 1, top, MAX_BINS):
            call(fm, mem, x, k, 1, outs=(), bins=bins)
        s = spectrum(x, k, top + 1)
        assert s[0] == 0 and s[top] >= 1 and spectrum(x, k, top)[top - 1] == s[top - 1] + s[top]
        spec = np.full(MAX_BINS + 1, 7, dtype=np.uint64)
        fc.einval(lambda: fm.canonical_kmers_raw(k, spectrum=spec))
        fc.einval(lambda: fm.canonical_kmers_raw(k, spectrum=spec[:0]))
        assert bool(np.all(spec == 7))


def run_refusals(ctx, flags, mem, lib):
    c, fm, _ = open_case(ctx, flags, mem, lib, "rows_tile_minus_1")
    L = ctx.L
    x = expected(c)
    with fm:
        m = x.table(2)["n_classes"]
        bufs = [mem.out(m * 2)] + [mem.out(8 * m) for _ in range(4)]
        pc, pl, pn, pm, pt = (b[1] for b in bufs)
        spec = np.full(8, 7, dtype=np.uint64)
        all_out = dict(cells_ptr=pc, lo_ptr=pl, count_ptr=pn, mate_lo_ptr=pm, total_ptr=pt, capacity=m, spectrum=spec)

        def untouched():
            return all(bool(np.all(mem.get(b) == FILL)) for b, _ in bufs) and bool(np.all(spec == 7))

        def raw(k, pairs_ptr, n_pairs, cell_bytes=1, rb=0, re=engine.UINT64_MAX, fmh=fm._h, outs=True):
            got = C.c_uint64(99)
            p = [C.c_void_p(b) if outs else None for b in (pc, pl, pn, pm, pt)]
            rc = L.grlbwt_fm_kmers_canonical(ctx._h, fmh, k, 1, 0, rb, re, pairs_ptr, n_pairs, cell_bytes, p[0], p[1], p[2], p[3], p[4], m,
                                             C.byref(got) if outs else None, spec.ctypes.data_as(C.c_void_p) if outs else None, 8 if outs else 0)
            return rc, got.value, L.grlbwt_last_error(ctx._h).decode()

        # those of grlbwt_fm_kmers
        fc.einval(lambda: fm.canonical_kmers_raw(0, **all_out))                                          # k = 0
        for w in (0, 3, 16):
            fc.einval(lambda: fm.canonical_kmers_raw(2, cell_bytes=w, **all_out))
        fc.einval(lambda: fm.canonical_kmers_raw(2, row_begin=5, row_end=4, lo_ptr=pl, capacity=m, spectrum=spec))
        fc.einval(lambda: fm.canonical_kmers_raw(2, row_begin=x.e.n + 1, total_ptr=pt, capacity=m, spectrum=spec))      # above the clamped end
        assert raw(2, None, 0, outs=False)[0] == EINVAL                                                 # no output at all
        fc.einval(lambda: fm.canonical_kmers_raw(2, lo_ptr=pl + 4, capacity=m))                          # not aligned
        fc.einval(lambda: fm.canonical_kmers_raw(2, mate_lo_ptr=pm + 1, capacity=m))
        assert untouched()
        # the complement map
        many = (C.c_uint64 * 258)(*range(1000, 1258))
        rc, got, msg = raw(2, C.cast(many, C.c_void_p), 129)
        assert rc == EINVAL and got == 0 and "129" in msg, msg
        rc, got, msg = raw(2, None, 3)
        assert rc == EINVAL and got == 0 and "NULL" in msg and "3" in msg, msg
        every = len(x.e.table(2)[0])                                                                    # (legal: 128 pairs, an empty map)
        assert fm.canonical_kmers_raw(2, pairs=[(1000 + 2 * i, 1001 + 2 * i) for i in range(128)]) == every
        assert fm.canonical_kmers_raw(2, pairs=()) == every and fm.canonical_kmer_info()["n_no_complement"] == every
        for pairs, bad in ((((65, 84), (65, 71)), 65), (((65, 84), (67, 84)), 84), (((65, 84), (84, 65)), 65), (((65, 84), (65, 84)), 65),
                           (((67, 67), (67, 71)), 67), (((65, 84), (10, 71)), 10), (((10, 10),), 10)):
            msg = fc.einval(lambda: fm.canonical_kmers_raw(2, pairs=pairs, **all_out))
            assert str(bad) in msg, (pairs, msg)
            if bad == 10:
                assert "separator" in msg, msg
        assert untouched()
        # a null index, null info
        rc, got, _ = raw(2, None, 0, fmh=None)
        assert rc == EINVAL and got == 0
        assert L.grlbwt_fm_kmers_canonical_info_get(None, None) == EINVAL and L.grlbwt_fm_kmers_canonical_info_get(fm._h, None) == EINVAL
        assert untouched()
    bad = ic.make_image(1, 1, [10, 65], [1, 2])              # not the BWT of a collection: the row of the second A is LF of itself
    keep, img = mem.put(bad)
    with engine.FmIndex(ctx, img, len(bad)) as fm:
        msg = fc.einval(lambda: fm.canonical_kmers_raw(3, **all_out))
        assert "not the BWT of a collection" in msg and untouched(), msg


def run_index_unchanged(ctx, flags, mem, lib):
    col = fc.COLS["dna"]
    pats = fc.collection_patterns(col)
    blob = fc.image_of(lib, col, flags)
    e = kc.Expected(col.data)
    x = Expected(e)
    for kw in ({}, {"locate": True}, {"locate": True, "checkpoints": True, "sample_bits": 3}, {"locate": True, "extract": True}):
        keep, img = mem.put(blob)
        with engine.FmIndex(ctx, img, len(blob), **kw) as fm:
            del keep
            kc.call(fm, mem, e, 4, 1, bins=8)                           # an earlier plain call: its counters stay
            before, counts, kinfo = fm.info(), fc.count(fm, mem, pats, 1), fm.kmer_info()
            buf, ptr = mem.out(e.n)
            lcp_before = (fm.lcp(0, 1, ptr), mem.body(buf, e.n).tobytes())
            call(fm, mem, x, 3, 1, bins=8)
            call(fm, mem, x, 7, 4, min_count=2)
            assert fm.info() == before and fc.count(fm, mem, pats, 1) == counts and fm.kmer_info() == kinfo, kw
            buf, ptr = mem.out(e.n)
            after = (fm.lcp(0, 1, ptr), mem.body(buf, e.n).tobytes())
            assert lcp_before[1] == after[1] and all(np.array_equal(a, b) for a, b in zip(lcp_before[0], after[0]))
            kc.call(fm, mem, e, 4, 1, bins=8)                           # and a plain call answers as before


def run_foreign(ctx, mem, c):
    """an image the engine did not make is refused or answered, and never runs past the guards; returns (answered, refused)"""
    blob = c.image()
    keep, img = mem.put(blob)
    try:
        fm = engine.FmIndex(ctx, img, len(blob))
    except engine.GrlbwtError as e:
        assert e.code == EINVAL, e
        return 0, 1
    done = refused = 0
    with fm:
        n = fm.info()["n_syms"]
        vals = sorted(set(int(v) for v in c.syms)) if hasattr(c, "syms") else []
        for k in (1, 2, 5):
            for pairs in (None, tuple((a, b) for a, b in zip(vals[1::2], vals[2::2]))[:128])[:2 if k == 2 else 1]:
                try:
                    m = fm.canonical_kmers_raw(k, pairs=pairs)
                except engine.GrlbwtError as e:
                    assert e.code == EINVAL, e
                    refused += 1
                    continue
                assert m <= n and fm.canonical_kmer_info()["n_selected"] == m
                bufs = [mem.out(m * k * 8)] + [mem.out(8 * m) for _ in range(4)]
                spec = np.full(10, 7, dtype=np.uint64)
                assert fm.canonical_kmers_raw(k, pairs=pairs, cell_bytes=8, cells_ptr=bufs[0][1], lo_ptr=bufs[1][1], count_ptr=bufs[2][1],
                                              mate_lo_ptr=bufs[3][1], total_ptr=bufs[4][1], capacity=m, spectrum=spec[:8]) == m
                lo, cnt, mate, tot = (mem.body(b[0], 8 * m).view(np.uint64) for b in bufs[1:])
                mem.body(bufs[0][0], m * k * 8)
                assert bool(np.all(spec[8:] == 7)) and int(spec[:8].sum()) == fm.canonical_kmer_info()["n_classes"]
                assert bool(np.all(lo[1:] > lo[:-1])) and bool(np.all(lo + cnt <= n)) and bool(np.all(cnt >= 1)) and bool(np.all(tot >= cnt))
                assert bool(np.all((mate == NONE) | (mate >= lo)))
                done += 1
    return done, refused
