"""Shared by tests/test_fm_kmers_sim.py (serial stand-in) and tests/test_fm_kmers_gpu.py (HIP library): the distinct k-mers of a
collection with their counts, and the abundance spectrum, from its FM index (grlbwt_fm_kmers).

Expected values share no code with the engine: a Python Counter of the windows of the rank-coded strings, sorted as tuples, gives
the k-mers in table order with their counts; the rows `lo` come from the LCP BY DEFINITION of tests/lcp_cases.py (a head is a row
with LCP < k whose suffix has at least k cells), whose counts must agree with the Counter's.  Cross-checks against the index:
FmIndex.count of the emitted cells is (lo, lo + count), the spectrum sums to distinct_kmers(k) of FmIndex.lcp where the passes got
that far, n_windows is the sum over the strings of max(0, len - k + 1).

The inputs are sized from the tiles the library reports (kmer_info() of a first tiny call), never from constants.  Every output
buffer has guard bytes right behind the entries the call may write."""
import ctypes as C
from collections import Counter

import numpy as np

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import lcp_cases as lc
from tests import merge_cases as mc

EINVAL = -22
DT = fc.DT
FILL = fc.FILL
MAX_BINS = 16384
ROWS = ["rows_tile_minus_1", "rows_tile", "rows_tile_plus_1", "rows_three_tiles_17"]
SMALL = ["twice", "one_string", "one_empty_string", "empty_strings", "rare_symbol", "two_bytes", "sigma_256", "wide_u64"]
NAMES = ROWS + SMALL + ["one_symbol", "early_distinct"]


# ------------------------------------------------------------------ expected values
class Expected:
    """the table of every k by the Counter; lo by the naive LCP (or given: `lo_of`, for a collection too long for the matrix)"""

    def __init__(self, cells, lo_of=None):
        cells = np.asarray(cells)
        self.n = len(cells)
        vals, inv = np.unique(cells, return_inverse=True)
        assert int(vals[0]) == int(cells[-1])
        self.vals = vals.astype(np.uint64)
        self.strings = [tuple(int(v) for v in s) for s in lc.split(inv.astype(np.int64))]
        self.n_strings = len(self.strings)
        self.longest = max(len(s) for s in self.strings)
        self.lo_of = lo_of
        self.naive = None if lo_of else lc.Expected(cells)
        self._tab = {}

    def table(self, k):
        """(lo, count, cells as values, shape (m, k)) of all k-mers, in table order"""
        if k not in self._tab:
            cnt = Counter()
            for s in self.strings:
                cnt.update(s[j:j + k] for j in range(len(s) - k + 1))
            keys = sorted(cnt)
            count = np.array([cnt[x] for x in keys], dtype=np.uint64)
            cells = self.vals[np.array(keys, dtype=np.int64).reshape(len(keys), k)] if keys else np.zeros((0, 1), dtype=np.uint64)
            if self.lo_of:
                lo = np.array(self.lo_of(k), dtype=np.uint64)
            else:
                e = self.naive
                bound = np.flatnonzero(e.lcp < k)
                heads = np.flatnonzero((e.lcp < k) & (e.slen >= k))
                nxt = np.append(bound, self.n)[np.searchsorted(bound, heads, side="right")]
                assert np.array_equal((nxt - heads).astype(np.uint64), count), "the Counter and the naive LCP disagree"
                lo = heads.astype(np.uint64)
            assert len(lo) == len(keys)
            self._tab[k] = (lo, count, cells)
        return self._tab[k]

    def windows(self, k):
        return sum(max(0, len(s) - k + 1) for s in self.strings)


class Case:
    def __init__(self, name, cells, w, lo_of=None):
        self.name, self.cells, self.w, self.lo_of = name, np.asarray(cells, dtype=DT[w]), w, lo_of
        self.n = len(self.cells)
        self._exp = None

    @property
    def exp(self):
        if self._exp is None:
            self._exp = Expected(self.cells, self.lo_of)
        return self._exp


def make_cases(T):
    P = {n: c for n, c in lc.cases(T).items() if n in ROWS + SMALL}
    P = {n: Case(n, c.cells, c.w) for n, c in P.items()}
    # one string of 3 T equal cells: the suffix of L cells is row L (the terminator sorts first), so the one k-mer heads row k
    one = np.concatenate([np.repeat(mc.ACGT[:1], 3 * T), [10]]).astype(np.uint8)
    P["one_symbol"] = Case("one_symbol", one, 1, lo_of=lambda k: [k] if k <= 3 * T else [])
    # early-distinct: 200 symbols, lengths 2 to 30: every suffix differs from its neighbours long before 9 cells
    rng = np.random.default_rng(20261021)
    pool = 300 + 7 * np.arange(200)
    strs = [pool[rng.integers(0, 200, size=int(rng.integers(2, 31)))] for _ in range(300)]
    P["early_distinct"] = Case("early_distinct", mc.text(strs, 5, 2), 2)
    assert sorted(P) == sorted(NAMES)
    return P


_cases = {}


def cases(T):
    if T not in _cases:
        _cases[T] = make_cases(T)
    return _cases[T]


def tiles(ctx, mem, lib, flags):
    """(tile_rows, tile_kmers, stage_bytes) from a first tiny call"""
    blob = mc.build(lib, flags, np.frombuffer(b"AC\nA\n", dtype=np.uint8), 1)
    keep, p = mem.put(blob)
    with engine.FmIndex(ctx, p, len(blob)) as fm:
        assert fm.kmers_raw(1) == 2
        i = fm.kmer_info()
    assert i["tile_rows"] >= 64 and i["tile_rows"] % 64 == 0 and i["tile_kmers"] >= 64 and i["stage_bytes"] >= 8 * i["tile_kmers"], i
    return i["tile_rows"], i["tile_kmers"], i["stage_bytes"]


def image(lib, flags, c):
    blob = mc.build(lib, flags, c.cells, c.w)
    if c.exp.naive is not None:
        assert np.array_equal(mc.decode(blob), c.exp.naive.bwt), c.name           # the rows are the sorted suffixes
    return blob


def open_case(ctx, flags, mem, lib, name, **kw):
    T = tiles(ctx, mem, lib, flags)
    c = cases(T[0])[name]
    blob = image(lib, flags, c)
    keep, img = mem.put(blob)
    return c, engine.FmIndex(ctx, img, len(blob), **kw), T


# ------------------------------------------------------------------ one call, guarded outputs, everything checked
def select(e, k, min_count=1, max_count=0, rb=0, re=None):
    lo, count, cells = e.table(k)
    re = e.n if re is None else min(re, e.n)
    m = (lo >= rb) & (lo < re) & (count >= max(min_count, 1))
    if max_count:
        m &= count <= max_count
    return lo[m], count[m], cells[m]


def spectrum(e, k, bins):
    _, count, _ = e.table(k)
    return np.bincount(np.minimum(count, bins - 1).astype(np.int64), minlength=bins).astype(np.uint64)


def call(fm, mem, e, k, w, min_count=1, max_count=0, rb=0, re=None, outs=("cells", "lo", "count"), bins=None, check_count=True):
    """grlbwt_fm_kmers with buffers of exactly the expected size, guards right behind; everything it wrote against `e`"""
    lo, count, cells = select(e, k, min_count, max_count, rb, re)
    m = len(lo)
    bc_, pc = mem.out(m * k * w)
    bl, pl = mem.out(8 * m)
    bn, pn = mem.out(8 * m)
    spec = None if bins is None else np.full(bins + 2, 7, dtype=np.uint64)
    got = fm.kmers_raw(k, min_count, max_count, rb, re, w, pc if "cells" in outs else None, pl if "lo" in outs else None,
                       pn if "count" in outs else None, m, None if bins is None else spec[:bins])
    assert got == m, (got, m)
    info = fm.kmer_info()
    tab = e.table(k)
    assert (info["k"], info["n_rows"], info["n_strings"]) == (k, e.n, e.n_strings), info
    assert (info["n_distinct"], info["n_selected"]) == (len(tab[0]), m), info
    assert info["n_windows"] == e.windows(k) == int(tab[1].sum()), info
    assert info["largest_count"] == (int(tab[1].max()) if len(tab[1]) else 0), info
    assert info["forward_steps"] == (m * k if "cells" in outs else 0), info
    assert info["passes"] <= max(k - 1, 0) and info["passes"] + info["length_passes"] <= min(k - 1, e.longest + 1), info
    assert info["scratch_bytes"] >= e.n // 2, info
    for name, buf, nbytes, want in (("cells", bc_, m * k * w, cells.astype(DT[w])), ("lo", bl, 8 * m, lo), ("count", bn, 8 * m, count)):
        if name in outs:
            have = mem.body(buf, nbytes).view(want.dtype)
            assert np.array_equal(have, want.reshape(-1)), (name, k, np.flatnonzero(have != want.reshape(-1))[:5])
        else:
            assert bool(np.all(mem.get(buf) == FILL)), name
    if bins is not None:
        assert np.array_equal(spec[:bins], spectrum(e, k, bins)) and bool(np.all(spec[bins:] == 7)), (k, bins)
        assert int(spec[:bins].sum()) == len(tab[0])
    if check_count and m and "cells" in outs:       # what grlbwt_fm_count answers for the emitted cells
        have = mem.body(bc_, m * k * w).view(DT[w]).reshape(m, k)
        ranges = fc.count(fm, mem, [[int(v) for v in row] for row in have], w)
        assert ranges == [(int(a), int(a + b)) for a, b in zip(lo, count)]
    return info


def lcp_distinct(fm, k):
    """distinct_kmers(k) of FmIndex.lcp, where its passes got that far (else None)"""
    ra, su = fm.lcp(k, 8, None)
    return engine.FmIndex.distinct_kmers(ra, su, k) if k <= len(ra) else None


# ------------------------------------------------------------------ the cases
def run_rows(ctx, flags, mem, lib, name):
    """rows around the tiles: the whole table at k = 1, 2, 5 and a larger one, with a spectrum"""
    c, fm, _ = open_case(ctx, flags, mem, lib, name)
    with fm:
        e = c.exp
        for k in (1, 2, 5, 12):
            info = call(fm, mem, e, k, c.w, bins=64)
            d = lcp_distinct(fm, k)
            assert d is None or d == info["n_distinct"], (k, d, info)
        assert lcp_distinct(fm, 2) is not None


def run_sizes_follow_the_tiles(ctx, flags, mem, lib):
    T, TK, _ = tiles(ctx, mem, lib, flags)
    P = cases(T)
    assert [P[n].n for n in ROWS] == [T - 1, T, T + 1, 3 * T + 17]
    assert P["one_symbol"].n == 3 * T + 1 and len(np.unique(P["one_symbol"].cells)) == 2
    e = P["early_distinct"].exp
    lens = [len(s) for s in e.strings]
    assert min(lens) == 2 and max(lens) == 30 and int(e.naive.lcp.max()) < 10 - 1       # the passes end before pass 9
    assert sum(1 for x in lens if x < 10) > 10 and sum(1 for x in lens if x > 10) > 10
    assert len(e.vals) == 201
    assert len(P["rows_three_tiles_17"].exp.table(5)[0]) > TK + 1


def run_entries_around_the_decode_tile(ctx, flags, mem, lib):
    """tile_kmers - 1, tile_kmers, tile_kmers + 1 selected entries, through the row window and through min_count"""
    c, fm, (T, TK, _) = open_case(ctx, flags, mem, lib, "rows_three_tiles_17")
    with fm:
        e = c.exp
        lo, count, _ = e.table(5)
        assert len(lo) > TK + 1
        for m in (TK - 1, TK, TK + 1):
            info = call(fm, mem, e, 5, 1, rb=0, re=int(lo[m]))
            assert info["n_selected"] == m
            info = call(fm, mem, e, 5, 1, rb=int(lo[7]), re=int(lo[7 + m]))
            assert info["n_selected"] == m
        # min_count on a k with enough repeated k-mers: the window's end trims the selection to the three sizes
        lo, count, _ = e.table(6)
        rep = lo[count >= 2]
        assert len(rep) > TK + 1, len(rep)
        for m in (TK - 1, TK, TK + 1):
            info = call(fm, mem, e, 6, 1, min_count=2, re=int(rep[m]))
            assert info["n_selected"] == m
        info = call(fm, mem, e, 6, 1, min_count=2, max_count=int(count.max()) - 1)
        assert 0 < info["n_selected"] < len(rep)


def run_values_of_k(ctx, flags, mem, lib):
    c, fm, (T, TK, stage) = open_case(ctx, flags, mem, lib, "rows_tile_plus_1")
    with fm:
        e = c.exp
        lo, count, cells = e.table(1)                                   # k = 1: the symbols with their frequencies
        vals, freq = np.unique(c.cells[c.cells != c.cells[-1]], return_counts=True)
        assert np.array_equal(cells.reshape(-1), vals.astype(np.uint64)) and np.array_equal(count, freq.astype(np.uint64))
        call(fm, mem, e, 1, 1, bins=8)
        call(fm, mem, e, 2, 1, bins=8)
        big = stage // (8 * TK) + 3                                     # chunked staging: k * 8 * tile_kmers is above the LDS
        assert big * 8 * TK > stage and big <= e.longest and len(e.table(big)[0]) > TK
        call(fm, mem, e, big, 8)
        call(fm, mem, e, 2 * (stage // (8 * TK)) + 1, 8)                # three chunks, the last one short
        call(fm, mem, e, stage // (2 * TK) + 1, 2)                      # and with 2-byte cells
        info = call(fm, mem, e, e.longest, 1, bins=4)                   # k = the longest string
        assert info["n_distinct"] >= 1
        for k in (e.longest + 1, 10 ** 6, 2 ** 63):                     # longer than every string: no k-mer
            info = call(fm, mem, e, k, 1, bins=4)
            assert info["n_distinct"] == info["n_windows"] == info["n_selected"] == 0


def run_early_distinct(ctx, flags, mem, lib):
    c, fm, _ = open_case(ctx, flags, mem, lib, "early_distinct")
    with fm:
        e = c.exp
        info = call(fm, mem, e, 10, 2, bins=16)
        assert info["passes"] < 9 and info["passes"] + info["length_passes"] == 9, info
        assert 0 < info["n_distinct"] and info["n_windows"] == sum(max(0, len(s) - 9) for s in e.strings)
        call(fm, mem, e, 30, 2, bins=2)
        call(fm, mem, e, 31, 2, bins=2)


def run_one_symbol(ctx, flags, mem, lib):
    c, fm, (T, TK, _) = open_case(ctx, flags, mem, lib, "one_symbol")
    with fm:
        e = c.exp
        for k in (1, 7, 70):
            info = call(fm, mem, e, k, 1, bins=MAX_BINS)
            assert (info["n_distinct"], info["largest_count"]) == (1, 3 * T - k + 1), info
            call(fm, mem, e, k, 1, rb=k, re=k + 1, bins=1)
            call(fm, mem, e, k, 1, rb=k + 1)                            # the head lies in front of the window: an empty table


def run_small(ctx, flags, mem, lib, name):
    c, fm, _ = open_case(ctx, flags, mem, lib, name)
    with fm:
        e = c.exp
        for k in (1, 2, 3, max(e.longest, 1), e.longest + 1):
            info = call(fm, mem, e, k, 8, bins=32)
            call(fm, mem, e, k, 8, min_count=2)
            d = lcp_distinct(fm, k)
            assert d is None or d == info["n_distinct"], (name, k)
        if name == "twice":
            assert all(int(v) % 2 == 0 for k in (1, 2, 3, 9) for v in e.table(k)[1])
        if name == "wide_u64":                                         # values as values; a narrower width is refused, nothing written
            assert int(e.vals.max()) == 2 ** 63 + 11
            m = len(e.table(2)[0])
            for w in (1, 2, 4):
                bufs = [mem.out(m * 2 * w), mem.out(8 * m), mem.out(8 * m)]
                msg = fc.einval(lambda: fm.kmers_raw(2, cell_bytes=w, cells_ptr=bufs[0][1], lo_ptr=bufs[1][1], count_ptr=bufs[2][1], capacity=m))
                assert "does not fit" in msg and all(bool(np.all(mem.get(b) == FILL)) for b, _ in bufs)
                assert fm.kmers_raw(2, cell_bytes=w, lo_ptr=bufs[1][1], capacity=m) == m       # without the cells the width is not looked at
        if name in ("one_empty_string", "empty_strings"):
            assert call(fm, mem, e, 1, 1, bins=3)["n_distinct"] == 0
        if name == "two_bytes":
            call(fm, mem, e, 2, 2)
            call(fm, mem, e, 2, 4)


def run_outputs_and_sizing(ctx, flags, mem, lib):
    """each output alone; capacity 0 without arrays reports the number; one entry short is EINVAL with nothing written"""
    c, fm, _ = open_case(ctx, flags, mem, lib, "rows_tile")
    with fm:
        e = c.exp
        for outs in (("cells",), ("lo",), ("count",), ()):
            call(fm, mem, e, 4, 1, outs=outs, bins=16 if not outs else None)
            call(fm, mem, e, 4, 1, outs=outs, bins=16)
        m = len(e.table(4)[0])
        assert fm.kmers_raw(4) == m                                     # n_kmers_out alone
        L = ctx.L
        bufs = [mem.out(m * 4), mem.out(8 * m), mem.out(8 * m)]
        spec = np.full(16, 7, dtype=np.uint64)
        for which in ((0, 1, 2), (0,), (1,), (2,)):
            p = [C.c_void_p(bufs[i][1]) if i in which else None for i in range(3)]
            got = C.c_uint64(0)
            rc = L.grlbwt_fm_kmers(ctx._h, fm._h, 4, 1, 0, 0, engine.UINT64_MAX, 1, p[0], p[1], p[2], m - 1, C.byref(got),
                                   spec.ctypes.data_as(C.c_void_p), 16)
            assert rc == EINVAL and got.value == m and "GRLBWT" not in L.grlbwt_last_error(ctx._h).decode()
            assert all(bool(np.all(mem.get(b) == FILL)) for b, _ in bufs) and bool(np.all(spec == 7))
            assert fm.kmer_info()["n_selected"] == m                    # the call got as far as counting
        lo, count, cells = fm.kmers(4)                                  # the binding sizes by the idiom
        want = e.table(4)
        assert np.array_equal(lo, want[0]) and np.array_equal(count, want[1]) and np.array_equal(cells.astype(np.uint64), want[2])
        assert cells.dtype == np.uint8 and cells.shape == (m, 4)
        lo, count, cells = fm.kmers(4, min_count=2, rows=(int(want[0][3]), int(want[0][-2])), cells=False)
        sel = select(e, 4, 2, 0, int(want[0][3]), int(want[0][-2]))
        assert cells is None and np.array_equal(lo, sel[0]) and np.array_equal(count, sel[1])
        assert np.array_equal(fm.kmer_spectrum(4, 9), spectrum(e, 4, 9))


def run_spectrum_bins(ctx, flags, mem, lib):
    c, fm, _ = open_case(ctx, flags, mem, lib, "rows_tile_minus_1")
    with fm:
        e = c.exp
        k = 3
        top = int(e.table(k)[1].max())
        assert top > 3
        info = call(fm, mem, e, k, 1, outs=(), bins=1)                  # one bin: the last one, bin 0 = n_distinct
        assert int(spectrum(e, k, 1)[0]) == info["n_distinct"]
        for bins in (2, top + 1, top, MAX_BINS):
            call(fm, mem, e, k, 1, outs=(), bins=bins)
        s = spectrum(e, k, top + 1)
        assert s[0] == 0 and s[top] >= 1 and spectrum(e, k, top)[top - 1] == s[top - 1] + s[top]
        spec = np.full(MAX_BINS + 1, 7, dtype=np.uint64)
        fc.einval(lambda: fm.kmers_raw(k, spectrum=spec))
        fc.einval(lambda: fm.kmers_raw(k, spectrum=spec[:0]))
        assert bool(np.all(spec == 7))


def run_row_windows(ctx, flags, mem, lib):
    """a partition of [0, n) into windows gives tables that concatenate to the whole table"""
    c, fm, (T, TK, _) = open_case(ctx, flags, mem, lib, "rows_three_tiles_17")
    with fm:
        e = c.exp
        cuts = [0, 1, e.n_strings, T - 1, T - 1, T + 64, 2 * T + 5, e.n]         # (an empty window among them)
        total = 0
        for a, b in zip(cuts, cuts[1:]):
            total += call(fm, mem, e, 6, 1, rb=a, re=b, check_count=False)["n_selected"]
        assert total == len(e.table(6)[0])
        call(fm, mem, e, 6, 1, rb=e.n, re=engine.UINT64_MAX, check_count=False)   # clamped to [n, n): empty


def run_refusals(ctx, flags, mem, lib):
    c, fm, _ = open_case(ctx, flags, mem, lib, "rows_tile_minus_1")
    L = ctx.L
    with fm:
        e = c.exp
        m = len(e.table(2)[0])
        bufs = [mem.out(m * 2), mem.out(8 * m), mem.out(8 * m)]
        pc, pl, pn = (b[1] for b in bufs)
        spec = np.full(8, 7, dtype=np.uint64)

        def untouched():
            return all(bool(np.all(mem.get(b) == FILL)) for b, _ in bufs) and bool(np.all(spec == 7))

        fc.einval(lambda: fm.kmers_raw(0, cells_ptr=pc, lo_ptr=pl, count_ptr=pn, capacity=m, spectrum=spec))            # k = 0
        for w in (0, 3, 16):
            fc.einval(lambda: fm.kmers_raw(2, cell_bytes=w, cells_ptr=pc, lo_ptr=pl, count_ptr=pn, capacity=m, spectrum=spec))
        fc.einval(lambda: fm.kmers_raw(2, row_begin=5, row_end=4, lo_ptr=pl, capacity=m, spectrum=spec))
        fc.einval(lambda: fm.kmers_raw(2, row_begin=e.n + 1, lo_ptr=pl, capacity=m, spectrum=spec))                     # above the clamped end
        rc = L.grlbwt_fm_kmers(ctx._h, fm._h, 2, 1, 0, 0, engine.UINT64_MAX, 1, None, None, None, 0, None, None, 0)     # no output at all
        assert rc == EINVAL
        got = C.c_uint64(99)                                                                                            # a null index
        assert L.grlbwt_fm_kmers(ctx._h, None, 2, 1, 0, 0, engine.UINT64_MAX, 1, C.c_void_p(pc), C.c_void_p(pl), C.c_void_p(pn), m,
                                 C.byref(got), spec.ctypes.data_as(C.c_void_p), 8) == EINVAL and got.value == 0
        assert L.grlbwt_fm_kmer_info_get(None, None) == EINVAL
        assert untouched()
    bad = ic.make_image(1, 1, [10, 65], [1, 2])              # not the BWT of a collection: the row of the second A is LF of itself
    keep, img = mem.put(bad)
    with engine.FmIndex(ctx, img, len(bad)) as fm:
        msg = fc.einval(lambda: fm.kmers_raw(3, cells_ptr=pc, lo_ptr=pl, count_ptr=pn, capacity=m, spectrum=spec))
        assert "not the BWT of a collection" in msg and untouched(), msg


def run_index_unchanged(ctx, flags, mem, lib):
    col = fc.COLS["dna"]
    pats = fc.collection_patterns(col)
    blob = fc.image_of(lib, col, flags)
    e = Expected(col.data)
    for kw in ({}, {"locate": True}, {"locate": True, "checkpoints": True, "sample_bits": 3}, {"locate": True, "extract": True}):
        keep, img = mem.put(blob)
        with engine.FmIndex(ctx, img, len(blob), **kw) as fm:
            del keep
            before, counts = fm.info(), fc.count(fm, mem, pats, 1)
            buf, ptr = mem.out(e.n)
            lcp_before = (fm.lcp(0, 1, ptr), mem.body(buf, e.n).tobytes())
            call(fm, mem, e, 3, 1, bins=8)
            call(fm, mem, e, 7, 4, min_count=2)
            assert fm.info() == before and fc.count(fm, mem, pats, 1) == counts, kw
            buf, ptr = mem.out(e.n)
            after = (fm.lcp(0, 1, ptr), mem.body(buf, e.n).tobytes())
            assert lcp_before[1] == after[1] and all(np.array_equal(a, b) for a, b in zip(lcp_before[0], after[0]))


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
        for k in (1, 2, 5):
            try:
                m = fm.kmers_raw(k)
            except engine.GrlbwtError as e:
                assert e.code == EINVAL, e
                refused += 1
                continue
            assert m <= n and fm.kmer_info()["n_selected"] == m
            bufs = [mem.out(m * k * 8), mem.out(8 * m), mem.out(8 * m)]
            spec = np.full(10, 7, dtype=np.uint64)
            assert fm.kmers_raw(k, cell_bytes=8, cells_ptr=bufs[0][1], lo_ptr=bufs[1][1], count_ptr=bufs[2][1], capacity=m, spectrum=spec[:8]) == m
            lo = mem.body(bufs[1][0], 8 * m).view(np.uint64)
            cnt = mem.body(bufs[2][0], 8 * m).view(np.uint64)
            mem.body(bufs[0][0], m * k * 8)
            assert bool(np.all(spec[8:] == 7)) and int(spec[:8].sum()) == fm.kmer_info()["n_distinct"]
            assert bool(np.all(lo[1:] > lo[:-1])) and bool(np.all(lo + cnt <= n)) and bool(np.all(cnt >= 1))
            done += 1
    return done, refused
