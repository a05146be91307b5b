"""Shared by tests/test_fm_lcp_sim.py (serial stand-in) and tests/test_fm_lcp_gpu.py (HIP library): the LCP array and the
suffix-length counts of a collection from its FM index (grlbwt_fm_lcp), against values that share no code with the engine.

  a  for every case the LCP BY DEFINITION: the suffixes of all strings padded into a matrix (the terminator and the padding
     below every cell), np.lexsort with the string's number as the least significant key, neighbouring rows compared
  b  for inputs of at most 2000 cells also a plain Python sort of tuples, whose terminators (-1, string) equal nothing
  c  the rows are those of bcr_check.naive_bcr_symbols: the symbols in front of the sorted suffixes are the decoded image
  d  the distinct k-mers from a brute-force set of windows

The inputs are sized from the tile the library reports (lcp_info()["tile_rows"] of a first tiny call), never from a constant.
Every output buffer has guard bytes behind it; the info of every call is checked against its outputs.  Expected values are
computed once per process and kept.
"""
import ctypes as C
import os

import numpy as np

from grlbwt_amd import engine
from tests import bcr_check as bc
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import merge_cases as mc
from tests import wide_check as wc

EINVAL = -22
DT = fc.DT
FILL = fc.FILL
HERE = os.path.dirname(os.path.abspath(__file__))
ACGT = mc.ACGT
NAMES = ["rows_tile_minus_1", "rows_tile", "rows_tile_plus_1", "rows_three_tiles_17", "one_symbol", "rare_symbol", "twice",
         "one_string", "one_empty_string", "empty_strings", "two_bytes", "wide_u64", "sigma_256"]
PLAIN_NAMES = ["rows_three_tiles_17", "one_symbol", "rare_symbol"]      # the cases the two forms of a pass are compared on


# ------------------------------------------------------------------ expected values
def split(cells):
    """the strings without their terminators"""
    cells = np.asarray(cells)
    ends = np.flatnonzero(cells == cells[-1])
    starts = np.concatenate([[0], ends[:-1] + 1])
    return [cells[a:b] for a, b in zip(starts, ends)]


class Expected:
    """lcp, the symbol in front of every sorted suffix (the BWT) and the suffixes' lengths, by the matrix of (a)"""

    def __init__(self, cells):
        cells = np.asarray(cells)
        self.n = len(cells)
        self.sep = int(cells[-1])
        strings = split(cells)
        self.k = len(strings)
        vals, inv = np.unique(cells, return_inverse=True)
        assert int(vals[0]) == self.sep
        ranks = split(inv.astype(np.int64))                          # cells as ranks >= 1, the terminator's rank is 0
        width = max(len(s) for s in strings) + 1
        M = np.zeros((self.n, width), dtype=np.int64)
        sid = np.zeros(self.n, dtype=np.int64)
        left = np.zeros(self.n, dtype=np.int64)
        slen = np.zeros(self.n, dtype=np.int64)
        at = 0
        for i, r in enumerate(ranks):
            m = len(r)
            for j in range(m + 1):
                M[at, :m - j] = r[j:]
                sid[at], slen[at] = i, m - j
                left[at] = r[j - 1] if j else 0
                at += 1
        order = np.lexsort([sid] + [M[:, c] for c in range(width - 1, -1, -1)])
        M, self.slen = M[order], slen[order]
        self.bwt = vals[left[order]].astype(np.uint64)
        eq = (M[1:] == M[:-1]) & (M[1:] != 0)
        self.lcp = np.concatenate([[0], np.cumprod(eq, axis=1).sum(axis=1)]).astype(np.int64)
        self.strings = ranks
        if self.n <= 2000:
            assert np.array_equal(self.lcp, tuple_lcp(cells)), "the two naive forms disagree"
            assert [int(v) for v in self.bwt] == bc.naive_bcr_symbols(cells)
        self._kmers = {}

    def kmers(self, k):
        """distinct windows of k cells that hold no terminator"""
        if k not in self._kmers:
            seen = set()
            for r in self.strings:
                b = r.tobytes()
                seen.update(b[8 * j:8 * (j + k)] for j in range(len(r) - k + 1))
            self._kmers[k] = len(seen)
        return self._kmers[k]


def tuple_lcp(cells):
    """(b): every suffix as a tuple of (cell, 0) and its terminator (-1, string); sorted; neighbours compared"""
    cells = np.asarray(cells)
    keys = []
    for i, s in enumerate(split(cells)):
        body = [int(v) for v in s]
        keys += [tuple((c, 0) for c in body[j:]) + ((-1, i),) for j in range(len(body) + 1)]
    keys.sort()
    out = [0]
    for a, b in zip(keys, keys[1:]):
        l = 0
        while a[l] == b[l]:
            l += 1
        out.append(l)
    return np.array(out, dtype=np.int64)


# ------------------------------------------------------------------ the cases, sized by the tile T
class Case:
    def __init__(self, name, cells, w):
        self.name, self.cells, self.w = name, np.asarray(cells, dtype=DT[w]), w
        self.n = len(self.cells)
        self._exp = None

    @property
    def exp(self):
        if self._exp is None:
            self._exp = Expected(self.cells)
        return self._exp


def dna(rng, n):
    """a DNA collection of exactly n cells: a few empty strings, a few strings present twice"""
    empty = ACGT[:0]
    first = [ACGT[rng.integers(0, 4, size=int(rng.integers(1, 61)))] for _ in range(3)]
    strs = mc.strings_to(rng, n, ACGT, 1, first=[empty, empty] + first + first)
    order = rng.permutation(len(strs))
    return mc.text([strs[i] for i in order], 10, 1)


def make_cases(T):
    rng = np.random.default_rng(20261020)
    P = []
    for n in (T - 1, T, T + 1, 3 * T + 17):
        P.append(Case("rows_%s" % {T - 1: "tile_minus_1", T: "tile", T + 1: "tile_plus_1"}.get(n, "three_tiles_17"), dna(rng, n), 1))
    P.append(Case("one_symbol", mc.text(mc.strings_to(rng, T + T // 2 + 3, ACGT[:1], 1), 10, 1), 1))
    # 'Z' in front of a suffix that sorts among the first rows and of one that sorts among the last: its two runs lie more than
    # a tile apart, and the second run's first row tests the ranks of everything between them
    z = np.frombuffer(b"Z", dtype=np.uint8)
    rare = [np.concatenate([z, np.repeat(ACGT[:1], 50)]), np.concatenate([z, np.repeat(ACGT[3:], 50)])]
    P.append(Case("rare_symbol", mc.text(mc.strings_to(rng, 2 * T + 9, ACGT, 1, first=rare), 10, 1), 1))
    half = dna(rng, T // 2 + 11)
    P.append(Case("twice", np.concatenate([half, half]), 1))
    P.append(Case("one_string", np.frombuffer(b"ACGT\n", dtype=np.uint8), 1))
    P.append(Case("one_empty_string", np.frombuffer(b"\n", dtype=np.uint8), 1))
    P.append(Case("empty_strings", np.frombuffer(b"\n\n\n\n\n", dtype=np.uint8), 1))
    raw = np.frombuffer(open(os.path.join(HERE, "golden", "test_2bytes_alphabet.txt"), "rb").read(), dtype=np.uint16)
    ends = np.flatnonzero(raw == raw[-1])                               # the golden collection, cut at a string boundary
    P.append(Case("two_bytes", raw[:int(ends[len(ends) // 2]) + 1], 2))
    P.append(Case("wide_u64", wc.collection(rng, 8, 30, 40, 12, 2 ** 30 - 3, 2 ** 63 + 11), 8))
    pool = 1000 + 3 * np.arange(255)                                    # 255 values and the separator
    P.append(Case("sigma_256", mc.text([pool[:60], pool[60:120], pool[120:180], pool[180:240], pool[240:]] + mc.strings_to(rng, 700, pool, 2), 5, 2), 2))
    return P


_cases = {}


def cases(T):
    if T not in _cases:
        _cases[T] = {c.name: c for c in make_cases(T)}
        assert list(_cases[T]) == NAMES
    return _cases[T]


def tile_rows(ctx, mem, lib, flags):
    """the tile of the pass kernel, from a first tiny call"""
    blob = mc.build(lib, flags, np.frombuffer(b"AC\nA\n", dtype=np.uint8), 1)
    keep, p = mem.put(blob)
    with engine.FmIndex(ctx, p, len(blob)) as fm:
        fm.lcp(0, 4, None)
        t = fm.lcp_info()["tile_rows"]
    assert t >= 64 and t % 64 == 0
    return t


# ------------------------------------------------------------------ one call, guarded outputs, info checked
def lcp(fm, mem, n, max_lcp=0, w=4, array=True, hist=True):
    """grlbwt_fm_lcp -> (values or None, rows_at, suffixes_of, info)"""
    buf, ptr = mem.out(n * w)
    ra, su = fm.lcp(max_lcp, w, ptr if array else None, hist)
    if array:
        got = mem.body(buf, n * w).view(DT[w]).astype(np.int64) if w < 8 else mem.body(buf, n * w).view(np.uint64)
    else:
        assert bool(np.all(mem.get(buf) == FILL))
        got = None
    return got, ra, su, fm.lcp_info()


def check(e, got, ra, su, info, max_lcp, w, flags=None):
    """the outputs of one call against the expected values under its cap"""
    lim = 2 ** (8 * w) - 1
    cap = min(max_lcp, lim) if max_lcp else lim
    top = int(e.lcp.max())
    passes = min(top, cap - 1)
    assert (info["n_rows"], info["n_strings"], info["lcp_bytes"]) == (e.n, e.k, w), info
    assert info["cap"] == (engine.UINT64_MAX if w == 8 and not max_lcp else cap), info
    assert (info["passes"], info["n_levels"]) == (passes, passes + 1), (info, top)
    assert info["n_capped"] == int((e.lcp >= cap).sum()), info
    assert info["max_lcp"] == min(top, cap), info
    assert info["scratch_bytes"] >= e.n // 2 and info["tile_rows"] >= 64, info
    if got is not None:
        want = np.minimum(e.lcp, min(cap, 2 ** 62))
        bad = np.flatnonzero(got.astype(np.int64) != want)
        assert not len(bad), (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    if ra is not None:
        assert len(ra) == len(su) == passes + 1
        assert [int(v) for v in ra] == [int((e.lcp == l).sum()) for l in range(passes + 1)]
        assert [int(v) for v in su] == [int((e.slen == l).sum()) for l in range(passes + 1)]
        assert int(ra.sum()) == e.n - info["n_capped"] and int(su[0]) == e.k


def image(lib, flags, c):
    blob = mc.build(lib, flags, c.cells, c.w)
    assert np.array_equal(mc.decode(blob), c.exp.bwt), c.name          # (c): the rows are the sorted suffixes
    return blob


def run_case(ctx, flags, mem, lib, name):
    """cases 1 to 6: the array, the histograms and the k-mer counts of one collection"""
    c = cases(tile_rows(ctx, mem, lib, flags))[name]
    e = c.exp
    blob = image(lib, flags, c)
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob)) as fm:
        del keep
        got, ra, su, info = lcp(fm, mem, e.n)
        check(e, got, ra, su, info, 0, 4)
        kmers = engine.FmIndex.distinct_kmers(ra, su)
        assert len(kmers) == len(ra) + 1
        for k in range(1, len(ra) + 1):
            assert kmers[k] == e.kmers(k) == engine.FmIndex.distinct_kmers(ra, su, k), (name, k)
        for k in (0, len(ra) + 1):
            try:
                engine.FmIndex.distinct_kmers(ra, su, k)
                raise AssertionError("k = %d was accepted" % k)
            except ValueError:
                pass
    return info


def run_sizes_follow_the_tile(ctx, flags, mem, lib):
    T = tile_rows(ctx, mem, lib, flags)
    P = cases(T)
    assert [P[n].n for n in NAMES[:4]] == [T - 1, T, T + 1, 3 * T + 17]
    for n in NAMES[:4]:
        s = split(P[n].cells)
        assert sum(1 for x in s if not len(x)) >= 2
        assert len(set(x.tobytes() for x in s)) <= len(s) - 3
    e = P["one_symbol"].exp
    assert e.n > T and len(np.unique(P["one_symbol"].cells)) == 2
    runs = bc.rle([int(v) for v in e.bwt])
    assert max(l for _, l in runs) > 64                                 # a run that crosses words
    e = P["rare_symbol"].exp
    rows = np.flatnonzero(e.bwt == np.uint64(ord("Z")))
    assert len(rows) == 2 and rows[1] - rows[0] > T, rows
    e = P["twice"].exp
    longest = max(len(s) for s in split(P["twice"].cells))
    assert int(e.lcp.max()) == longest and bool(np.all(e.lcp <= e.slen))            # full lengths, never more
    assert int(((e.lcp == e.slen) & (e.slen > 0)).sum()) >= (e.n - e.k) // 2         # every suffix has a twin
    assert P["empty_strings"].exp.n == P["empty_strings"].exp.k == 5
    assert len(np.unique(P["sigma_256"].cells)) == 256 and int(P["wide_u64"].cells.max()) == 2 ** 63 + 11
    assert int(P["one_string"].exp.lcp.max()) == 0


def run_foreign(ctx, flags, mem, lib):
    """case 6, the last: one image in another encoding -- empty records, split runs, other widths -- has the same LCP"""
    c = cases(tile_rows(ctx, mem, lib, flags))["rows_tile_plus_1"]
    e = c.exp
    blob = image(lib, flags, c)
    cut = mc.split_runs(ctx, mem, blob, 2, 7)
    _, _, sym, ln = bc.parse_rl_bwt(cut)
    assert int((ln == 0).sum()) > 0 and not bc.runs_are_maximal(sym) and len(cut) != len(blob)
    _, _, sym, ln = bc.parse_rl_bwt(blob)
    for other in (cut, ic.make_image(8, 8, sym, ln)):
        keep, img = mem.put(other)
        with engine.FmIndex(ctx, img, len(other)) as fm:
            got, ra, su, info = lcp(fm, mem, e.n)
            check(e, got, ra, su, info, 0, 4)


def run_caps(ctx, flags, mem, lib):
    """case 7: max_lcp 1, 2, 7; the four widths; a single-letter pair that saturates one byte"""
    c = cases(tile_rows(ctx, mem, lib, flags))["rows_tile_plus_1"]
    e = c.exp
    assert int(e.lcp.max()) > 7
    blob = image(lib, flags, c)
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob)) as fm:
        for cap in (1, 2, 7):
            got, ra, su, info = lcp(fm, mem, e.n, cap, 4)
            check(e, got, ra, su, info, cap, 4)
            assert info["n_capped"] > 0 and int(got.max()) == cap
        for w in (1, 2, 4, 8):
            got, ra, su, info = lcp(fm, mem, e.n, 0, w)
            check(e, got, ra, su, info, 0, w)
            got, ra, su, info = lcp(fm, mem, e.n, 7, w)
            check(e, got, ra, su, info, 7, w)
    one = np.concatenate([np.repeat(ACGT[:1], 300), [10]]).astype(np.uint8)
    c = Case("saturating", np.concatenate([one, one]), 1)
    e = c.exp
    assert int(e.lcp.max()) == 300
    blob = image(lib, flags, c)
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob)) as fm:
        got, ra, su, info = lcp(fm, mem, e.n, 0, 1)
        check(e, got, ra, su, info, 0, 1)
        assert (info["passes"], info["cap"], int(got.max()), info["n_capped"]) == (254, 255, 255, int((e.lcp >= 255).sum()))
        got, ra, su, info = lcp(fm, mem, e.n, 0, 2)
        check(e, got, ra, su, info, 0, 2)
        assert info["passes"] == 300


def run_outputs_are_independent(ctx, flags, mem, lib):
    """case 8: without the array the same histograms, without the histograms the same array"""
    c = cases(tile_rows(ctx, mem, lib, flags))["rows_three_tiles_17"]
    e = c.exp
    blob = image(lib, flags, c)
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob)) as fm:
        for cap in (0, 7):
            got, ra, su, info = lcp(fm, mem, e.n, cap, 2)
            check(e, got, ra, su, info, cap, 2)
            none, ra2, su2, info2 = lcp(fm, mem, e.n, cap, 2, array=False)
            check(e, none, ra2, su2, info2, cap, 2)
            assert np.array_equal(ra, ra2) and np.array_equal(su, su2) and info == info2
            got3, ra3, su3, info3 = lcp(fm, mem, e.n, cap, 2, hist=False)
            check(e, got3, ra3, su3, info3, cap, 2)
            assert ra3 is None and su3 is None and np.array_equal(got, got3) and info == info3


def run_sizing_idiom(ctx, flags, mem, lib, monkeypatch):
    """FmIndex.lcp with histograms first sized too small: the refusal's number of levels sizes the second call"""
    c = cases(tile_rows(ctx, mem, lib, flags))["rows_tile"]
    e = c.exp
    blob = image(lib, flags, c)
    keep, img = mem.put(blob)
    monkeypatch.setattr(engine.FmIndex, "LCP_HIST_FIRST", 2)
    assert int(e.lcp.max()) + 1 > 2
    with engine.FmIndex(ctx, img, len(blob)) as fm:
        for array in (True, False):
            got, ra, su, info = lcp(fm, mem, e.n, 0, 2, array=array)
            check(e, got, ra, su, info, 0, 2)


def run_index_unchanged(ctx, flags, mem, lib):
    """case 9: index_bytes and a count batch, before and after, with and without the locate structures and checkpoints"""
    col = fc.COLS["dna"]
    pats = fc.collection_patterns(col)
    blob = fc.image_of(lib, col, flags)
    e = Case("dna", col.data, 1).exp
    for kw in ({}, {"locate": True}, {"locate": True, "checkpoints": True, "sample_bits": 3}, {"locate": True, "extract": True}):
        keep, img = mem.put(blob)
        with engine.FmIndex(ctx, img, len(blob), **kw) as fm:
            del keep
            before, counts = fm.info(), fc.count(fm, mem, pats, 1)
            got, ra, su, info = lcp(fm, mem, e.n, 0, 1)
            check(e, got, ra, su, info, 0, 1)
            got, ra, su, info = lcp(fm, mem, e.n, 5, 8)
            check(e, got, ra, su, info, 5, 8)
            assert fm.info() == before and fc.count(fm, mem, pats, 1) == counts, kw
            if kw.get("locate"):
                fc.dna_rows(fm, mem, col)


def run_refusals(ctx, flags, mem, lib):
    """case 10"""
    c = cases(tile_rows(ctx, mem, lib, flags))["rows_tile_minus_1"]
    e = c.exp
    blob = image(lib, flags, c)
    keep, img = mem.put(blob)
    L = ctx.L
    with engine.FmIndex(ctx, img, len(blob)) as fm:
        buf, ptr = mem.out(4 * e.n)
        levels = int(e.lcp.max()) + 1
        ra = np.full(levels + 2, 7, dtype=np.uint64)
        su = np.full(levels + 2, 7, dtype=np.uint64)
        pra, psu = ra.ctypes.data_as(C.c_void_p), su.ctypes.data_as(C.c_void_p)

        def untouched():
            return bool(np.all(mem.get(buf) == FILL)) and bool(np.all(ra == 7)) and bool(np.all(su == 7))

        fc.einval(lambda: fm.lcp(0, 3, ptr))                         # a bad width
        fc.einval(lambda: fm.lcp(0, 0, ptr))
        fc.einval(lambda: fm.lcp(0, 4, None, want_hist=False))       # no output at all
        assert untouched()
        got = C.c_uint64(99)                                          # a null index
        assert L.grlbwt_fm_lcp(ctx._h, None, 0, 4, ptr, pra, psu, levels, C.byref(got)) == EINVAL and got.value == 0
        assert L.grlbwt_fm_lcp_info_get(None, None) == EINVAL
        assert untouched()
        # histograms one level too short, with and without the array: the code, the number of levels, nothing written
        for p in (ptr, None):
            for which in ((pra, psu), (pra, None), (None, psu)):
                got = C.c_uint64(0)
                assert L.grlbwt_fm_lcp(ctx._h, fm._h, 0, 4, p, which[0], which[1], levels - 1, C.byref(got)) == EINVAL
                assert got.value == levels and "GRLBWT" not in L.grlbwt_last_error(ctx._h).decode()
                assert untouched()
        got = C.c_uint64(0)                                           # the reported capacity suffices
        assert L.grlbwt_fm_lcp(ctx._h, fm._h, 0, 4, ptr, pra, psu, levels, C.byref(got)) == 0 and got.value == levels
        check(e, mem.body(buf, 4 * e.n).view(np.uint32), ra[:levels], su[:levels], fm.lcp_info(), 0, 4)
        assert bool(np.all(ra[levels:] == 7)) and bool(np.all(su[levels:] == 7))
    # not the BWT of a collection: the row of the second A is LF of itself
    bad = ic.make_image(1, 1, [10, 65], [1, 2])
    keep, img = mem.put(bad)
    with engine.FmIndex(ctx, img, len(bad)) as fm:
        msg = fc.einval(lambda: fm.lcp(0, 4, None))
        assert "not the BWT of a collection" in msg, msg
