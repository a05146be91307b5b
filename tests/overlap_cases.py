"""Shared by tests/test_fm_overlaps_sim.py (serial stand-in) and tests/test_fm_overlaps_gpu.py (HIP library): the suffix-prefix
overlaps of queries with the strings of a collection (grlbwt_fm_overlaps, grlbwt_fm_overlaps_of, grlbwt_fm_overlap_targets),
against values from the text alone: the whole strings sorted by (cells, number) are the prefix ranks, and for every query and
every L the strings that start with the query's last L cells are found by a prefix test.  Nothing of the engine is involved.

  A  a collection made for overlaps (reads of 30 cells at stride 7 from a random genome of 400 cells, shuffled; 6 duplicates; 4
     reads that are proper prefixes of others; 2 empty strings; one periodic read; one read with a symbol of its own) and
     fm_cases.COLS identical / two_bytes / wide_u64: both calls at min_len 1 / 8, max_len 0 / 16, with and without PROPER;
     overlaps_of(all ids) against overlaps(the strings' own cells); the lo / hi columns against fm_cases.count of the suffix.
  B  targets: every hit list of A expanded; a collection of 2 * tile_entries + 70 one-cell strings with synthetic ranges around
     the tile boundaries.
  C  launch shapes: 0, 1, 63, 64, 65 and 5000 queries, empty ones between them, off[0] = 7.
  D  refusals and the sizing calls: nothing is written.
  E  foreign images (tests/image_cases.py): the same definition on the RECORDS (fm_cases.RecordIndex).

Every output buffer has guard bytes behind it (fm_cases.Mem); the info of every call is checked against its outputs.  The
brute-force values are computed once per process and kept.
"""
import numpy as np
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import match_cases as mc

DT = fc.DT
PROPER = engine.FM_OVERLAP_PROPER if hasattr(engine, "FM_OVERLAP_PROPER") else 1
SHAPES = (0, 1, 63, 64, 65, 5000)
SEED = 20261020
CONFIGS = [(mn, mx, fl) for mn in (1, 8) for mx in (0, 16) for fl in (0, PROPER)]
NAMES = ["reads", "identical", "two_bytes", "wide_u64"]
A, C_, G, T, N_, NL = 65, 67, 71, 84, 78, 10


# ------------------------------------------------------------------ A: the collection made for overlaps
def make_reads():
    rng = np.random.default_rng(SEED)
    acgt = np.array([A, C_, G, T], dtype=np.uint8)
    genome = acgt[rng.integers(0, 4, size=400)]
    reads = [genome[a:a + 30].copy() for a in range(0, 371, 7)]
    n0 = len(reads)
    reads += [reads[i].copy() for i in (4, 4, 11, 20, 33, 47)]             # 6 duplicates: read 4 is there three times
    reads += [reads[i][:l].copy() for i, l in ((2, 5), (9, 12), (17, 20), (30, 29))]      # proper prefixes of others
    reads += [acgt[:0], acgt[:0]]
    reads.append(np.array([A, C_] * 15, dtype=np.uint8))                  # a self-border at every even length
    odd = reads[25].copy()
    odd[25] = N_                                                          # a symbol no other read has
    reads.append(odd)
    order = rng.permutation(len(reads))
    data = np.concatenate([np.concatenate([reads[i], [NL]]) for i in order]).astype(np.uint8)
    return fc.Collection("reads", data, 1), genome, n0


READS, GENOME, N_STRIDE = make_reads()


def collection(name):
    return READS if name == "reads" else fc.COLS[name]


def queries_of(col):
    """every string of the collection, in number order (what overlaps_of answers for all ids), then: for the reads 30-cell windows
    of the genome at every offset 0 .. 40; a string with a non-symbol and one with the separator 5 cells from the end; a string
    with a cell in front of it that is no symbol; a pattern longer than any string; the separator alone; a non-symbol alone"""
    qs = [[int(v) for v in s] for s in col.strings]
    full = [q for q in qs if len(q) >= 8]
    bad = mc.non_symbol(col)
    if col.name == "reads":
        qs += [[int(v) for v in GENOME[a:a + 30]] for a in range(41)]
    a, b = list(full[0]), list(full[len(full) // 2])
    a[len(a) - 5] = bad
    b[len(b) - 5] = col.sep
    qs += [a, b, [bad] + full[1], full[2] + full[3] + full[2], [col.sep], [bad]]
    return qs


class Expected:
    """rank -> string number, and per query the hits (L, tlo, thi) at min_len 1 without a cap or PROPER: every other setting is
    a filter of that list"""

    def __init__(self, name):
        self.col = col = collection(name)
        self.strs = [tuple(int(v) for v in s) for s in col.strings]
        self.order = sorted(range(len(self.strs)), key=lambda i: (self.strs[i], i))
        self.sorted = [self.strs[i] for i in self.order]
        self.symbols = set(int(v) for v in np.unique(col.data))
        self.queries = queries_of(col)
        self.full = [self.hits_of(q) for q in self.queries]

    def hits_of(self, q):
        m, out = len(q), []
        for L in range(1, m + 1):
            c = q[m - L]
            if c == self.col.sep or c not in self.symbols:
                break
            suf = tuple(q[m - L:])
            at = [t for t, s in enumerate(self.sorted) if s[:L] == suf]      # the prefix test
            if at:
                assert at == list(range(at[0], at[-1] + 1)), (q, L)
                out.append((L, at[0], at[-1] + 1))
        return out

    def want(self, idx, min_len, max_len, flags):
        out = []
        for i in idx:
            m = len(self.queries[i])
            out.append([h for h in self.full[i]
                        if h[0] >= max(min_len, 1) and (not max_len or h[0] <= max_len) and not (flags & PROPER and h[0] == m)])
        return out

    def strings_of(self, tlo, thi):
        return self.order[tlo:thi]


_expected = {}


def expected(name):
    if name not in _expected:
        _expected[name] = Expected(name)
    return _expected[name]


def not_vacuous(ex):
    """on the brute-force values alone, for the reads"""
    k = len(ex.strs)
    lens = set(h[0] for hs in ex.full for h in hs)
    assert set(range(2, 31)) <= lens, sorted(set(range(2, 31)) - lens)
    assert max(h[2] - h[1] for hs in ex.full for h in hs) >= 3
    idx = list(range(len(ex.queries)))
    proper = ex.want(idx[:k], 1, 0, PROPER)
    border = [i for i in range(k) if any(ex.order[t] == i for h in proper[i] for t in range(h[1], h[2]))]
    assert border, "no string overlaps itself with a proper suffix"
    at8 = ex.want(idx, 8, 0, 0)
    none = [i for i in idx if len(ex.queries[i]) >= 8 and not at8[i]]
    assert none, "every query of 8 cells or more has a hit at min_len 8"
    return sorted(lens), border, none


# ------------------------------------------------------------------ the calls on a batch, guarded outputs, info checked
def _call(fm, kind, ptrs, n, w, min_len, max_len, flags, hoff, ln, tlo, thi, cap, lo, hi):
    if kind == "cells":
        return fm.overlaps(ptrs[0], w, ptrs[1], n, min_len, max_len, flags, hoff, ln, tlo, thi, cap, lo, hi)
    return fm.overlaps_of(ptrs[0], n, min_len, max_len, flags, hoff, ln, tlo, thi, cap, lo, hi)


def overlaps(fm, mem, kind, arg, w, min_len, max_len, flags, rows=True, lead=0, capacity=None):
    """grlbwt_fm_overlaps (kind "cells": arg = patterns) or grlbwt_fm_overlaps_of (kind "ids": arg = string numbers) -> per query
    the list of (L, tlo, thi, lo, hi) in the order written (lo and hi None without the row arrays); the info of the call.
    capacity None: what the sizing call reports."""
    n = len(arg)
    if kind == "cells":
        keep, pc, po, nc = mc.put_batch(mem, arg, w, lead)
        ptrs = (pc, po)
    else:
        keep, pi = mem.put(np.asarray(arg, dtype=np.uint64).tobytes())
        ptrs, nc = (pi,), None
    if capacity is None:
        try:
            cap = _call(fm, kind, ptrs, n, w, min_len, max_len, flags, None, None, None, None, 0, None, None)
        except engine.GrlbwtError as e:
            assert e.code == fc.EINVAL, e
            cap = e.n_hits
    else:
        cap = capacity
    hoff, ph = mem.out(8 * (n + 1))
    cols = [mem.out(8 * cap) for _ in range(5)]
    got = _call(fm, kind, ptrs, n, w, min_len, max_len, flags, ph, cols[0][1], cols[1][1], cols[2][1], cap,
                cols[3][1] if rows else None, cols[4][1] if rows else None)
    assert got <= cap
    H = mem.body(hoff, 8 * (n + 1)).view(np.uint64)
    assert int(H[0]) == 0 and int(H[-1]) == got and bool(np.all(H[1:] >= H[:-1])), H[:8]
    for b, _ in cols[:3 + 2 * rows]:
        assert bool(np.all(mem.get(b)[8 * got:] == fc.FILL)), "entries behind the last one were written"
    for b, _ in cols[3 + 2 * rows:]:
        assert bool(np.all(mem.get(b) == fc.FILL)), "a row array that was not given was written"
    ln, tlo, thi, lo, hi = [mem.body(b, 8 * cap).view(np.uint64)[:got] for b, _ in cols]
    out = []
    for i in range(n):
        out.append([(int(ln[j]), int(tlo[j]), int(thi[j]), int(lo[j]) if rows else None, int(hi[j]) if rows else None)
                    for j in range(int(H[i]), int(H[i + 1]))])
    info = fm.overlap_info()
    assert (info["n_patterns"], info["n_hits"], info["n_ranges"], info["n_entries"]) == (n, got, 0, 0), info
    assert info["n_targets"] == int((thi - tlo).sum(dtype=np.uint64)) and info["longest"] == (int(ln.max()) if got else 0), info
    assert info["tile_entries"] >= 64, info
    assert info["n_cells"] >= sum(max(h[0] for h in hs) for hs in out if hs), info           # a hit at L took L query steps at least
    if nc is not None:
        assert info["n_cells"] <= nc, (info, nc)
    assert info["n_cells"] + got <= info["steps"] <= 2 * info["n_cells"], info               # a hit took a separator step
    return out, info


def targets(fm, mem, ranges, with_range=True, capacity=None):
    """grlbwt_fm_overlap_targets -> per range the list of string numbers; the info"""
    n = len(ranges)
    kl, pl = mem.put(np.array([r[0] for r in ranges], dtype=np.uint64).tobytes())
    kh, ph = mem.put(np.array([r[1] for r in ranges], dtype=np.uint64).tobytes())
    if capacity is None:
        try:
            cap = fm.overlap_targets(pl, ph, n, None, None, 0)
        except engine.GrlbwtError as e:
            assert e.code == fc.EINVAL, e
            cap = e.n_entries
        assert cap == sum(b - a for a, b in ranges)
    else:
        cap = capacity
    eoff, pe = mem.out(8 * (n + 1))
    st, ps = mem.out(8 * cap)
    rg, pr = mem.out(8 * cap)
    got = fm.overlap_targets(pl, ph, n, pe, ps, cap, pr if with_range else None)
    assert got == sum(b - a for a, b in ranges) <= cap
    E = mem.body(eoff, 8 * (n + 1)).view(np.uint64)
    assert [int(v) for v in E] == [0] + [int(v) for v in np.cumsum([b - a for a, b in ranges], dtype=np.uint64)], E[:8]
    assert bool(np.all(mem.get(st)[8 * got:] == fc.FILL)), "entries behind the last one were written"
    S = mem.body(st, 8 * cap).view(np.uint64)[:got]
    if with_range:
        assert bool(np.all(mem.get(rg)[8 * got:] == fc.FILL))
        Rg = mem.body(rg, 8 * cap).view(np.uint64)[:got]
        assert np.array_equal(Rg, np.repeat(np.arange(n, dtype=np.uint64), [b - a for a, b in ranges]))
    else:
        assert bool(np.all(mem.get(rg) == fc.FILL))
    info = fm.overlap_info()
    assert (info["n_ranges"], info["n_entries"], info["n_patterns"], info["n_hits"], info["steps"]) == (n, got, 0, 0, 0), info
    return [[int(v) for v in S[int(E[r]):int(E[r + 1])]] for r in range(n)], info


def with_rows(ex, fm, mem, want):
    """the expected entries with the rows grlbwt_fm_count answers for each suffix"""
    w = ex.col.w
    sufs = {}
    for i, hs in want:
        q = ex.queries[i]
        for L, _, _ in hs:
            sufs[tuple(q[len(q) - L:])] = None
    keys = list(sufs)
    for k, r in zip(keys, fc.count(fm, mem, [list(k) for k in keys], w)):
        assert r[0] < r[1], k
        sufs[k] = r
    return [[(L, a, b) + sufs[tuple(ex.queries[i][len(ex.queries[i]) - L:])] for L, a, b in hs] for i, hs in want]


def run_collection(ctx, flags, mem, lib, name):
    """A and the first half of B on one collection"""
    ex = expected(name)
    col = ex.col
    k = len(ex.strs)
    blob = fc.image_of(lib, col, flags)
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob), locate=True) as fm, engine.FmIndex(ctx, img, len(blob)) as plain:
        del keep
        info = fm.info()
        assert info["n_strings"] == k
        tile = fm.overlap_info()["tile_entries"]
        assert tile >= 64
        idx = list(range(len(ex.queries)))
        for min_len, max_len, fl in CONFIGS:
            want = ex.want(idx, min_len, max_len, fl)
            full = with_rows(ex, fm, mem, list(zip(idx, want)))
            got, _ = overlaps(fm, mem, "cells", ex.queries, col.w, min_len, max_len, fl)
            bad = [(i, ex.queries[i][:8], g[:3], e[:3]) for i, (g, e) in enumerate(zip(got, full)) if g != e]
            assert not bad, (name, min_len, max_len, fl, bad[:3])
            of, _ = overlaps(fm, mem, "ids", list(range(k)), col.w, min_len, max_len, fl)
            assert of == got[:k], (name, min_len, max_len, fl, [i for i in range(k) if of[i] != got[i]][:5])
            norows, _ = overlaps(plain, mem, "cells", ex.queries, col.w, min_len, max_len, fl, rows=False)     # an index without locate
            assert [[h[:3] for h in hs] for hs in norows] == want, (name, min_len, max_len, fl)
            if col.w < 8 and (min_len, max_len) == (1, 0):                   # the same patterns as wider cells
                wide, _ = overlaps(fm, mem, "cells", ex.queries, 8, min_len, max_len, fl)
                assert wide == got, (name, fl)
            # B: the hit lists expanded
            ranges = [(h[1], h[2]) for hs in got for h in hs]
            strs, tinfo = targets(fm, mem, ranges, with_range=fl == 0)
            assert strs == [ex.strings_of(a, b) for a, b in ranges], (name, min_len, max_len, fl)
            assert tinfo["tile_entries"] == tile
        if name == "identical":
            whole = ex.want([0], 1, 0, 0)[0][-1]
            assert whole == (40, 0, 64) and ex.strings_of(0, 64) == list(range(64))      # 64 equal strings: a range of 64 in number order


# ------------------------------------------------------------------ B: synthetic ranges around the tile boundaries
def run_tile_ranges(ctx, flags, mem, lib):
    ex0 = expected("reads")
    blob0 = fc.image_of(lib, ex0.col, flags)
    keep, img = mem.put(blob0)
    with engine.FmIndex(ctx, img, len(blob0), locate=True) as fm:
        tile = fm.overlap_info()["tile_entries"]
    n = 2 * tile + 70
    rng = np.random.default_rng(SEED + tile)
    cells = np.array([A, C_, G, T], dtype=np.uint8)[rng.integers(0, 4, size=n)]
    data = np.empty(2 * n, dtype=np.uint8)
    data[0::2] = cells
    data[1::2] = NL
    col = fc.Collection("one_cell_%d" % tile, data, 1)
    order = sorted(range(n), key=lambda i: (int(cells[i]), i))
    sizes = [0, tile - 1, 1, 1, tile - 1, tile, 0, tile, tile + 1, 2 * tile + 3, 0, 1, 0]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    assert {tile - 1, tile, tile + 1} <= set(int(s) for s in starts)          # a range starts on, one before and one behind a boundary
    assert sizes[5] == tile and starts[5] % tile == 0 and sizes[6] == 0 and sizes[7] == tile      # an empty range between two full tiles
    ranges = []
    for i, s in enumerate(sizes):
        a = (7 * i + 3) % (n - s + 1)
        ranges.append((a, a + s))
    blob = fc.image_of(lib, col, flags)
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob), locate=True) as fm:
        assert fm.info()["n_strings"] == n
        for with_range in (True, False):
            strs, info = targets(fm, mem, ranges, with_range)
            assert strs == [order[a:b] for a, b in ranges]
            assert info["tile_entries"] == tile and info["n_entries"] == sum(sizes)
        strs, _ = targets(fm, mem, [(0, n)])                                 # the whole table
        assert strs == [order]
        strs, _ = targets(fm, mem, [(5, 5), (n, n), (0, 0)])                # nothing but empty ranges
        assert strs == [[], [], []]
        strs, _ = targets(fm, mem, [])
        assert strs == []


# ------------------------------------------------------------------ C: launch shapes
def run_shapes(ctx, flags, mem, lib, on_info=None):
    """every shape: n queries, every fourth one empty, 7 cells in front of the first; the same numbers as ids with repeats;
    on_info(n, info) sees the launch counters of both"""
    ex = expected("reads")
    k = len(ex.strs)
    pool = [i for i in range(len(ex.queries)) if len(ex.queries[i]) >= 8][:48]
    want = ex.want(pool, 8, 0, 0)
    assert sum(1 for hs in want if len(hs) >= 2) >= 10
    by_id = ex.want(list(range(k)), 8, 0, PROPER)
    blob = fc.image_of(lib, ex.col, flags)
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob), locate=True) as fm:
        for n in SHAPES:
            pats, exp = [], []
            for i in range(n):
                if i % 4 == 3:
                    pats.append([])
                    exp.append([])
                else:
                    pats.append(ex.queries[pool[i % len(pool)]])
                    exp.append(want[i % len(pool)])
            got, info = overlaps(fm, mem, "cells", pats, 1, 8, 0, 0, rows=False, lead=7)
            assert [[h[:3] for h in hs] for hs in got] == exp, (n, [i for i, (g, e) in enumerate(zip(got, exp)) if [h[:3] for h in g] != e][:5])
            if on_info:
                on_info(n, info)
            ids = [(i * 13) % k for i in range(n)]
            got, info = overlaps(fm, mem, "ids", ids, 1, 8, 0, PROPER, rows=False)
            assert [[h[:3] for h in hs] for hs in got] == [by_id[i] for i in ids], n
            if on_info:
                on_info(n, info)


# ------------------------------------------------------------------ D: refusals
def run_refusals(ctx, flags, mem, lib):
    ex = expected("reads")
    k = len(ex.strs)
    pats = ex.queries[:40]
    n = len(pats)
    want = ex.want(list(range(n)), 8, 0, 0)
    total = sum(len(hs) for hs in want)
    assert total >= 2
    n_targets = sum(h[2] - h[1] for hs in want for h in hs)
    blob = fc.image_of(lib, ex.col, flags)
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob), locate=True) as fm, engine.FmIndex(ctx, img, len(blob)) as plain:
        keepb, pc, po, _ = mc.put_batch(mem, pats, 1)
        ids = np.arange(n, dtype=np.uint64)
        ki, pi = mem.put(ids.tobytes())
        ids_bad = ids.copy()
        ids_bad[17] = k
        ids_bad[30] = k + 5
        kb, pib = mem.put(ids_bad.tobytes())
        outs = [mem.out(8 * (n + 1))] + [mem.out(8 * total) for _ in range(5)]
        ptr = [p for _, p in outs]

        def untouched(bufs=outs):
            return all(bool(np.all(mem.get(b) == fc.FILL)) for b, _ in bufs)

        def cells(f=fm, cells_=pc, w=1, off=po, np_=n, fl=0, hoff=ptr[0], lo=ptr[4], hi=ptr[5], cap=total):
            return f.overlaps(cells_, w, off, np_, 8, 0, fl, hoff, ptr[1], ptr[2], ptr[3], cap, lo, hi)

        def of(f=fm, ids_=pi, fl=0, hoff=ptr[0], lo=ptr[4], hi=ptr[5], cap=total):
            return f.overlaps_of(ids_, n, 8, 0, fl, hoff, ptr[1], ptr[2], ptr[3], cap, lo, hi)

        kd, pd = mem.put(np.array([0, 2, 1, 3], dtype=np.uint64).tobytes())
        for bad in (lambda: cells(fl=2), lambda: cells(fl=PROPER | 0x80000000), lambda: of(fl=4),      # unknown flags
                    lambda: cells(hi=None), lambda: cells(lo=None), lambda: of(hi=None), lambda: of(lo=None),      # one of lo / hi alone
                    lambda: cells(w=3), lambda: cells(w=0),                   # a bad width
                    lambda: cells(off=pd, np_=3),                             # decreasing offsets
                    lambda: cells(cells_=None),                               # cells missing while there are some
                    lambda: cells(hoff=None), lambda: of(hoff=None),          # no hit offsets
                    lambda: of(f=plain)):                                     # an index without locate
            fc.einval(bad)
            assert untouched()
        msg = fc.einval(lambda: of(ids_=pib))                                # an id out of range: the first such entry is named
        assert "entry 17 " in msg, msg
        assert untouched()
        L = ctx.L                                                            # a null index
        got = engine.C.c_uint64(7)
        assert L.grlbwt_fm_overlaps(ctx._h, None, pc, 1, po, n, 8, 0, 0, ptr[0], ptr[1], ptr[2], ptr[3], None, None, total, engine.C.byref(got)) == fc.EINVAL
        assert got.value == 0
        assert L.grlbwt_fm_overlap_info_get(None, None) == fc.EINVAL
        assert untouched()
        # capacity 0 sizing and one entry too few: the code, the number, nothing written
        for call in (cells, of):
            with pytest.raises(engine.GrlbwtError) as e:
                call(cap=total - 1)
            assert e.value.code == fc.EINVAL and e.value.n_hits == total, (e.value, total)
            assert "GRLBWT" not in str(e.value)
            assert untouched()
            with pytest.raises(engine.GrlbwtError) as e:
                call(hoff=None, lo=None, hi=None, cap=0)
            assert e.value.code == fc.EINVAL and e.value.n_hits == total
            assert untouched()
        assert cells() == total and not untouched()
        # targets
        ranges = [(h[1], h[2]) for hs in want for h in hs]
        nr = len(ranges)
        lo_ = np.array([r[0] for r in ranges], dtype=np.uint64)
        hi_ = np.array([r[1] for r in ranges], dtype=np.uint64)
        kl, pl = mem.put(lo_.tobytes())
        kh, ph = mem.put(hi_.tobytes())
        touts = [mem.out(8 * (nr + 1)), mem.out(8 * n_targets), mem.out(8 * n_targets)]
        tp = [p for _, p in touts]

        def tg(f=fm, lo=pl, hi=ph, eoff=tp[0], cap=n_targets):
            return f.overlap_targets(lo, hi, nr, eoff, tp[1], cap, tp[2])

        over = hi_.copy()
        over[nr // 2] = k + 1                                               # thi > n_strings
        ko, pov = mem.put(over.tobytes())
        swapped = lo_.copy()
        swapped[3] = hi_[3] + 1                                             # tlo > thi
        ks, psw = mem.put(swapped.tobytes())
        fc.einval(lambda: tg(f=plain))
        assert untouched(touts)
        msg = fc.einval(lambda: tg(hi=pov))
        assert "range %d " % (nr // 2) in msg, msg
        assert untouched(touts)
        msg = fc.einval(lambda: tg(lo=psw))
        assert "range 3 " in msg, msg
        assert untouched(touts)
        fc.einval(lambda: tg(eoff=None))
        assert untouched(touts)
        for cap in (n_targets - 1, 0):
            with pytest.raises(engine.GrlbwtError) as e:
                tg(cap=cap)
            assert e.value.code == fc.EINVAL and e.value.n_entries == n_targets, (e.value, n_targets)
            assert untouched(touts)
        assert tg() == n_targets and not untouched(touts)


# ------------------------------------------------------------------ E: by definition, on the records of a foreign image
def search_records(ri, q, min_len, max_len, flags):
    out = []
    if not ri.present or not ri.n:
        return out
    sep = ri.present[0]
    lo, hi, m = 0, ri.n, len(q)
    for L in range(1, m + 1):
        c = q[m - L]
        if c == sep or c not in ri.per:
            break
        lo, hi = ri.C[c] + ri.rank(c, lo), ri.C[c] + ri.rank(c, hi)
        if lo >= hi:
            break
        if L >= max(min_len, 1) and not (flags & PROPER and L == m):
            a, b = ri.rank(sep, lo), ri.rank(sep, hi)
            if a < b:
                out.append((L, a, b, lo, hi))
        if max_len and L >= max_len:
            break
    return out


def run_foreign(ctx, mem, c):
    ri = fc.RecordIndex(c.syms, c.lens)
    qs = fc.foreign_patterns(c, ri)
    blob = c.image()
    keep, img = mem.put(blob)
    n_hits = 0
    with engine.FmIndex(ctx, img, len(blob)) as fm:
        del keep
        for w in (1, 2, 4, 8):
            idx = [i for i, q in enumerate(qs) if fc.fits(q, w)]
            for min_len, max_len, fl in ((1, 0, 0), (2, 3, PROPER)):
                want = [search_records(ri, qs[i], min_len, max_len, fl) for i in idx]
                got, _ = overlaps(fm, mem, "cells", [qs[i] for i in idx], w, min_len, max_len, fl)
                bad = [(qs[i], g[:3], e[:3]) for i, g, e in zip(idx, got, want) if g != e]
                assert not bad, (c.name, w, min_len, max_len, fl, bad[:3])
                n_hits += sum(len(e) for e in want)
    return n_hits
