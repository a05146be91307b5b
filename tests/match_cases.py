"""Shared by tests/test_fm_match_sim.py (serial stand-in) and tests/test_fm_match_gpu.py (HIP library): the longest match that
ends at every query cell (grlbwt_fm_match) and the maximal exact matches (grlbwt_fm_mems), against values from code that shares
nothing with the engine.

  A  collections the engine builds (fm_cases.COLS): the lengths from the TEXT alone -- for each end, lengthen while the piece
     holds no separator and occurs in the text -- the rows from fm_cases.count of the piece itself (tested elsewhere against
     the text), hi - lo against a sliding compare; MEMs from the rule applied to those lengths.
  B  the pattern set is not vacuous (on the brute-force values only).
  C  foreign images (tests/image_cases.py): the greedy backward search by definition on the RECORDS (fm_cases.RecordIndex).
  D  launch shapes: 0, 1, 63, 64, 65 and about 5000 cells, as few long patterns and as many one-cell and empty ones, off[0] > 0.
  E  refusals.

Every output buffer has guard bytes behind it (fm_cases.Mem); the info of every call is checked against its outputs.  The
brute-force values are computed once per process and kept.
"""
import numpy as np
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import image_cases as ic

DT = fc.DT
SHAPES = (0, 1, 63, 64, 65, 5000)
CAPS = (0, 1, 16)
MEM_SETTINGS = [(0, 0), (8, 0), (0, 16), (8, 16)]          # (min_len, max_len)


# ------------------------------------------------------------------ the two calls on a batch, guarded outputs, info checked
def put_batch(mem, patterns, w, lead=0):
    """-> (keepalive, cells pointer, offsets pointer, n_cells); `lead` cells that belong to no pattern come first (off[0] = lead)"""
    cells, off = fc.pack(patterns, w)
    if lead:
        cells = np.concatenate([np.full(lead, 65, dtype=DT[w]), cells])
        off = off + np.uint64(lead)
    kc, pc = mem.put(cells.tobytes())
    ko, po = mem.put(off.tobytes())
    return (kc, ko), pc, po, int(off[-1] - off[0])


def check_info(fm, n_patterns, L, max_len, n_mems):
    info = fm.match_info()
    assert (info["n_patterns"], info["n_cells"], info["n_mems"]) == (n_patterns, len(L), n_mems), info
    assert info["matched_cells"] == int(L.sum(dtype=np.uint64)) and info["longest"] == (int(L.max()) if len(L) else 0), info
    assert info["n_capped"] == (int((L == np.uint64(max_len)).sum()) if max_len else 0), info
    return info


def match(fm, mem, patterns, w, max_len=0, ranges=True, lead=0):
    """grlbwt_fm_match on a batch: (lengths, lo, hi) per cell, lo and hi None without ranges; the info of the call"""
    keep, pc, po, nc = put_batch(mem, patterns, w, lead)
    ln, pl = mem.out(8 * nc)
    lo, plo = mem.out(8 * nc)
    hi, phi = mem.out(8 * nc)
    fm.match(pc, w, po, len(patterns), max_len, pl, plo if ranges else None, phi if ranges else None)
    L = mem.body(ln, 8 * nc).view(np.uint64)
    info = check_info(fm, len(patterns), L, max_len, 0)
    if not ranges:
        assert bool(np.all(mem.get(lo) == fc.FILL)) and bool(np.all(mem.get(hi) == fc.FILL))
        return L, None, None, info
    return L, mem.body(lo, 8 * nc).view(np.uint64), mem.body(hi, 8 * nc).view(np.uint64), info


def mems(fm, mem, patterns, w, min_len, max_len, ranges=True, capacity=None, lead=0):
    """grlbwt_fm_mems on a batch: the entries (pattern, begin, length[, lo, hi]) in the order written"""
    keep, pc, po, nc = put_batch(mem, patterns, w, lead)
    cap = nc if capacity is None else capacity
    bufs = [mem.out(8 * cap) for _ in range(5)]
    ptr = [p for _, p in bufs]
    n = fm.mems(pc, w, po, len(patterns), min_len, max_len, ptr[0], ptr[1], ptr[2], cap, ptr[3] if ranges else None, ptr[4] if ranges else None)
    assert n <= cap
    cols = [mem.body(b, 8 * cap).view(np.uint64)[:n] for b, _ in bufs[:5 if ranges else 3]]
    for b, _ in bufs[:5 if ranges else 3]:
        assert bool(np.all(mem.get(b)[8 * n:] == fc.FILL)), "entries behind the last one were written"
    if not ranges:
        assert bool(np.all(mem.get(bufs[3][0]) == fc.FILL)) and bool(np.all(mem.get(bufs[4][0]) == fc.FILL))
    info = fm.match_info()
    assert (info["n_patterns"], info["n_cells"], info["n_mems"]) == (len(patterns), nc, n), info
    return [tuple(int(c[j]) for c in cols) for j in range(n)]


def mems_by_rule(Ls, min_len, max_len):
    """the rule of the header applied to per-pattern lengths: (pattern, begin, length) in (pattern, end) order"""
    out = []
    floor = max(min_len, 1)
    for i, L in enumerate(Ls):
        if max_len:
            L = [min(v, max_len) for v in L]
        for e, v in enumerate(L):
            if v >= floor and (e + 1 == len(L) or L[e + 1] <= v):
                out.append((i, e + 1 - v, v))
    return out


# ------------------------------------------------------------------ A: by definition, on the text
def non_symbol(col):
    have = set(int(v) for v in np.unique(col.data))
    v = int(col.data.max()) + 1
    if v >= 1 << (8 * col.w):
        v = next(x for x in range(1, 1 << (8 * col.w)) if x not in have)
    return v


def collection_patterns(col):
    """Whole strings; the same with one cell changed; chimeras of two pieces of 20 cells (or the strings' length) of different
    strings; piece + non-symbol + piece + separator + piece; random cells; a pattern longer than any string; [], one body
    symbol, one non-symbol, the separator alone."""
    rng = np.random.default_rng(20261019 + col.n)
    body = sorted(set(int(v) for v in np.unique(col.data)) - {col.sep})
    full = [[int(v) for v in s] for s in col.strings if len(s)]
    longest = max(len(s) for s in full)
    bad = non_symbol(col)
    heavy = longest > 100                     # (one string of 500 cells: a whole string costs 125000 steps uncapped)
    n_whole = 2 if heavy else min(60, 4 * len(full))
    pats = []

    def pick():
        return full[int(rng.integers(len(full)))]

    def piece(m):
        s = pick()
        m = min(m, len(s))
        a = int(rng.integers(0, len(s) - m + 1))
        return s[a:a + m]

    for _ in range(n_whole):
        s = pick()
        pats.append(s)
        q = list(s)
        i = int(rng.integers(len(q)))
        q[i] = [v for v in body + [bad] if v != q[i]][int(rng.integers(len(body)))]
        pats.append(q)
    for _ in range(n_whole // 2):
        pats.append(piece(20) + piece(20))
    for _ in range(max(n_whole * 2 // 5, 2)):
        pats.append(piece(12) + [bad] + piece(9) + [col.sep] + piece(12))
    for _ in range(6):
        vals = body + [bad, col.sep]
        pats.append([vals[int(rng.integers(len(vals)))] if rng.random() < 0.1 else body[int(rng.integers(len(body)))] for _ in range(40)])
    pats.append([body[i % len(body)] for i in range(longest + 3)])
    pats += [[], [body[0]], [bad], [col.sep]]
    return pats


class Expected:
    """lengths (uncapped) per pattern, and for every end with L > 0 the piece and the number of its occurrences"""

    def __init__(self, col):
        self.col, self.pats = col, collection_patterns(col)
        text = col.data.tobytes()
        w, dt = col.w, DT[col.w]

        def positions(p):
            b = np.array(p, dtype=dt).tobytes()
            out, at = [], text.find(b)
            while at >= 0:
                if at % w == 0:
                    out.append(at // w)
                at = text.find(b, at + 1)
            return out

        def occurs(p):
            b = np.array(p, dtype=dt).tobytes()
            at = text.find(b)
            while at >= 0 and at % w:
                at = text.find(b, at + 1)
            return at >= 0

        self.L, self.ends, self.occ = [], [], []               # ends: (pattern, end, length) where the length is not 0
        for i, p in enumerate(self.pats):
            Lp = []
            for e in range(len(p)):
                n = 0
                while n <= e and p[e - n] != col.sep and occurs(p[e - n:e + 1]):
                    n += 1
                Lp.append(n)
                if n:
                    piece = p[e + 1 - n:e + 1]
                    self.ends.append((i, e, n))
                    self.occ.append(len(positions(piece)) if w == 1 else len(col.matches(piece)))
            self.L.append(Lp)
        self.flat = np.array([v for Lp in self.L for v in Lp], dtype=np.uint64)

    def capped(self, max_len):
        return np.minimum(self.flat, np.uint64(max_len)) if max_len else self.flat      # (occurring is monotone in the length)

    def pieces(self, max_len=0):
        """the matched piece of every end whose length is not 0"""
        return [self.pats[i][e + 1 - (min(n, max_len) if max_len else n):e + 1] for i, e, n in self.ends]


_expected = {}


def expected(name):
    if name not in _expected:
        _expected[name] = Expected(fc.COLS[name])
    return _expected[name]


def not_vacuous(ex):
    """B, for the DNA collection: the figures the tests rest on"""
    flat = ex.flat
    n = len(flat)
    assert 3 * int((flat >= 8).sum()) >= n, (int((flat >= 8).sum()), n)
    assert 5 * int((flat >= 16).sum()) >= n, (int((flat >= 16).sum()), n)
    assert int((flat == 0).sum()) >= 40
    assert len(np.unique(flat)) >= 30
    per = {}
    for i, _, _ in mems_by_rule(ex.L, 8, 0):
        per[i] = per.get(i, 0) + 1
    assert sum(1 for v in per.values() if v >= 2) >= 60


def run_collection(ctx, flags, mem, lib, name):
    """A on one collection: lengths and ranges under every cap, without the ranges, as wider cells; MEMs under the four settings"""
    ex = expected(name)
    col, pats = ex.col, ex.pats
    blob = fc.image_of(lib, col, flags)
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob)) as fm:
        del keep
        hit = np.flatnonzero(ex.flat)
        for cap in CAPS:
            rows = fc.count(fm, mem, ex.pieces(cap), col.w)
            if not cap:
                bad = [(p[:8], r, o) for p, r, o in zip(ex.pieces(), rows, ex.occ) if r[1] - r[0] != o or o == 0]
                assert not bad, (name, bad[:5])
            want_lo, want_hi = np.zeros(len(ex.flat), dtype=np.uint64), np.zeros(len(ex.flat), dtype=np.uint64)
            want_lo[hit] = [r[0] for r in rows]
            want_hi[hit] = [r[1] for r in rows]
            Lc, loc, hic, _ = match(fm, mem, pats, col.w, cap)
            assert np.array_equal(Lc, ex.capped(cap)), (name, cap, np.flatnonzero(Lc != ex.capped(cap))[:5])
            assert np.array_equal(loc, want_lo) and np.array_equal(hic, want_hi), (name, cap)
            if not cap:
                L, lo, hi = Lc, loc, hic
        Ln, _, _, _ = match(fm, mem, pats, col.w, 16, ranges=False)
        assert np.array_equal(Ln, ex.capped(16))
        if col.w < 8:                                              # the same patterns as wider cells
            Lw, low, hiw, _ = match(fm, mem, pats, 8, 0)
            assert np.array_equal(Lw, L) and np.array_equal(low, lo) and np.array_equal(hiw, hi)
        first = np.concatenate([[0], np.cumsum([len(p) for p in pats])]).astype(np.int64)
        for min_len, max_len in MEM_SETTINGS:
            want = mems_by_rule(ex.L, min_len, max_len)
            got = mems(fm, mem, pats, col.w, min_len, max_len)
            assert [g[:3] for g in got] == want, (name, min_len, max_len)
            if not max_len:                                        # the rows of the entry's end
                ends = [int(first[i]) + b + m - 1 for i, b, m in want]
                assert [g[3:] for g in got] == [(int(lo[x]), int(hi[x])) for x in ends], (name, min_len)
            assert mems(fm, mem, pats, col.w, min_len, max_len, ranges=False) == want


# ------------------------------------------------------------------ C: by definition, on the records of a foreign image
def foreign_queries(c, ri):
    """fm_cases.foreign_patterns joined, five at a time, into longer queries; the single ones that hold a wide value too"""
    pats = fc.foreign_patterns(c, ri)
    out = [sum(pats[a:a + 5], []) for a in range(0, len(pats), 5)]
    out += [[]] + [p for p in pats if p and max(p) >= 256][:8]
    return out


def greedy(ri, q, e, sep, max_len=0):
    """the longest match ending at cell e of q: RecordIndex's search step while the range stays non-empty"""
    lo, hi, n = 0, ri.n, 0
    while n <= e and (not max_len or n < max_len):
        c = q[e - n]
        if c == sep or c not in ri.per:
            break
        a, b = ri.C[c] + ri.rank(c, lo), ri.C[c] + ri.rank(c, hi)
        if a >= b:
            break
        lo, hi, n = a, b, n + 1
    return (n, lo, hi) if n else (0, 0, 0)


_foreign = {}


def foreign_expected(c):
    if c.name not in _foreign:
        ri = fc.RecordIndex(c.syms, c.lens)
        qs = foreign_queries(c, ri)
        sep = ri.present[0] if ri.present else None
        _foreign[c.name] = (ri, qs, {cap: [[greedy(ri, q, e, sep, cap) for e in range(len(q))] for q in qs] for cap in (0, 2)})
    return _foreign[c.name]


def run_foreign(ctx, mem, c):
    ri, qs, want = foreign_expected(c)
    for q, rows in zip(qs, want[0]):                               # the greedy search agrees with the whole-pattern one
        for e, (n, lo, hi) in enumerate(rows):
            assert not n or ri.search(q[e + 1 - n:e + 1]) == (lo, hi)
    blob = c.image()
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob)) as fm:
        del keep
        for w in (1, 2, 4, 8):
            idx = [i for i, q in enumerate(qs) if fc.fits(q, w)]
            batch = [qs[i] for i in idx]
            for cap in (0, 2):
                flat = [r for i in idx for r in want[cap][i]]
                L, lo, hi, _ = match(fm, mem, batch, w, cap)
                got = list(zip(L.tolist(), lo.tolist(), hi.tolist()))
                bad = [(x, g, e) for x, (g, e) in enumerate(zip(got, flat)) if g != e]
                assert not bad, (c.name, w, cap, bad[:5])
            per = [[r[0] for r in want[0][i]] for i in idx]
            rule = mems_by_rule(per, 2, 0)
            got = mems(fm, mem, batch, w, 2, 0)
            assert [g[:3] for g in got] == rule, (c.name, w)
            assert [g[3:] for g in got] == [want[0][idx[i]][b + m - 1][1:] for i, b, m in rule], (c.name, w)


# ------------------------------------------------------------------ D: launch shapes
def shape_batches(ex, n):
    """n cells as the patterns of A taken in turn (the last one cut short: an end's length depends on the cells in front of it
    alone) with an empty pattern after every third one, and as n patterns of one cell each between empty ones"""
    pats, L = [], []
    left, i = n, 0
    src = [k for k, p in enumerate(ex.pats) if p]
    while left:
        k = src[i % len(src)]
        m = min(left, len(ex.pats[k]))
        pats.append(ex.pats[k][:m])
        L += ex.L[k][:m]
        left -= m
        i += 1
        if i % 3 == 0:
            pats.append([])
    long = (pats + [[]], np.array(L, dtype=np.uint64))
    cells = [v for p in pats for v in p]
    body = set(ex.col.data.tolist()) - {ex.col.sep}
    alone = {v: int(v in body) for v in set(cells)}
    ones = []
    for j, v in enumerate(cells):
        ones += [[v]] + ([[]] * (j % 4 == 0))
    return long, ([[]] + ones, np.array([alone[v] for v in cells], dtype=np.uint64))


def run_shapes(ctx, flags, mem, lib, on_info=None):
    """every shape with and without cells in front of the first pattern; on_info(n, n_patterns, info) sees the launch counters"""
    ex = expected("dna")
    blob = fc.image_of(lib, ex.col, flags)
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob)) as fm:
        for n in SHAPES:
            for pats, want in shape_batches(ex, n):
                for lead in (0, 7):
                    for cap in (0, 16):
                        L, lo, hi, info = match(fm, mem, pats, 1, cap, lead=lead)
                        assert np.array_equal(L, np.minimum(want, np.uint64(cap)) if cap else want), (n, lead, cap)
                        assert bool(np.all((hi > lo) == (L > 0)))
                        if on_info:
                            on_info(n, len(pats), info)
                    per, at = [], 0
                    for p in pats:
                        per.append(want[at:at + len(p)].tolist())
                        at += len(p)
                    got = mems(fm, mem, pats, 1, 0, 0, lead=lead)
                    assert [g[:3] for g in got] == mems_by_rule(per, 0, 0), (n, lead)
        L, lo, hi, info = match(fm, mem, [], 1, 0)                 # no pattern at all
        assert len(L) == 0 and info["walk_lanes"] == 0
        assert mems(fm, mem, [], 1, 0, 0) == []


# ------------------------------------------------------------------ E: refusals
def run_refusals(ctx, flags, mem, lib):
    ex = expected("dna")
    pats = ex.pats[:40]
    nc = sum(len(p) for p in pats)
    blob = fc.image_of(lib, ex.col, flags)
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob)) as fm:
        keepb, pc, po, _ = put_batch(mem, pats, 1)
        outs = [mem.out(8 * nc) for _ in range(5)]
        ptr = [p for _, p in outs]

        def untouched():
            return all(bool(np.all(mem.get(b) == fc.FILL)) for b, _ in outs)

        kd, pd = mem.put(np.array([0, 2, 1, 3], dtype=np.uint64).tobytes())
        for call in (lambda: fm.match(pc, 3, po, len(pats), 0, ptr[0], ptr[1], ptr[2]),                      # a bad width
                     lambda: fm.match(pc, 1, pd, 3, 0, ptr[0], ptr[1], ptr[2]),                              # decreasing offsets
                     lambda: fm.match(pc, 1, po, len(pats), 0, ptr[0], ptr[1], None),                        # lo without hi
                     lambda: fm.match(pc, 1, po, len(pats), 0, ptr[0], None, ptr[2]),
                     lambda: fm.match(None, 1, po, len(pats), 0, ptr[0], ptr[1], ptr[2]),                    # no cells
                     lambda: fm.mems(pc, 0, po, len(pats), 0, 0, ptr[0], ptr[1], ptr[2], nc, ptr[3], ptr[4]),
                     lambda: fm.mems(pc, 1, pd, 3, 0, 0, ptr[0], ptr[1], ptr[2], nc, ptr[3], ptr[4]),
                     lambda: fm.mems(pc, 1, po, len(pats), 0, 0, ptr[0], ptr[1], ptr[2], nc, ptr[3], None),
                     lambda: fm.mems(None, 1, po, len(pats), 0, 0, ptr[0], ptr[1], ptr[2], nc, ptr[3], ptr[4])):
            fc.einval(call)
            assert untouched()
        # a null index
        L = ctx.L
        assert L.grlbwt_fm_match(ctx._h, None, pc, 1, po, len(pats), 0, ptr[0], None, None) == fc.EINVAL
        assert L.grlbwt_fm_mems(ctx._h, None, pc, 1, po, len(pats), 0, 0, ptr[0], ptr[1], ptr[2], None, None, nc, None) == fc.EINVAL
        assert L.grlbwt_fm_match_info_get(None, None) == fc.EINVAL
        assert untouched()
        # one entry too few: the code, the number, nothing written; then the reported capacity is enough
        want = mems_by_rule(ex.L[:40], 8, 0)
        assert len(want) >= 2
        with pytest.raises(engine.GrlbwtError) as e:
            fm.mems(pc, 1, po, len(pats), 8, 0, ptr[0], ptr[1], ptr[2], len(want) - 1, ptr[3], ptr[4])
        assert e.value.code == fc.EINVAL and e.value.n_mems == len(want), (e.value, len(want))
        with pytest.raises(engine.GrlbwtError) as e:              # the sizing call: no arrays at all
            fm.mems(pc, 1, po, len(pats), 8, 0, None, None, None, 0)
        assert e.value.code == fc.EINVAL and e.value.n_mems == len(want)
        assert untouched()
        assert mems(fm, mem, pats, 1, 8, 0, capacity=e.value.n_mems) == [
            w + (int(lo), int(hi)) for w, (lo, hi) in zip(want, fc.count(fm, mem, [pats[i][b:b + m] for i, b, m in want], 1))]
