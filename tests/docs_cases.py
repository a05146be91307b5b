"""Shared by tests/test_fm_docs_sim.py (serial stand-in) and tests/test_fm_docs_gpu.py (HIP library): the strings behind row
ranges of an FM index (grlbwt_docs_create / grlbwt_docs_count / grlbwt_docs_list).

The expected values come from the TEXT, never from the engine: the document array is sa_cases.expected(col)[0] (a sort of the
suffixes), and the answer for a range [lo, hi) is np.unique(DA[lo:hi], return_index=True, return_counts=True) ordered by index.
The one exception is the foreign images (7), whose document array is grlbwt_fm_sa's own: there is no text to sort.  Every output
buffer has guard bytes on both sides (the out / body / untouched helpers of sa_cases).

  1  the ranges grlbwt_fm_count gives for the patterns of every collection, both index forms: count, list with all four arrays
  2  shapes that can break a tile kernel
  3  one output at a time
  4  occurrences, and what the flag costs
  5  refusals, before any store
  6  the index is unchanged, and the handle outlives it
  7  foreign images (tests/image_cases.py, by the callers)
"""
import ctypes as C

import numpy as np
import pytest

from grlbwt_amd import engine
from tests import fm_cases as fc
from tests import sa_cases as sc
from tests import walk_cases as wk

EINVAL = -22
FORMS = (None, 2, 6)             # None: form 0, an index without checkpoints; else form 1 at these sample_bits
FORM_IDS = ["strings", "segments_b2", "segments_b6"]
TILE = 2048


def make_reads():
    """3000 reads of 40 cells from a genome of 600: every one-cell pattern's range spans 13 to 16 tiles and holds all 3000 strings"""
    rng = np.random.default_rng(20261021)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rng.integers(0, 4, size=600)]
    at = rng.integers(0, 561, size=3000)
    data = np.full((3000, 41), 10, dtype=np.uint8)
    data[:, :40] = genome[at[:, None] + np.arange(40)]
    col = fc.Collection("reads3000", data.reshape(-1), 1)
    # the properties the cases lean on, so that they cannot silently degrade
    assert col.n == 123000 and len(col.strings) == 3000
    per = np.stack([(data[:, :40] == c).sum(axis=1) for c in acgt])             # occurrences of each cell value in each read
    sizes = per.sum(axis=1)
    assert int(sizes.min()) == 26549 and int(sizes.max()) == 31543               # rows of the four one-cell ranges
    assert all(13 <= -(-int(s) // TILE) <= 16 for s in sizes)
    assert int(per.min()) >= 1                                                    # each range holds all 3000 documents
    assert sorted(int(v) for v in per.max(axis=1)) == [14, 15, 17, 19]          # the most occurrences in one document
    return col


READS = make_reads()
COLS = {n: wk.COLS[n] for n in ("dna", "identical", "mixed", "repeats", "wide_u64")}
COLS[sc.SINGLES.name] = sc.SINGLES
COLS[READS.name] = READS
NAMES = list(COLS)
assert max(c.n for c in COLS.values()) < 420000


def da_of(col):
    return sc.expected(col)[0]


# ------------------------------------------------------------------ expected values, from the text
def answer(da, lo, hi):
    """(strings, first rows, occurrences) of [lo, hi) in ascending first row"""
    v, i, c = np.unique(da[lo:hi], return_index=True, return_counts=True)
    o = np.argsort(i, kind="stable")
    return v[o].astype(np.uint64), (i[o] + lo).astype(np.uint64), c[o].astype(np.uint64)


class Expect:
    def __init__(self, da, ranges):
        S, F, O, R, off = [], [], [], [], [0]
        for r, (lo, hi) in enumerate(ranges):
            v, f, c = answer(da, lo, hi)
            S.append(v), F.append(f), O.append(c), R.append(np.full(len(v), r, dtype=np.uint64))
            off.append(off[-1] + len(v))
        z = np.zeros(0, dtype=np.uint64)
        self.string, self.first, self.occ, self.range = (np.concatenate(x) if x else z for x in (S, F, O, R))
        self.offsets = np.array(off, dtype=np.uint64)
        self.ndocs = np.diff(self.offsets)
        self.total = off[-1]
        self.rows = sum(hi - lo for lo, hi in ranges)
        self.largest = max([hi - lo for lo, hi in ranges], default=0)
        self.most = int(self.ndocs.max(initial=0))


# ------------------------------------------------------------------ one call, guarded outputs
def put_ranges(mem, ranges):
    a = np.array(ranges, dtype=np.uint64).reshape(-1, 2)
    klo, plo = mem.put(np.ascontiguousarray(a[:, 0]).tobytes())
    khi, phi = mem.put(np.ascontiguousarray(a[:, 1]).tobytes())
    return (klo, khi), plo, phi


def count(docs, mem, ranges):
    keep, plo, phi = put_ranges(mem, ranges)
    nr = len(ranges)
    nb, pn = sc.out(mem, 8 * nr)
    total = docs.count(plo, phi, nr, pn)
    return sc.body(mem, nb, 8 * nr).view(np.uint64), total


def listing(docs, mem, ranges, capacity, first=True, occ=True, rng=True):
    """grlbwt_docs_list -> (entry_offsets, string, first_row, occ, range, n_entries); an array that is not asked for comes back as
    None, its buffer checked for the fill"""
    keep, plo, phi = put_ranges(mem, ranges)
    nr = len(ranges)
    eb, pe = sc.out(mem, 8 * (nr + 1))
    bufs = [sc.out(mem, 8 * capacity) for _ in range(4)]
    want = (True, first, occ, rng)
    ptr = [p if w else None for (b, p), w in zip(bufs, want)]
    ne = docs.list(plo, phi, nr, pe, ptr[0], capacity, ptr[1], ptr[2], ptr[3])
    assert ne <= capacity
    outs = []
    for (b, p), w in zip(bufs, want):
        if not w:
            assert sc.untouched(mem, b)
            outs.append(None)
            continue
        h = sc.body(mem, b, 8 * capacity)
        assert bool(np.all(h[8 * ne:] == sc.FILL)), "words behind the last entry were written"
        outs.append(h[:8 * ne].view(np.uint64))
    return (sc.body(mem, eb, 8 * (nr + 1)).view(np.uint64),) + tuple(outs) + (ne,)


def check_create(info, col, flags, bits, occ):
    n, k = col.n, len(col.strings)
    w = 8 if flags & engine.FLAG_FORCE_IDX64 else 4
    assert (info["n_rows"], info["n_strings"], info["flags"], info["idx_bytes"]) == (n, k, engine.DOCS_OCCURRENCES if occ else 0, w), info
    assert info["held_bytes"] == (2 * n + (n + k + 1 if occ else 0)) * w, info
    assert info["sort_bits"] == wk.ceil_log2(k), info
    assert info["form"] == (0 if bits is None else 1) and info["walk_steps"] == n - k, info      # one step per row, less the rows walks stop at
    assert info["scratch_bytes"] > 0 and info["tile_entries"] == TILE, info


def check_query(info, ranges, e):
    assert (info["n_ranges"], info["n_range_rows"], info["n_entries"]) == (len(ranges), e.rows, e.total), info
    assert (info["largest_range"], info["most_docs"]) == (e.largest, e.most), info


def check(col, docs, mem, ranges, occ=True):
    """count and list of one batch against the text, and what the info states of each"""
    ranges = [(int(a), int(b)) for a, b in ranges]
    e = Expect(da_of(col), ranges)
    nd, total = count(docs, mem, ranges)
    assert total == e.total, (col.name, total, e.total)
    bad = np.flatnonzero(nd != e.ndocs)
    assert not len(bad), (col.name, bad[:5], nd[bad[:5]], e.ndocs[bad[:5]])
    check_query(docs.info(), ranges, e)
    eoff, s, f, o, r, ne = listing(docs, mem, ranges, total, occ=occ)
    assert ne == e.total
    assert np.array_equal(eoff, e.offsets), (col.name, eoff[:8], e.offsets[:8])
    for got, want, what in ((s, e.string, "string"), (f, e.first, "first_row"), (o, e.occ, "occ"), (r, e.range, "range")):
        if got is None:
            continue
        bad = np.flatnonzero(got != want)
        assert not len(bad), (col.name, what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    check_query(docs.info(), ranges, e)
    return e


def counted_ranges(fm, mem, col):
    return fc.count(fm, mem, wk.patterns_of(col) if col.name in wk.COLS else fc.collection_patterns(col), col.w)


# ------------------------------------------------------------------ 1: ranges of counted patterns
def run_counted(ctx, flags, mem, lib, name, bits):
    col = COLS[name]
    with sc.index(ctx, flags, mem, lib, col, bits) as fm:
        ranges = counted_ranges(fm, mem, col)
        assert (0, col.n) in ranges and (0, 0) in ranges           # the empty pattern; a pattern that does not occur
        with fm.documents(occurrences=True) as docs:
            check_create(docs.info(), col, flags, bits, True)
            e = check(col, docs, mem, ranges)
            assert e.most == len(col.strings) and e.largest == col.n
            check_create(docs.info(), col, flags, bits, True)


# ------------------------------------------------------------------ 2: shapes that can break a tile kernel
def shape_batches(col, T):
    n, k = col.n, len(col.strings)
    assert n > 100 + 3 * T + 17 and k >= 2
    rng = np.random.default_rng(n)
    out = [[(0, 0), (n, n), (0, n), (0, k), (k - 1, k + 1), (T - 1, T + 1), (0, T), (T, 2 * T), (n - 1, n)]]
    lo = rng.integers(0, n, size=5000)
    small = [(int(a), int(a) + int(s)) for a, s in zip(lo, rng.integers(0, 2, size=5000))]
    rows = np.cumsum([b - a for a, b in small])
    assert int((rows < T).sum()) > 256 and 1 < -(-int(rows[-1]) // T) <= 3      # more than 256 range starts, empties included, in the first tile
    out.append(small)
    out.append([(0, T // 2), (100, 100 + 3 * T + 17), (5, 9)])                  # the second range begins in tile 0 and ends in tile 3
    a, b = n // 3, n // 3 + 700
    out.append([(a, b)] * 5 + [(a + 10, b + 10), (a + 5, b - 5), (n - 100, n), (n // 2, n // 2 + 300), (50, 400), (0, 60)])
    return out


def run_shapes(ctx, flags, mem, lib, name, bits):
    col = COLS[name]
    with sc.index(ctx, flags, mem, lib, col, bits) as fm, fm.documents(occurrences=True) as docs, fm.documents() as plain:
        T = docs.info()["tile_entries"]
        for batch in shape_batches(col, T):
            check(col, docs, mem, batch)
            check(col, plain, mem, batch, occ=False)               # (on the device a list without occurrences is the tile emit's, one with them the generic emit's)
        if name == "mixed":                                        # the whole collection: 370 000 rows, 5 documents
            assert -(-col.n // T) > 180 and len(col.strings) == 5
            e = check(col, docs, mem, [(0, col.n)])
            assert e.total == 5
            check(col, plain, mem, [(0, col.n)], occ=False)


# ------------------------------------------------------------------ 3: one output at a time
def run_one_output(ctx, flags, mem, lib, name, bits):
    col = COLS[name]
    with sc.index(ctx, flags, mem, lib, col, bits) as fm, fm.documents(occurrences=True) as docs:
        ranges = counted_ranges(fm, mem, col)
        e = Expect(da_of(col), ranges)
        nd, total = count(docs, mem, ranges)
        for first, occ, rng in ((True, False, False), (False, True, False), (False, False, True), (False, False, False)):
            eoff, s, f, o, r, ne = listing(docs, mem, ranges, total, first=first, occ=occ, rng=rng)
            assert ne == total == e.total and np.array_equal(np.diff(eoff), nd) and np.array_equal(s, e.string)
            assert (f is None) == (not first) and (o is None) == (not occ) and (r is None) == (not rng)
            assert f is None or np.array_equal(f, e.first)
            assert o is None or np.array_equal(o, e.occ)
            assert r is None or np.array_equal(r, e.range)
        # room to spare: the words behind the last entry stay as they were (listing checks it)
        eoff, s, f, o, r, ne = listing(docs, mem, ranges, total + 77)
        assert ne == total and np.array_equal(s, e.string) and np.array_equal(o, e.occ)
        # no range at all
        nd0, t0 = count(docs, mem, [])
        assert t0 == 0 and len(nd0) == 0
        eoff, s, f, o, r, ne = listing(docs, mem, [], 4)
        assert ne == 0 and list(eoff) == [0] and docs.info()["n_ranges"] == 0


# ------------------------------------------------------------------ 4: occurrences
def run_occurrences(ctx, flags, mem, lib, name, bits):
    col = COLS[name]
    n, k = col.n, len(col.strings)
    w = 8 if flags & engine.FLAG_FORCE_IDX64 else 4
    body = sorted(set(int(v) for v in np.unique(col.data)) - {col.sep})
    with sc.index(ctx, flags, mem, lib, col, bits) as fm:
        ranges = fc.count(fm, mem, [[c] for c in body] + [[body[0], body[1]], []], col.w) + [(n // 4, 3 * n // 4), (k, n), (0, k)]
        with fm.documents(occurrences=True) as docs, fm.documents() as plain:
            e = check(col, docs, mem, ranges)
            if name == "repeats":
                assert k == 2 and int(e.occ.max()) > 5000           # thousands of occurrences per document
            else:
                assert 14 <= int(e.occ[e.range < 4].max()) <= 19 and int(e.ndocs[:4].min()) == k
            check_create(plain.info(), col, flags, bits, False)
            assert docs.info()["held_bytes"] - plain.info()["held_bytes"] == (n + k + 1) * w
            check(col, plain, mem, ranges, occ=False)               # everything but the occurrences
            # dev_occ on a handle made without the flag: refused, every buffer untouched
            keep, plo, phi = put_ranges(mem, ranges)
            bufs = [sc.out(mem, 8 * (len(ranges) + 1))] + [sc.out(mem, 8 * e.total) for _ in range(4)]
            msg = fc.einval(lambda: plain.list(plo, phi, len(ranges), bufs[0][1], bufs[1][1], e.total, bufs[2][1], bufs[3][1], bufs[4][1]))
            assert "occurrence" in msg, msg
            assert all(sc.untouched(mem, b) for b, p in bufs)


# ------------------------------------------------------------------ 5: refusals, before any store
def run_refusals(ctx, flags, mem, lib, bits):
    col = COLS["dna"]
    n = col.n
    L = ctx.L
    blob = fc.image_of(lib, col, flags)
    keep, img = mem.put(blob)
    with engine.FmIndex(ctx, img, len(blob)) as nolocate:          # an index without the locate structures
        msg = fc.einval(lambda: nolocate.documents())
        assert "locating" in msg, msg
    with sc.index(ctx, flags, mem, lib, col, bits) as fm:
        h = C.c_void_p(1)
        assert L.grlbwt_docs_create(ctx._h, fm._h, 2, C.byref(h)) == EINVAL and not h.value        # unknown flag bits
        h = C.c_void_p(1)
        assert L.grlbwt_docs_create(ctx._h, fm._h, 0x101, C.byref(h)) == EINVAL and not h.value
        h = C.c_void_p(1)
        assert L.grlbwt_docs_create(ctx._h, None, 0, C.byref(h)) == EINVAL and not h.value         # a null index
        assert L.grlbwt_docs_info_get(None, None) == EINVAL
        with fm.documents(occurrences=True) as docs:
            good = [(0, n), (3, 40), (7, 7)]
            e = Expect(da_of(col), good)
            nb, pn = sc.out(mem, 8 * 3)
            eb, pe = sc.out(mem, 8 * 4)
            arr = [sc.out(mem, 8 * e.total) for _ in range(4)]
            ps, pf, po, pr = (p for b, p in arr)
            got = C.c_uint64(99)

            def clean():
                return all(sc.untouched(mem, b) for b in [nb, eb] + [b for b, p in arr])

            for bad, word in (([(0, n), (5, 4), (7, 7)], "range 1"), ([(0, n), (3, 40), (0, n + 1)], "range 2"),
                              ([(n + 1, n + 1), (2, 1)], "range 0")):
                keep2, plo, phi = put_ranges(mem, bad)
                msg = fc.einval(lambda: docs.count(plo, phi, len(bad), pn))
                assert word in msg, msg                              # the message names the first such range
                msg = fc.einval(lambda: docs.list(plo, phi, len(bad), pe, ps, e.total, pf, po, pr))
                assert word in msg, msg
                assert clean()
            keep2, plo, phi = put_ranges(mem, good)
            vp = C.c_void_p
            assert L.grlbwt_docs_count(ctx._h, None, vp(plo), vp(phi), 3, vp(pn), C.byref(got)) == EINVAL and got.value == 0      # a null handle
            assert L.grlbwt_docs_list(ctx._h, None, vp(plo), vp(phi), 3, vp(pe), vp(ps), vp(pf), vp(po), vp(pr), e.total, C.byref(got)) == EINVAL
            fc.einval(lambda: docs.count(plo, phi, 3, None))         # a missing output
            fc.einval(lambda: docs.list(plo, phi, 3, None, ps, e.total, pf, po, pr))
            fc.einval(lambda: docs.list(plo, phi, 3, pe, None, e.total, pf, po, pr))
            assert clean()
            with pytest.raises(engine.GrlbwtError) as err:           # capacity one short: the count is still reported
                docs.list(plo, phi, 3, pe, ps, e.total - 1, pf, po, pr)
            assert err.value.code == EINVAL and err.value.n_entries == e.total, err.value
            assert clean()
            check(col, docs, mem, good)                              # the handle still answers


# ------------------------------------------------------------------ 6: the index is unchanged, and the handle outlives it
def run_index_unchanged(ctx, flags, mem, lib):
    """after sa_cases.run_index_unchanged: info (index_bytes), a count batch and a locate batch, before and after"""
    col = COLS["dna"]
    n = col.n
    pats = fc.collection_patterns(col)
    rows = (np.arange(500, dtype=np.uint64) * np.uint64(7919)) % np.uint64(n)
    blob = fc.image_of(lib, col, flags)
    for kw in ({"locate": True}, {"locate": True, "checkpoints": True, "sample_bits": 3}, {"locate": True, "extract": True},
               {"locate": True, "checkpoints": True, "sample_bits": 3, "extract": True}):
        keep, img = mem.put(blob)
        fm = engine.FmIndex(ctx, img, len(blob), **kw)
        del keep
        before, counts = fm.info(), fc.count(fm, mem, pats, 1)
        s0, o0 = fc.locate(fm, mem, rows)
        docs = fm.documents(occurrences=True)
        check(col, docs, mem, counts)
        assert fm.info() == before and fc.count(fm, mem, pats, 1) == counts, kw
        s1, o1 = fc.locate(fm, mem, rows)
        assert s1.tobytes() == s0.tobytes() and o1.tobytes() == o0.tobytes(), kw
        fc.dna_rows(fm, mem, col)
        fm.close()                                                   # the handle holds no pointer into the index
        junk = [mem.put(bytes(1 << 16)) for _ in range(4)]         # (memory the index gave back is handed out again)
        check(col, docs, mem, counts)
        docs.close()
        del junk


# ------------------------------------------------------------------ 7: foreign images
def run_foreign(ctx, mem, c):
    """Where FmIndex(locate=True) succeeds, documents() succeeds exactly when grlbwt_fm_sa's array has no "none" -- and then agrees
    with unique over that array -- and else refuses with EINVAL: rows lie on no chain.  This is the one check that leans on an
    engine output.  Returns (handles made, handles refused)."""
    blob = c.image()
    made = refused = 0
    for bits in sc.FOREIGN_BITS:
        keep, img = mem.put(blob)
        kw = {} if bits is None else dict(checkpoints=True, sample_bits=bits)
        try:
            fm = engine.FmIndex(ctx, img, len(blob), locate=True, **kw)
        except engine.GrlbwtError as e:
            assert e.code == EINVAL, e
            continue
        with fm:
            n = fm.info()["n_syms"]
            if n == 0:
                continue
            da, _, _ = sc.call(fm, mem, n, sa=False)
            lost = int((da == np.uint64(fc.NONE)).sum())
            if lost:
                msg = fc.einval(lambda: fm.documents(occurrences=True))
                assert "not the BWT of a collection" in msg, msg
                refused += 1
                continue
            with fm.documents(occurrences=True) as docs:
                rng = np.random.default_rng(n)
                a = rng.integers(0, n + 1, size=40)
                b = rng.integers(0, n + 1, size=40)
                ranges = [(0, n), (0, 0), (n, n)] + [(int(min(x, y)), int(max(x, y))) for x, y in zip(a, b)]
                e = Expect(da, ranges)
                nd, total = count(docs, mem, ranges)
                assert total == e.total and np.array_equal(nd, e.ndocs), (c.name, bits)
                eoff, s, f, o, r, ne = listing(docs, mem, ranges, total)
                assert np.array_equal(eoff, e.offsets) and np.array_equal(s, e.string) and np.array_equal(f, e.first), (c.name, bits)
                assert np.array_equal(o, e.occ) and np.array_equal(r, e.range), (c.name, bits)
                made += 1
    return made, refused
