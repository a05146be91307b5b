"""Shared by tests/test_fm_repeats_sim.py (serial stand-in) and tests/test_fm_repeats_gpu.py (HIP library): the right-maximal and
maximal repeats of a collection from its FM index (grlbwt_fm_repeats).

Expected values share no code with the engine.
  a  the row rules of the header on the LCP BY DEFINITION and the BWT of tests/lcp_cases.Expected: a stack walk over the LCP
     array gives every row its nearest smaller-or-equal value in front and its nearest smaller value behind; a row whose value
     is above the one in front is a split row; left-maximal is "the BWT symbols of the rows are not one symbol other than the
     separator", by prefix sums of the changes
  b  for collections of at most 2000 cells also the SUBSTRING DEFINITION: a dict from every substring to its occurrences, its
     left and its right extensions, string starts and ends as tokens of their own; compared as sorted (len, count, maximal)
  c  the two staircases by the closed forms of the issue: one string A^m has (split, lo, count) = (len + 1, len, m + 1 - len)
     for len = 1 .. m - 1, one string B^m C has (split, lo, count, len) = (p, 1, p, m + 1 - p) for p = 2 .. m, all left-maximal.
     Their images are written by hand: the BWT of A^m is A^m $, that of B^m C is C $ B^m.

The inputs are sized from tile_rows, tree_fanout and tree_levels of a first tiny call, never from constants.  Every output buffer
has guard bytes right behind the entries the call may write; the info of every call is checked against its outputs."""
import ctypes as C

import numpy as np

from grlbwt_amd import engine
from tests import bcr_check as bc
from tests import fm_cases as fc
from tests import image_cases as ic
from tests import lcp_cases as lc
from tests import merge_cases as mc

EINVAL = -22
FILL = fc.FILL
ROWS = ["rows_tile_minus_1", "rows_tile", "rows_tile_plus_1", "rows_three_tiles_17"]
SMALL = ["twice", "one_string", "one_empty_string", "empty_strings", "rare_symbol", "two_bytes", "sigma_256", "wide_u64"]
OUTS = ("lo", "count", "len", "split")


# ------------------------------------------------------------------ expected values
class Table:
    """every right-maximal repeat (split, lo, count, len, maximal) in ascending split row, from lcp and bwt by the row rules (a)"""

    def __init__(self, lcp, bwt, sep, n_strings):
        lcp = [int(v) for v in lcp]
        n = self.n = len(lcp)
        self.n_strings = n_strings
        self.top = max(lcp) if n else 0
        prev, nxt, st = [-1] * n, [n] * n, []
        for p in range(n):
            while st and lcp[st[-1]] > lcp[p]:
                st.pop()
            prev[p] = st[-1] if st else -1
            st.append(p)
        st = []
        for p in range(n - 1, -1, -1):
            while st and lcp[st[-1]] >= lcp[p]:
                st.pop()
            nxt[p] = st[-1] if st else n
            st.append(p)
        bwt = np.asarray(bwt, dtype=np.uint64)
        change = np.zeros(n + 1, dtype=np.int64)                      # change[i]: rows in [1, i) whose symbol differs from the row before
        if n > 1:
            change[2:] = np.cumsum(bwt[1:] != bwt[:-1])
        rows = [p for p in range(1, n) if lcp[p] >= 1 and prev[p] >= 0 and lcp[prev[p]] < lcp[p]]
        self.split = np.array(rows, dtype=np.uint64)
        self.lo = np.array([prev[p] for p in rows], dtype=np.uint64)
        self.count = np.array([nxt[p] - prev[p] for p in rows], dtype=np.uint64)
        self.len = np.array([lcp[p] for p in rows], dtype=np.uint64)
        lo, end = self.lo.astype(np.int64), (self.lo + self.count).astype(np.int64)
        self.maximal = (bwt[lo] == np.uint64(sep)) | (change[end] > change[lo + 1]) if rows else np.zeros(0, dtype=bool)
        assert bool(np.all(self.count >= 2))

    @classmethod
    def closed(cls, split, lo, count, length, n, n_strings, top):
        t = cls.__new__(cls)
        t.n, t.n_strings, t.top = n, n_strings, top
        t.split, t.lo, t.count, t.len = (np.asarray(a, dtype=np.uint64) for a in (split, lo, count, length))
        t.maximal = np.ones(len(t.split), dtype=bool)
        return t

    def bounds(self, min_len=1, max_len=0):
        m = self.len >= max(min_len, 1)
        return m & (self.len <= max_len) if max_len else m

    def select(self, min_len=1, max_len=0, min_count=2, max_count=0, maximal=False, rb=0, re=None):
        re = self.n if re is None else min(re, self.n)
        m = self.bounds(min_len, max_len) & (self.count >= max(min_count, 2)) & (self.split >= rb) & (self.split < re)
        if max_count:
            m &= self.count <= max_count
        if maximal:
            m &= self.maximal
        return m


def by_substrings(cells):
    """(b): sorted (len, count, left-maximal) of the right-maximal repeats, from every substring with its extensions"""
    vals, inv = np.unique(np.asarray(cells), return_inverse=True)
    seen = {}
    for si, s in enumerate(lc.split(inv.astype(np.int64))):
        s = tuple(int(v) for v in s)
        for i in range(len(s)):
            left = s[i - 1] if i else ("start", si)
            for j in range(i + 1, len(s) + 1):
                e = seen.setdefault(s[i:j], [0, set(), set()])
                e[0] += 1
                e[1].add(left)
                e[2].add(s[j] if j < len(s) else ("end", si, i))
    return sorted((len(w), e[0], len(e[1]) >= 2) for w, e in seen.items() if len(e[2]) >= 2)


class Case:
    def __init__(self, name, cells, w):
        self.name, self.cells, self.w = name, cells, w
        self._tab = None

    @property
    def tab(self):
        if self._tab is None:
            e = lc.Expected(self.cells)
            self.bwt = e.bwt
            t = self._tab = Table(e.lcp, e.bwt, e.sep, e.k)
            if t.n <= 2000:
                assert sorted(zip(t.len.tolist(), t.count.tolist(), t.maximal.tolist())) == by_substrings(self.cells), self.name
        return self._tab


def both_kinds():
    """strings that share XAB and also hold AB behind another cell: AB is maximal, XAB and XA are right-maximal only where X is
    always behind the same cell"""
    s = [b"QXABC", b"QXABD", b"YABE", b"ZABF", b"QXAG", b"AB", b"", b"QXABC"]
    return mc.text([np.frombuffer(x, dtype=np.uint8) for x in s], 10, 1)


_cases = {}


def cases(T):
    if T not in _cases:
        P = {n: Case(n, c.cells, c.w) for n, c in lc.cases(T).items() if n in ROWS + SMALL}
        P["both_kinds"] = Case("both_kinds", both_kinds(), 1)
        _cases[T] = P
    return _cases[T]


def a_staircase(m, max_len=0):
    """(image, table) of one string A^m; with max_len only the repeats up to that length"""
    top = min(max_len, m - 1) if max_len else m - 1
    ln = np.arange(1, top + 1, dtype=np.uint64)
    tab = Table.closed(ln + 1, ln, m + 1 - ln, ln, m + 1, 1, m - 1)
    return ic.make_image(1, 4, [65, 10], [m, 1]), tab


def b_staircase(m):
    p = np.arange(2, m + 1, dtype=np.uint64)
    tab = Table.closed(p, np.ones(len(p)), p, m + 1 - p, m + 2, 1, m - 1)
    return ic.make_image(1, 4, [67, 10, 66], [1, 1, m]), tab


def shape(ctx, mem, lib, flags):
    """(tile_rows, tree_fanout) from a first tiny call"""
    blob = mc.build(lib, flags, np.frombuffer(b"AC\nA\n", dtype=np.uint8), 1)
    keep, p = mem.put(blob)
    with engine.FmIndex(ctx, p, len(blob)) as fm:
        assert fm.repeats_raw() == 1                                   # "A", twice
        i = fm.repeat_info()
    assert i["tree_fanout"] >= 2 and i["tile_rows"] >= i["tree_fanout"] and i["tile_rows"] % 64 == 0 and i["tree_levels"] == 1, i
    return i["tile_rows"], i["tree_fanout"]


def levels_of(n, fanout):
    """levels of the tree, the values' included: up to the first that is a single node"""
    levels = 1
    while n > fanout:
        n, levels = -(-n // fanout), levels + 1
    return levels


def image(lib, flags, c):
    blob = mc.build(lib, flags, c.cells, c.w)
    t = c.tab
    assert np.array_equal(mc.decode(blob), c.bwt), c.name             # the rows are the sorted suffixes
    return blob, t


def open_case(ctx, flags, mem, lib, name, **kw):
    T, F = shape(ctx, mem, lib, flags)
    c = cases(T)[name]
    blob, t = image(lib, flags, c)
    keep, img = mem.put(blob)
    return c, t, engine.FmIndex(ctx, img, len(blob), **kw), (T, F)


# ------------------------------------------------------------------ one call, guarded outputs, everything checked
def call(fm, mem, t, min_len=1, max_len=0, min_count=2, max_count=0, maximal=False, rb=0, re=None, outs=OUTS, fanout=None):
    """grlbwt_fm_repeats with buffers of exactly the expected size, guards right behind; everything it wrote and its info against `t`.
    (A table by a closed form under max_len holds no longer repeats: its bounds are the call's.)"""
    sel = t.select(min_len, max_len, min_count, max_count, maximal, rb, re)
    m = int(sel.sum())
    bufs = {o: mem.out(8 * m) for o in OUTS}
    ptr = {o: bufs[o][1] if o in outs else None for o in OUTS}
    got = fm.repeats_raw(min_len, max_len, min_count, max_count, engine.FM_REPEATS_MAXIMAL if maximal else 0, rb, re,
                         ptr["lo"], ptr["count"], ptr["len"], ptr["split"], m)
    assert got == m, (got, m)
    info = fm.repeat_info()
    inb = t.bounds(min_len, max_len)
    assert (info["n_rows"], info["n_strings"], info["min_len"], info["max_len"]) == (t.n, t.n_strings, max(min_len, 1), max_len), info
    assert info["passes"] == (min(t.top, max_len) if max_len else t.top), (info, t.top)
    assert (info["n_repeats"], info["n_maximal"], info["n_selected"]) == (int(inb.sum()), int((inb & t.maximal).sum()), m), info
    assert info["longest"] == (int(t.len[inb].max()) if inb.any() else 0), info
    assert info["largest_count"] == (int(t.count[inb].max()) if inb.any() else 0), info
    cap = max_len + 1 if max_len and max_len < 2 ** 32 - 1 else 2 ** 32 - 1
    assert info["value_bytes"] == (1 if cap < 2 ** 8 else 2 if cap < 2 ** 16 else 4), info
    assert info["tile_rows"] == info["tree_fanout"] ** 2 and info["tree_levels"] == levels_of(t.n, info["tree_fanout"]), info
    assert info["scratch_bytes"] >= t.n * info["value_bytes"], info
    if not mem.on_gpu:
        assert info["far_searches"] == 0, info
    for o in OUTS:
        if o in outs:
            have = mem.body(bufs[o][0], 8 * m).view(np.uint64)
            want = getattr(t, o)[sel]
            assert np.array_equal(have, want), (o, np.flatnonzero(have != want)[:5], have[:5], want[:5])
        else:
            assert bool(np.all(mem.get(bufs[o][0]) == FILL)), o
    return info


# ------------------------------------------------------------------ the cases
def run_collection(ctx, flags, mem, lib, name):
    """case 1: the whole table of one collection, the maximal ones, and a few filters"""
    c, t, fm, _ = open_case(ctx, flags, mem, lib, name)
    with fm:
        info = call(fm, mem, t)
        call(fm, mem, t, maximal=True)
        call(fm, mem, t, min_len=2, max_len=3, min_count=3)
        if name in ("one_string", "one_empty_string", "empty_strings"):
            assert info["n_repeats"] == 0
        if name == "twice":
            assert len(t.count) and all(int(v) % 2 == 0 for v in t.count)
            whole = set(len(s) for s in lc.split(c.cells))
            assert whole & set(int(v) for v in t.len)                   # whole strings are repeats
        if name in ROWS:
            assert info["n_repeats"] > info["n_maximal"] > 0
    return info


def run_sizes_follow_the_shape(ctx, flags, mem, lib):
    T, F = shape(ctx, mem, lib, flags)
    P = cases(T)
    assert [len(P[n].cells) for n in ROWS] == [T - 1, T, T + 1, 3 * T + 17]
    assert len(P["wide_u64"].cells) <= 2000 and len(P["sigma_256"].cells) <= 2000 and len(P["both_kinds"].cells) <= 2000     # (b) runs
    t = P["both_kinds"].tab
    assert bool(t.maximal.any()) and not bool(t.maximal.all())


def run_staircases(ctx, flags, mem, lib, deep):
    """case 2: every forward search of A^m ends at the last row, every backward search of B^m C at row 1"""
    T, F = shape(ctx, mem, lib, flags)
    m = 3 * T
    for blob, t in (a_staircase(m), b_staircase(m)):
        keep, img = mem.put(blob)
        with engine.FmIndex(ctx, img, len(blob)) as fm:
            info = call(fm, mem, t)
            assert info["n_repeats"] == info["n_maximal"] == m - 1 and info["longest"] == m - 1 and info["largest_count"] == m
            assert (info["far_searches"] > 0) == mem.on_gpu, info
            call(fm, mem, t, min_len=T - 1, max_len=T + 1, rb=T, re=2 * T + 1)
    # a search that crosses a whole node of the first level above the tiles, and of the level above where there is one: the
    # forward searches of A^m, with max_len so that the passes stay few (the capped rows lie between a row and the last)
    sizes = [F * T + 5]
    if deep and F * F * T + 5 <= 2 ** 25:
        sizes.append(F * F * T + 5)
    for m in sizes:
        blob, t = a_staircase(m, 9)
        keep, img = mem.put(blob)
        with engine.FmIndex(ctx, img, len(blob)) as fm:
            info = call(fm, mem, t, max_len=9)
            assert info["tree_levels"] >= 4 and info["passes"] == 9 and info["value_bytes"] == 1, info
            assert info["n_repeats"] == 9 and (info["far_searches"] > 0) == mem.on_gpu, info
            call(fm, mem, t, min_len=3, max_len=9, maximal=True, outs=("count",))


def run_filters(ctx, flags, mem, lib):
    """case 3"""
    c, t, fm, _ = open_case(ctx, flags, mem, lib, "rows_tile_plus_1")
    with fm:
        assert t.top > 7
        for lens in ((2, 0), (1, 1), (3, 3), (2, 7), (t.top, 0), (t.top + 1, 0), (1, t.top), (1, 255), (1, 256), (1, 2 ** 16), (5, 2 ** 63)):
            info = call(fm, mem, t, min_len=lens[0], max_len=lens[1])
            if lens[1] and lens[1] < t.top:
                assert info["passes"] <= lens[1]
        base = call(fm, mem, t)
        for mc_ in (0, 1, 2):
            assert call(fm, mem, t, min_count=mc_)["n_selected"] == base["n_selected"]
        big = int(t.count.max())
        assert 0 < call(fm, mem, t, min_count=3)["n_selected"] < base["n_selected"]
        assert 0 < call(fm, mem, t, min_count=3, max_count=big - 1)["n_selected"]
        call(fm, mem, t, max_count=2)
        call(fm, mem, t, min_count=big + 1)
        call(fm, mem, t, min_len=2, max_len=6, min_count=3, max_count=9, maximal=True)
    c, t, fm, _ = open_case(ctx, flags, mem, lib, "both_kinds")
    with fm:
        both = call(fm, mem, t)
        only = call(fm, mem, t, maximal=True)
        assert 0 < only["n_selected"] == both["n_maximal"] < both["n_selected"]
    # a foreign image with neighbouring records of one symbol is answered by symbols
    c, t, fm, _ = open_case(ctx, flags, mem, lib, "rows_tile_plus_1")
    fm.close()
    blob, _ = image(lib, flags, c)
    cut = mc.split_runs(ctx, mem, blob, 2, 7)
    _, _, sym, ln = bc.parse_rl_bwt(cut)
    assert int((ln == 0).sum()) > 0 and not bc.runs_are_maximal(sym)
    keep, img = mem.put(cut)
    with engine.FmIndex(ctx, img, len(cut)) as fm:
        call(fm, mem, t)
        call(fm, mem, t, maximal=True)


def run_windows(ctx, flags, mem, lib):
    """case 4"""
    c, t, fm, (T, F) = open_case(ctx, flags, mem, lib, "rows_three_tiles_17")
    with fm:
        cuts = [0, 1, t.n_strings, T - 1, T - 1, T + 64, 2 * T + 5, t.n]         # (an empty window among them)
        total = 0
        for a, b in zip(cuts, cuts[1:]):
            total += call(fm, mem, t, rb=a, re=b)["n_selected"]
        assert total == len(t.split)
        assert call(fm, mem, t, rb=t.n, re=engine.UINT64_MAX)["n_selected"] == 0   # clamped to [n, n): empty
        # the emit takes 64 selected rows per wave at a time (the library has no entry tile to report): selections around tree_fanout entries
        assert len(t.split) > F + 8
        for m in (F - 1, F, F + 1):
            assert call(fm, mem, t, re=int(t.split[m]))["n_selected"] == m
            assert call(fm, mem, t, rb=int(t.split[7]), re=int(t.split[7 + m]))["n_selected"] == m
            assert call(fm, mem, t, maximal=True, re=int(t.split[t.maximal][m]))["n_selected"] == m


def run_outputs_and_sizing(ctx, flags, mem, lib):
    """case 5"""
    c, t, fm, _ = open_case(ctx, flags, mem, lib, "rows_tile")
    L = ctx.L
    with fm:
        for outs in (("lo",), ("count",), ("len",), ("split",), ("lo", "split"), ()):
            call(fm, mem, t, min_len=2, outs=outs)
        sel = t.select(min_len=2)
        m = int(sel.sum())
        assert fm.repeats_raw(2) == m                                   # the sizing call
        bufs = [mem.out(8 * m) for _ in range(4)]
        for which in ((0, 1, 2, 3), (0,), (1,), (2,), (3,)):
            p = [C.c_void_p(bufs[i][1]) if i in which else None for i in range(4)]
            got = C.c_uint64(0)
            rc = L.grlbwt_fm_repeats(ctx._h, fm._h, 2, 0, 2, 0, 0, 0, engine.UINT64_MAX, p[0], p[1], p[2], p[3], m - 1, C.byref(got))
            assert rc == EINVAL and got.value == m and "GRLBWT" not in L.grlbwt_last_error(ctx._h).decode()
            assert all(bool(np.all(mem.get(b) == FILL)) for b, _ in bufs)
            assert fm.repeat_info()["n_selected"] == m                  # the call got as far as counting
        lo, count, length = fm.repeats(min_len=2)                       # the binding sizes by the idiom
        assert np.array_equal(lo, t.lo[sel]) and np.array_equal(count, t.count[sel]) and np.array_equal(length, t.len[sel])
        sel = t.select(1, 5, 3, 0, True, int(t.split[3]), int(t.split[-2]))
        got = fm.repeats(max_len=5, min_count=3, maximal=True, rows=(int(t.split[3]), int(t.split[-2])), split=True)
        assert len(got) == 4 and all(np.array_equal(g, getattr(t, o)[sel]) for g, o in zip(got, ("lo", "count", "len", "split")))


def run_refusals(ctx, flags, mem, lib):
    """case 6"""
    c, t, fm, _ = open_case(ctx, flags, mem, lib, "rows_tile_minus_1")
    L = ctx.L
    m = len(t.split)
    bufs = [mem.out(8 * m + 8) for _ in range(4)]
    p = [b[1] for b in bufs]

    def untouched():
        return all(bool(np.all(mem.get(b) == FILL)) for b, _ in bufs)

    def refused(fn):
        msg = fc.einval(fn)
        assert "GRLBWT" not in msg and "GRLBWT" not in L.grlbwt_last_error(ctx._h).decode() and untouched(), msg
        return msg

    with fm:
        for flags_ in (2, 3, 2 ** 31):
            refused(lambda: fm.repeats_raw(flags=flags_, lo_ptr=p[0], capacity=m))                          # unknown flag bits
        refused(lambda: fm.repeats_raw(3, 2, lo_ptr=p[0], capacity=m))                                      # max_len below min_len
        refused(lambda: fm.repeats_raw(5, 4, lo_ptr=p[0], capacity=m))
        refused(lambda: fm.repeats_raw(row_begin=5, row_end=4, lo_ptr=p[0], capacity=m))
        refused(lambda: fm.repeats_raw(row_begin=t.n + 1, lo_ptr=p[0], capacity=m))                         # above the clamped end
        assert L.grlbwt_fm_repeats(ctx._h, fm._h, 1, 0, 2, 0, 0, 0, engine.UINT64_MAX, None, None, None, None, 0, None) == EINVAL    # no output at all
        assert "GRLBWT" not in L.grlbwt_last_error(ctx._h).decode()
        for i in range(4):                                                                                  # an array not aligned to 8
            q = [C.c_void_p(x + (4 if j == i else 0)) for j, x in enumerate(p)]
            got = C.c_uint64(99)
            assert L.grlbwt_fm_repeats(ctx._h, fm._h, 1, 0, 2, 0, 0, 0, engine.UINT64_MAX, q[0], q[1], q[2], q[3], m, C.byref(got)) == EINVAL
            assert got.value == 0 and "GRLBWT" not in L.grlbwt_last_error(ctx._h).decode() and untouched()
        got = C.c_uint64(99)                                                                                # a null index
        q = [C.c_void_p(x) for x in p]
        assert L.grlbwt_fm_repeats(ctx._h, None, 1, 0, 2, 0, 0, 0, engine.UINT64_MAX, q[0], q[1], q[2], q[3], m, C.byref(got)) == EINVAL and got.value == 0
        assert L.grlbwt_fm_repeat_info_get(None, None) == EINVAL and L.grlbwt_fm_repeat_info_get(fm._h, None) == EINVAL
        assert untouched()
    bad = ic.make_image(1, 1, [10, 65], [1, 2])              # not the BWT of a collection: the row of the second A is LF of itself
    keep, img = mem.put(bad)
    with engine.FmIndex(ctx, img, len(bad)) as fm:
        msg = refused(lambda: fm.repeats_raw(lo_ptr=p[0], count_ptr=p[1], len_ptr=p[2], split_ptr=p[3], capacity=m))
        assert "not the BWT of a collection" in msg, msg


def run_index_unchanged(ctx, flags, mem, lib):
    """case 7"""
    col = fc.COLS["dna"]
    pats = fc.collection_patterns(col)
    blob = fc.image_of(lib, col, flags)
    t = Case("dna", col.data, 1).tab
    for kw in ({}, {"locate": True}, {"locate": True, "checkpoints": True, "sample_bits": 3}, {"locate": True, "extract": True}):
        keep, img = mem.put(blob)
        with engine.FmIndex(ctx, img, len(blob), **kw) as fm:
            del keep
            before, counts = fm.info(), fc.count(fm, mem, pats, 1)
            buf, ptr = mem.out(t.n)
            lcp_before = (fm.lcp(0, 1, ptr), mem.body(buf, t.n).tobytes())
            call(fm, mem, t)
            call(fm, mem, t, min_len=2, max_len=4, maximal=True)
            assert fm.info() == before and fc.count(fm, mem, pats, 1) == counts, kw
            buf, ptr = mem.out(t.n)
            after = (fm.lcp(0, 1, ptr), mem.body(buf, t.n).tobytes())
            assert lcp_before[1] == after[1] and all(np.array_equal(a, b) for a, b in zip(lcp_before[0], after[0]))


def extract(fm, mem, strings, begins, ends):
    """grlbwt_fm_extract of a batch of ranges: a list of tuples of cells"""
    n = len(strings)
    keep = [mem.put(np.asarray(a, dtype=np.uint64).tobytes()) for a in (strings, begins, ends)]
    cap = int(sum(int(e) - int(b) for b, e in zip(begins, ends)))
    out, po = mem.out(cap)
    off, poff = mem.out(8 * (n + 1))
    got = fm.extract(keep[0][1], keep[1][1], keep[2][1], n, 1, po, cap, poff)
    cells, offs = mem.body(out, cap)[:got], mem.body(off, 8 * (n + 1)).view(np.uint64)
    return [tuple(int(v) for v in cells[int(a):int(b)]) for a, b in zip(offs, offs[1:])]


def run_cross_check(ctx, flags, mem, lib):
    """case 8: every entry against locate, extract and count of the same index"""
    c, t, fm, _ = open_case(ctx, flags, mem, lib, "rows_tile_minus_1", locate=True, extract=True)
    with fm:
        lo, count, length, split = fm.repeats(split=True)
        assert np.array_equal(split, t.split) and len(lo) > 100
        s, o = fc.locate(fm, mem, lo)
        words = extract(fm, mem, s, o, o + length)
        assert all(len(w) == int(l) and 10 not in w for w, l in zip(words, length))
        assert fc.count(fm, mem, [list(w) for w in words], 1) == [(int(a), int(a + b)) for a, b in zip(lo, count)]
        s2, o2 = fc.locate(fm, mem, lo + count - np.uint64(1))
        first, last = extract(fm, mem, s, o, o + length + np.uint64(1)), extract(fm, mem, s2, o2, o2 + length + np.uint64(1))
        for a, b, l in zip(first, last, length):                        # the two ends of the range go on differently, or a string ends
            assert a[:int(l)] == b[:int(l)] and (a[-1] != b[-1] or a[-1] == 10), (a, b)


def run_foreign(ctx, mem, c):
    """case 9: an image the engine did not make is refused or answered, and never runs past the guards; returns (answered, refused)"""
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
        for kw in ({}, {"max_len": 3}, {"min_len": 2, "flags": engine.FM_REPEATS_MAXIMAL}):
            try:
                m = fm.repeats_raw(**kw)
            except engine.GrlbwtError as e:
                assert e.code == EINVAL, e
                refused += 1
                continue
            assert m < max(n, 1) and fm.repeat_info()["n_selected"] == m
            bufs = [mem.out(8 * m) for _ in range(4)]
            assert fm.repeats_raw(lo_ptr=bufs[0][1], count_ptr=bufs[1][1], len_ptr=bufs[2][1], split_ptr=bufs[3][1], capacity=m, **kw) == m
            lo, cnt, ln, sp = (mem.body(b, 8 * m).view(np.uint64) for b, _ in bufs)
            assert bool(np.all(lo < sp)) and bool(np.all(sp < lo + cnt)) and bool(np.all(lo + cnt <= n)) and bool(np.all(sp[1:] > sp[:-1]))
            assert bool(np.all(ln >= kw.get("min_len", 1)))
            done += 1
    return done, refused
